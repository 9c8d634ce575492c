"""Time the full-mesh LBS export kernels alone (for rocprofv3): python tools/lbs_bench.py [F] [reps] [model] [--shape E] [--repeats N] [--f64]
--f64: the f64 export (moshii_lbs_forward[_shape]_f64) instead of the f32 one.
--shape E: the export with per-frame coefficients of a free shape block of E columns (moshii_lbs_forward_shape_f32) -- the body gets E
extra shapedirs columns (a unit coefficient moves a vertex by up to 1 cm), the coefficients are N(0, 1); same poses otherwise.
--repeats N: N timed rounds of `reps` calls each, one line per round (run-to-run spread).
--normals [F] [reps] [--model NAME]: vertex normals and virtual markers of exported meshes on the triangulated synthetic body of the
family (synth.synth_mesh_model, seed 1000; default smplh, 4000 frames): the export alone, the normals alone through the LDS kernel
and through the gather kernel, export + normals, and the virtual-marker call for 53 markers -- HIP events on device buffers, us and the
fraction of 8 TB/s under F V 24 B + the face table.
--surface-distance [F] [reps] [--model NAME]: the signed marker-to-skin distance of 53 points a frame on the same body: the staged f32
kernel, the gather kernel in f32 and f64, and the fused entry (export + distance, meshes in the handle's scratch) -- ms, point-triangle
tests per second and the share of the f32 vector peak the tests' arithmetic comes to.
--joints [F] [--model NAME]: posed joints and world joint rotations (moshii_joints_*) of F frames (default 4000, smplh) on device
buffers, f32 and f64, with and without the rotations: HIP events around one call, median of 20 after 3 warm-ups, the launch shape and
the bytes moved; beside it moshii_lbs_forward_f32 on the same frames, timed the same way.
--render [F] [--size W] [--model NAME]: shaded previews (moshii_render_f32) of F frames (default 256, smplh) at W x W (default 512) with
53 + 53 markers on device buffers, one fitted camera: HIP events around one call, median of 10 after 3 warm-ups -- the export alone, the
normals alone, the render call (normals + k_render_project + k_render_tiles) and, as the difference of the last two, project + tiles;
ms per frame each, and the fused moshii_render_posed_f32 for the whole chain."""
import ctypes as C, sys, time
import numpy as np
sys.path.insert(0, '.')


def normals_bench(argv):
    import os
    import torch
    from moshpp_amd import synth, workload
    mt = 'smplh'
    if '--model' in argv:
        i = argv.index('--model')
        mt = argv[i + 1]
        del argv[i:i + 2]
    F = int(argv[0]) if len(argv) > 0 else 4000
    reps = int(argv[1]) if len(argv) > 1 else 10
    M = {'smplh': 53, 'smpl': 41, 'smplx': 89, 'mano': 33}[mt]
    dd = synth.synth_mesh_model(mt, seed=1000)
    job = workload.make_job(mt, 8, M, seed=1000, optimize_fingers=(mt == 'mano'), dd=dd)
    solver = workload.make_solver(job)
    model, sm = solver.dev, job['sm']
    faces = np.asarray(dd['f'], dtype=np.int32)
    model.set_faces(faces)
    V = sm.V
    good = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    table = (V + 1) * 4 + 3 * int(good.sum()) * (4 if V <= 65535 else 8)
    val = np.bincount(faces.ravel(), minlength=V)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    pose = torch.from_numpy(rng.normal(0, 0.3, (F, sm.NP)).astype(np.float32)).to(dev)
    trans = torch.from_numpy(rng.normal(0, 1, (F, 3)).astype(np.float32)).to(dev)
    verts = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
    vids = rng.choice(V, 53, replace=False).astype(np.int32)
    dist = np.full(53, 0.0095)
    mk = torch.empty((F, 53, 3), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    export = lambda: model.lbs_forward_device(F, pose.data_ptr(), trans.data_ptr(), verts.data_ptr(), stream)
    nrm = lambda: model.vertex_normals_device(F, verts.data_ptr(), normals.data_ptr(), stream)
    both = lambda: (export(), nrm())
    vm = lambda: model.virtual_markers_device(F, pose.data_ptr(), trans.data_ptr(), vids, dist, mk.data_ptr(), None, stream)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):              # three rounds: the spread
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3 / reps)
        return min(ts), max(ts)

    print(f'{mt} mesh body: V = {V}, {len(faces)} faces, valence {val.min()} .. {val.max()}, face table {table / 1e3:.1f} KB, F = {F}, '
          f'{reps} calls a round, 3 rounds (fastest .. slowest round); library {os.path.basename(capi.LIB_PATH)} {capi.load().moshii_source_hash().decode()}')
    nb = F * V * 24 + table
    legs = [('export alone', export, F * V * 12, 'F V 12 B'), ('normals, LDS kernel', nrm, nb, 'F V 24 B + table')]
    for name, fn, nbytes, what in legs:
        lo, hi = timed(fn)
        print(f'  {name:34s} {lo * 1e6:8.1f} .. {hi * 1e6:8.1f} us   {nbytes / lo / 8e12 * 100:5.1f} % of 8 TB/s under {what}')
    kname, klds, kthreads = capi.last_launch_info()
    assert kname == 'k_vn_lds', kname
    print(f'  ({kname}: {klds} B of LDS a workgroup, {kthreads} threads)')
    os.environ['MOSHII_VN_KERNEL'] = 'gather'
    lo, hi = timed(nrm)
    del os.environ['MOSHII_VN_KERNEL']
    assert capi.last_launch_info()[0] == 'k_vn_gather<float>', capi.last_launch_info()
    print(f'  {"normals, gather kernel":34s} {lo * 1e6:8.1f} .. {hi * 1e6:8.1f} us   {nb / lo / 8e12 * 100:5.1f} % of 8 TB/s under F V 24 B + table')
    lo, hi = timed(both)
    print(f'  {"export + normals":34s} {lo * 1e6:8.1f} .. {hi * 1e6:8.1f} us   {(F * V * 36 + table) / lo / 8e12 * 100:5.1f} % of 8 TB/s under F V 36 B + table')
    lo, hi = timed(vm)
    print(f'  {"virtual markers, 53 markers":34s} {lo * 1e6:8.1f} .. {hi * 1e6:8.1f} us   (meshes in the handle\'s scratch; {F * 53 * 12 / 1e6:.1f} MB reach the caller)')
    ref = model.vertex_normals(verts[:2].cpu().numpy())
    print(f'  check: device-buffer normals vs the host-buffer call on 2 frames: max |diff| {np.abs(normals[:2].cpu().numpy() - ref).max():.1e}')


def surface_distance_bench(argv):
    import os
    import torch
    from moshpp_amd import synth, workload
    mt = 'smplh'
    if '--model' in argv:
        i = argv.index('--model')
        mt = argv[i + 1]
        del argv[i:i + 2]
    F = int(argv[0]) if len(argv) > 0 else 4000
    reps = int(argv[1]) if len(argv) > 1 else 5
    N = 53
    dd = synth.synth_mesh_model(mt, seed=1000)
    job = workload.make_job(mt, 8, {'smplh': 53, 'smpl': 41, 'smplx': 89, 'mano': 33}[mt], seed=1000, optimize_fingers=(mt == 'mano'), dd=dd)
    solver = workload.make_solver(job)
    model, sm = solver.dev, job['sm']
    faces = np.asarray(dd['f'], dtype=np.int32)
    model.set_faces(faces)
    V, NF = sm.V, len(faces)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    pose = torch.from_numpy(rng.normal(0, 0.3, (F, sm.NP)).astype(np.float32)).to(dev)
    trans = torch.from_numpy(rng.normal(0, 1, (F, 3)).astype(np.float32)).to(dev)
    verts = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    model.lbs_forward_device(F, pose.data_ptr(), trans.data_ptr(), verts.data_ptr(), stream)
    torch.cuda.synchronize()
    # the points: markers about a centimetre off the skin -- 53 vertices of each frame, moved by up to 1.5 cm
    vids = torch.from_numpy(rng.choice(V, N, replace=False)).to(dev)
    points = (verts[:, vids] + torch.from_numpy(rng.uniform(-0.015, 0.015, (F, N, 3)).astype(np.float32)).to(dev)).contiguous()
    dist = torch.empty((F, N), dtype=torch.float32, device=dev)
    face = torch.empty((F, N), dtype=torch.int32, device=dev)
    part = torch.empty((F, N), dtype=torch.int32, device=dev)
    near = torch.empty((F, N, 3), dtype=torch.float32, device=dev)
    F64 = min(F, 1000)                            # (the f64 leg on fewer frames: it is the slow one)
    verts64, points64 = verts[:F64].double(), points[:F64].double()
    dist64 = torch.empty((F64, N), dtype=torch.float64, device=dev)
    near64 = torch.empty((F64, N, 3), dtype=torch.float64, device=dev)
    plain = lambda: model.surface_distance_device(F, verts.data_ptr(), N, points.data_ptr(), dist.data_ptr(), face.data_ptr(), part.data_ptr(),
                                                  near.data_ptr(), stream)
    plain64 = lambda: model.surface_distance_device(F64, verts64.data_ptr(), N, points64.data_ptr(), dist64.data_ptr(), face.data_ptr(),
                                                    part.data_ptr(), near64.data_ptr(), stream, f32=False)
    fused = lambda: model.marker_surface_distance_device(F, pose.data_ptr(), trans.data_ptr(), N, points.data_ptr(), dist.data_ptr(),
                                                         face.data_ptr(), part.data_ptr(), near.data_ptr(), stream)
    export = lambda: model.lbs_forward_device(F, pose.data_ptr(), trans.data_ptr(), verts.data_ptr(), stream)

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):              # three rounds: the spread
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3 / reps)
        return min(ts), max(ts)

    OPS = 75                                      # f32 operations of one point-triangle test in sd_search (fma = 2), counted from the source
    print(f'{mt} mesh body: V = {V}, {NF} faces, F = {F} frames x {N} points = {F * N * NF / 1e9:.2f} G point-triangle tests, {reps} calls a round, '
          f'3 rounds (fastest .. slowest round); library {os.path.basename(capi.LIB_PATH)} {capi.load().moshii_source_hash().decode()}')

    def line(name, lo, hi, frames, peak=True):
        tests = frames * N * NF
        extra = f'   {tests * OPS / lo / 157.3e12 * 100:5.1f} % of the 157.3 TFLOPS f32 vector peak at {OPS} flop a test' if peak else ''
        print(f'  {name:38s} {lo * 1e3:9.3f} .. {hi * 1e3:9.3f} ms   {tests / lo / 1e9:8.1f} G tests/s{extra}')

    os.environ['MOSHII_SD_KERNEL'] = 'lds'
    lo, hi = timed(plain)
    del os.environ['MOSHII_SD_KERNEL']
    kname, klds, kthreads = capi.last_launch_info()
    assert kname == 'k_sd_lds', kname
    line('staged f32 kernel (k_sd_lds)', lo, hi, F)
    print(f'  ({kname}: {klds} B of LDS a workgroup, {kthreads} threads)')
    staged = dist.clone()
    lo_g, hi_g = timed(plain)
    assert capi.last_launch_info()[0] == 'k_sd_gather<float>', capi.last_launch_info()
    line('gather f32 kernel (the default)', lo_g, hi_g, F)
    same = bool((staged == dist).all() | (torch.isnan(staged) & torch.isnan(dist)).all())
    print(f'  (the two f32 kernels agree bit for bit: {same}; staged / gather time {lo / lo_g:.2f})')
    lo, hi = timed(plain64)
    assert capi.last_launch_info()[0] == 'k_sd_gather<double>', capi.last_launch_info()
    line(f'gather f64 kernel ({F64} frames)', lo, hi, F64, peak=False)
    lo, hi = timed(export)
    print(f'  {"export alone":38s} {lo * 1e3:9.3f} .. {hi * 1e3:9.3f} ms')
    lo, hi = timed(fused)
    line('fused entry (export + distance, default)', lo, hi, F, peak=False)
    ref = model.surface_distance(verts[:2].cpu().numpy(), points[:2].cpu().numpy())
    plain()
    torch.cuda.synchronize()
    print(f'  check: device-buffer distances vs the host-buffer call on 2 frames: max |diff| {np.abs(dist[:2].cpu().numpy() - ref.distance).max():.1e}; '
          f'|d| median {float(dist.abs().median()) * 1e3:.2f} mm, {float((dist < 0).float().mean()) * 100:.1f} % inside')


def joints_bench(argv):
    import os
    import torch
    from moshpp_amd import synth, workload
    mt = 'smplh'
    if '--model' in argv:
        i = argv.index('--model')
        mt = argv[i + 1]
        del argv[i:i + 2]
    F = int(argv[0]) if len(argv) > 0 else 4000
    job = workload.make_job(mt, 8, {'smplh': 53, 'smpl': 41, 'smplx': 89, 'mano': 33}[mt], seed=1000, optimize_fingers=(mt == 'mano'),
                            dd=synth.synth_model(mt, seed=1000))
    solver = workload.make_solver(job)
    model, sm = solver.dev, job['sm']
    K, V, NP = sm.K, sm.V, sm.NP
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    pose_h, trans_h = rng.normal(0, 0.3, (F, NP)), rng.normal(0, 1, (F, 3))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):                      # HIP events around ONE call, median of 20 after 3 warm-ups
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return np.median(ts), min(ts), max(ts)

    print(f'{mt}: K = {K} joints, NP = {NP} pose variables, V = {V}, F = {F} frames, device buffers, HIP events around one call, median of 20 '
          f'calls after 3 warm-ups (fastest .. slowest); library {os.path.basename(capi.LIB_PATH)} {capi.load().moshii_source_hash().decode()}')
    keep = {}
    for dt, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        isz = np.dtype(dt).itemsize
        pose = torch.from_numpy(pose_h.astype(dt)).to(dev)
        trans = torch.from_numpy(trans_h.astype(dt)).to(dev)
        joints = torch.empty((F, K, 3), dtype=tdt, device=dev)
        rot = torch.empty((F, K, 3, 3), dtype=tdt, device=dev)
        for with_rot in (True, False):
            fn = lambda: model.posed_joints_device(F, pose.data_ptr(), trans.data_ptr(), joints.data_ptr(), rot.data_ptr() if with_rot else None,
                                                   stream, f32=dt == np.float32)
            med, lo, hi = timed(fn)
            kname, klds, kthreads = capi.last_launch_info()
            nbytes = F * (NP + 3) * isz + F * K * (12 if with_rot else 3) * isz
            print(f'  {kname:18s} {"joints + rotations" if with_rot else "joints alone":20s} {med:8.1f} us ({lo:.1f} .. {hi:.1f})   grid {(F + 3) // 4} x {kthreads} threads '
                  f'(one wave a frame), {klds} B LDS; {nbytes / 1e6:.2f} MB moved (in {F * (NP + 3) * isz / 1e6:.2f}, out {(nbytes - F * (NP + 3) * isz) / 1e6:.2f}) '
                  f'-> {nbytes / med / 1e3:.1f} GB/s')
        keep[dt] = (pose, trans, joints.cpu().numpy(), rot.cpu().numpy())
    pose, trans = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (pose_h, trans_h))
    verts = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
    med, lo, hi = timed(lambda: model.lbs_forward_device(F, pose.data_ptr(), trans.data_ptr(), verts.data_ptr(), stream))
    print(f'  for scale: moshii_lbs_forward_f32 on the same frames {med:8.1f} us ({lo:.1f} .. {hi:.1f}), {F * V * 12 / 1e6:.1f} MB out')
    ref = model.posed_joints(pose_h[:2].astype(np.float32), trans_h[:2].astype(np.float32), dtype=np.float32)
    print(f'  check: device-buffer joints vs the host-buffer call on 2 frames: max |diff| {np.abs(keep[np.float32][2][:2] - ref).max():.1e}; '
          f'f32 vs f64 joints on all frames: max |diff| {np.abs(keep[np.float32][2] - keep[np.float64][2]).max():.1e} m')


def render_bench(argv):
    import os
    import torch
    from moshpp_amd import preview, synth, workload
    mt, W = 'smplh', 512
    for flag in ('--model', '--size'):
        if flag in argv:
            i = argv.index(flag)
            if flag == '--model':
                mt = argv[i + 1]
            else:
                W = int(argv[i + 1])
            del argv[i:i + 2]
    F = int(argv[0]) if len(argv) > 0 else 256
    M = {'smplh': 53, 'smpl': 41, 'smplx': 89, 'mano': 33}[mt]
    dd = synth.synth_mesh_model(mt, seed=1000)
    job = workload.make_job(mt, 8, M, seed=1000, optimize_fingers=(mt == 'mano'), dd=dd)
    solver = workload.make_solver(job)
    model, sm = solver.dev, job['sm']
    faces = np.asarray(dd['f'], dtype=np.int32)
    model.set_faces(faces)
    V, NF, N = sm.V, len(faces), 2 * 53
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    pose_h = rng.normal(0, 0.3, (F, sm.NP)).astype(np.float32)
    trans_h = rng.normal(0, 0.1, (F, 3)).astype(np.float32)
    cam = preview.preview_camera(model.posed_joints(pose_h, trans_h, dtype=np.float32), (W, W), view=(20.0, 10.0), up='y')
    vids = rng.choice(V, 53, replace=False)
    pts_h = np.zeros((F, N, 3), dtype=np.float32)
    pose, trans = torch.from_numpy(pose_h).to(dev), torch.from_numpy(trans_h).to(dev)
    verts = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((F, V, 3), dtype=torch.float32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    export = lambda: model.lbs_forward_device(F, pose.data_ptr(), trans.data_ptr(), verts.data_ptr(), stream)
    nrm = lambda: model.vertex_normals_device(F, verts.data_ptr(), normals.data_ptr(), stream)
    export(); nrm()
    torch.cuda.synchronize()
    vh, nh = verts[:, vids].cpu().numpy(), normals[:, vids].cpu().numpy()
    pts_h[:, :53] = vh + 0.0095 * nh                       # markers where a solve would put them: on the skin, 9.5 mm out
    pts_h[:, 53:] = vh + 0.0095 * nh + rng.normal(0, 0.004, vh.shape).astype(np.float32)
    pts = torch.from_numpy(pts_h).to(dev)
    prgb = np.array([preview.OBSERVED_RGB] * 53 + [preview.SIMULATED_RGB] * 53, dtype=np.uint8)
    rgb = torch.empty((F, W, W, 3), dtype=torch.uint8, device=dev)
    ids = torch.empty((F, W, W), dtype=torch.int32, device=dev)
    depth = torch.empty((F, W, W), dtype=torch.float32, device=dev)
    kw = dict(N=N, points_ptr=pts.data_ptr(), point_rgb=prgb, point_radius=0.0095, rgb_ptr=rgb.data_ptr(), ids_ptr=ids.data_ptr(),
              depth_ptr=depth.data_ptr(), stream=stream)
    render = lambda: model.render_device(F, verts.data_ptr(), cam, (W, W), **kw)
    fused = lambda: model.render_posed_device(F, pose.data_ptr(), trans.data_ptr(), cam, (W, W), **kw)

    def timed(fn):                      # HIP events around ONE call, median of 10 after 3 warm-ups
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return np.median(ts), min(ts), max(ts)

    print(f'{mt} mesh body: V = {V}, {NF} faces, {N} markers, F = {F} frames at {W} x {W}, one camera, rgb + ids + depth, device buffers, HIP events '
          f'around one call, median of 10 calls after 3 warm-ups (fastest .. slowest); library {os.path.basename(capi.LIB_PATH)} '
          f'{capi.load().moshii_source_hash().decode()}')
    res = {}
    for name, fn in (('export (moshii_lbs_forward_f32)', export), ('normals (moshii_vertex_normals_f32)', nrm),
                     ('render call: normals + project + tiles', render), ('fused: export + normals + project + tiles', fused)):
        med, lo, hi = timed(fn)
        res[name] = med
        print(f'  {name:44s} {med:9.3f} ms ({lo:.3f} .. {hi:.3f})   {med / F * 1e3:9.2f} us a frame')
    kname, klds, kthreads = capi.last_launch_info()
    tiles = ((W + 31) // 32) ** 2
    pt = res['render call: normals + project + tiles'] - res['normals (moshii_vertex_normals_f32)']
    feed = res['export (moshii_lbs_forward_f32)'] + res['normals (moshii_vertex_normals_f32)']
    print(f'  ({kname}: {tiles} tiles x {F} frames = {tiles * F} workgroups of {kthreads} threads, {klds} B of LDS each; {(NF + N + 1023) // 1024} list chunks a tile)')
    print(f'  project + tiles (render call - normals)      {pt:9.3f} ms   {pt / F:9.4f} ms a frame')
    print(f'  export + normals that feed them              {feed:9.3f} ms   {feed / F:9.4f} ms a frame')
    print(f'  the rasteriser costs {pt / feed:.1f} x the export and normals it consumes')
    torch.cuda.synchronize()
    host = model.render(verts[:2].cpu().numpy(), cam, (W, W), points=pts_h[:2], point_rgb=prgb, point_radius=0.0095)
    same = all(np.array_equal(host[k], a[:2].cpu().numpy()) for k, a in (('rgb', rgb), ('ids', ids), ('depth', depth)))
    i0 = ids[0].cpu().numpy()
    print(f'  check: device-buffer call vs the host-buffer call on 2 frames: {"same bits" if same else "DIFFERENT"}; frame 0: background '
          f'{100 * (i0 < 0).mean():.1f} %, body {100 * ((i0 >= 0) & (i0 < NF)).mean():.1f} %, markers {100 * (i0 >= NF).mean():.2f} %')


if '--render' in sys.argv:
    from moshpp_amd import capi
    sys.argv.remove('--render')
    render_bench(sys.argv[1:])
    sys.exit(0)
if '--joints' in sys.argv:
    from moshpp_amd import capi
    sys.argv.remove('--joints')
    joints_bench(sys.argv[1:])
    sys.exit(0)
if '--surface-distance' in sys.argv:
    from moshpp_amd import capi
    sys.argv.remove('--surface-distance')
    surface_distance_bench(sys.argv[1:])
    sys.exit(0)
if '--normals' in sys.argv:
    from moshpp_amd import capi
    sys.argv.remove('--normals')
    normals_bench(sys.argv[1:])
    sys.exit(0)
E_SHAPE, REPEATS = 0, 1
F64 = '--f64' in sys.argv          # time moshii_lbs_forward[_shape]_f64 instead of the f32 export
if F64:
    sys.argv.remove('--f64')
for flag in ('--shape', '--repeats'):
    if flag in sys.argv:
        i = sys.argv.index(flag)
        val = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        if flag == '--shape':
            E_SHAPE = val
        else:
            REPEATS = val
import torch
from moshpp_amd import capi, workload
F = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
mt = sys.argv[3] if len(sys.argv) > 3 else 'smplh'
M = {'smplh': 53, 'smpl': 41, 'smplx': 89, 'mano': 33}[mt]
# LBS_BODY=mesh: the synthetic body with the vertex order of a registered mesh (bone by bone, along each bone) instead of shuffled ids
import os
from moshpp_amd import synth
order = os.environ.get('LBS_BODY', 'shuffled')
if os.environ.get('LBS_V'):   # (experiment: another vertex count, e.g. 6912 = 108 x 64: 128-byte-aligned output rows)
    synth.MODEL_DIMS = dict(synth.MODEL_DIMS); synth.MODEL_DIMS[mt] = (int(os.environ['LBS_V']), synth.MODEL_DIMS[mt][1])
if E_SHAPE:
    dd = dict(synth.synth_model(mt, seed=1000, vertex_order=order, num_betas=16 + E_SHAPE))
    sd = np.array(dd['shapedirs'], dtype=np.float64)
    sd[:, :, 16:] *= 0.01 / np.maximum(np.abs(sd[:, :, 16:]).max(axis=(0, 1), keepdims=True), 1e-12)
    dd['shapedirs'] = sd
    job = workload.make_job(mt, 8, M, seed=1000, optimize_fingers=(mt == 'mano'), dd=dd, num_betas=16 + E_SHAPE)
else:
    job = workload.make_job(mt, 8, M, seed=1000, optimize_fingers=(mt == 'mano'), dd=synth.synth_model(mt, seed=1000, vertex_order=order))
solver = workload.make_solver(job)
if E_SHAPE:
    solver.dev.set_free_shape(16, E_SHAPE)
sm = job['sm']
dev = torch.device('cuda', 0)
rng = np.random.default_rng(0)
NPDT = np.float64 if F64 else np.float32
pose_h = rng.normal(0, 0.3, (F, sm.NP)).astype(NPDT)
if os.environ.get('LBS_HANDS') == 'still':   # a body-only Stage-II result (the reference's default): the hand-pose variables are the same in every frame
    pose_h[:, sm.body_dof:] = 0.0
pose = torch.from_numpy(pose_h).to(dev)
trans = torch.from_numpy(rng.normal(0, 1, (F, 3)).astype(NPDT)).to(dev)
verts = torch.empty((F, sm.V, 3), dtype=torch.float64 if F64 else torch.float32, device=dev)
stream = torch.cuda.current_stream().cuda_stream
shape_h = rng.normal(0, 1, (F, max(E_SHAPE, 1))).astype(NPDT)
shape = torch.from_numpy(shape_h).to(dev)
if E_SHAPE:
    run = lambda: solver.dev.lbs_forward_device(F, pose.data_ptr(), trans.data_ptr(), verts.data_ptr(), C.c_void_p(stream), shape_ptr=shape.data_ptr(), f32=not F64)
else:
    run = lambda: solver.dev.lbs_forward_device(F, pose.data_ptr(), trans.data_ptr(), verts.data_ptr(), C.c_void_p(stream), f32=not F64)
for _ in range(3):
    run()
torch.cuda.synchronize()
out_bytes = F * sm.V * (24 if F64 else 12)
for _ in range(REPEATS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) * 1e-3 / reps
    print(f'{mt} {"f64" if F64 else "f32"} [{order} vertex order{", still hands" if os.environ.get("LBS_HANDS") == "still" else ""}{f", {E_SHAPE} shape coefficients" if E_SHAPE else ""}] F={F}: {t*1e6:.1f} us per call, output {out_bytes/1e6:.1f} MB -> {out_bytes/t/1e9:.0f} GB/s ({out_bytes/t/8e12*100:.1f}% of 8 TB/s), {F/t:.0f} frames/s')

if os.environ.get('LBS_CHECK'):
    ref = solver.dev.lbs_forward(pose[:40].cpu().numpy().astype(np.float64), trans[:40].cpu().numpy().astype(np.float64),
                                 shape=shape_h[:40].astype(np.float64) if E_SHAPE else None)
    got = verts[:40].cpu().numpy()
    print(f'  check vs the f64 kernel on 40 frames: max |diff| {np.abs(got - ref).max():.2e} m')
if int(os.environ.get('MOSHII_LBS_STOP', '0')) & 16:
    torch.cuda.synchronize()
    lib = capi.load()
    lib.moshii_internal_l32.restype = C.c_void_p
    lib.moshii_internal_l32.argtypes = [C.c_void_p]
    buf_ = (C.c_longlong * 1024)()
    lib.moshii_internal_lbs_debug_times.argtypes = [C.c_void_p, C.c_void_p]
    lib.moshii_internal_lbs_debug_times(lib.moshii_internal_l32(solver.dev.handle), buf_)
    raw = np.array(buf_[:], dtype=np.int64)
    st = raw[:192].reshape(8, 24)
    ps = raw[192:202]
    if ps[6]:
        print(f'prep first loads (cycles after start): joint record {int(ps[6] - ps[0])}, this frame\'s pose variables {int(ps[7] - ps[0])}, frame 0\'s {int(ps[8] - ps[0])}, component window {int(ps[9] - ps[0])}')
    print('prep (workgroup 0, wave 0): ' + ' | '.join(f'{n} +{int(ps[k + 1] - ps[k])}' for k, n in enumerate(['hand PCA -> fullpose', 'Rodrigues + features', 'chain', 'transform rows out', 'feature pieces out'])))
    names = ['start', 'tables + first loads issued', 'k-loop done'] + [f'block {h} done' for h in range(8)] + ['rows out']
    for ti in range(7):
        row = st[ti]
        if ti < 6 and st[ti + 1][11]:
            print(f'  (shader clock between the starts of tiles {ti} and {ti + 1}: {(st[ti + 1][0] - row[0]) / max(1, st[ti + 1][12] - row[12]) * 0.1:.2f} GHz)')
        if row[11] == 0:
            break
        print(f'tile {ti}: ' + ' | '.join(f'{names[k]} +{int(row[k] - row[k - 1]) if k else 0}' for k in range(12)) + f' | [block 3: wait + round-0 matrix instructions + next loads issued +{int(row[16] - row[5])}, previous rows read +{int(row[17] - row[16])}, stored +{int(row[13] - row[17])}, further rounds +{int(row[14] - row[13])}, apply + exchange +{int(row[15] - row[14])}, barrier +{int(row[6] - row[15])}]' + f' | total {int(row[11] - row[0])}' + (f' | gap to next {int(st[ti + 1][0] - row[11])}' if ti < 6 and st[ti + 1][11] else ''))
if int(os.environ.get('MOSHII_LBS_STOP', '0')) & 32:
    lib = capi.load()
    lib.moshii_internal_l32.restype = C.c_void_p
    lib.moshii_internal_l32.argtypes = [C.c_void_p]
    buf = (C.c_longlong * 1024)()
    lib.moshii_internal_lbs_debug_times.argtypes = [C.c_void_p, C.c_void_p]
    rc = lib.moshii_internal_lbs_debug_times(lib.moshii_internal_l32(solver.dev.handle), buf)
    tt = np.array(buf[:], dtype=np.int64).reshape(512, 2)
    t0 = tt[:, 0].min()
    st_, en_ = (tt[:, 0] - t0) * 0.01, (tt[:, 1] - t0) * 0.01    # us
    print(f'workgroups (last call): start {st_.min():.1f} .. {st_.max():.1f} us, end {en_.min():.1f} .. {en_.max():.1f} us, duration median {np.median(en_ - st_):.1f} us (min {np.min(en_ - st_):.1f}, max {np.max(en_ - st_):.1f})')
    for x in range(8):
        sel = np.arange(512) % 8 == x
        d = (en_ - st_)[sel]
        print(f'  XCD {x}: duration median {np.median(d):.1f} us, max {d.max():.1f}; first 32 slots {np.median(d[:32]):.1f}, last 32 slots {np.median(d[32:]):.1f}; latest end {en_[sel].max():.1f}')
