"""GPU: signed point-to-mesh distance on the device -- the cases of tests/test_surface_distance_emulation.py plus the full-size bodies
(SMPL-H: a frame beyond 64 KB of LDS; an SMPL-X-sized body: the largest frame the staged kernel takes; a wider one that must fall back
to the gather kernel), the fused entry across batches, streams and device buffers, and a solved sequence.  Points, checker and
bounds: tests/surface_distance_common.py."""
import ctypes as C

import numpy as np
import pytest

from tests import normals_common as nc
from tests import surface_distance_common as sd

pytestmark = pytest.mark.gpu

FIELDS = ('distance', 'face', 'part', 'nearest')


def _same(a, b):
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))


def _staged_and_gather(dev, case, F, N, f64_frames=3):
    """The staged and the gather f32 kernel bit for bit, a repeat call bit for bit, both held to the checker; the f64 kernel on the
    first frames."""
    from moshpp_amd import capi
    faces = case['faces']
    pose, trans = nc.inputs(case, F)
    v32 = dev.lbs_forward(pose, trans, dtype=np.float32)
    pts, seed = sd.build_points(v32.astype(np.float64), faces, N)
    p32 = pts.astype(np.float32)
    with nc.env(MOSHII_SD_KERNEL='lds'):
        lds = dev.surface_distance(v32, p32)
        assert capi.last_launch_info()[0] == 'k_sd_lds'
        _same(lds, dev.surface_distance(v32, p32))               # no order of arrival decides anything
    gat = dev.surface_distance(v32, p32)                         # the default: the gather kernel
    assert capi.last_launch_info()[0] == 'k_sd_gather<float>'
    _same(gat, dev.surface_distance(v32, p32))
    _same(lds, gat)
    sd.check(lds, v32, p32, faces, f'{case["model_type"]} F={F} N={N} (seed {seed}) staged')
    if f64_frames:
        v64 = dev.lbs_forward(pose[:f64_frames], trans[:f64_frames])
        p64, _ = sd.build_points(v64, faces, N)
        r64 = dev.surface_distance(v64, p64)
        assert capi.last_launch_info()[0] == 'k_sd_gather<double>'
        _same(r64, dev.surface_distance(v64, p64))
        sd.check(r64, v64, p64, faces, f'{case["model_type"]} f64')
    return lds


@pytest.mark.parametrize('model_type,n_verts,F', [('mano', 778, 1), ('mano', 778, 37), ('smpl', 1500, 19)])
def test_small_bodies_all_three_kernels(model_type, n_verts, F):
    case = nc.mesh_case(model_type, n_verts)
    dev = nc.device_model(case)
    _staged_and_gather(dev, case, F, 37)
    one = dev.surface_distance(dev.lbs_forward(*nc.inputs(case, F), dtype=np.float32), np.zeros((F, 1, 3), np.float32))
    assert np.isfinite(one.distance).all()                       # one point a frame: the one-point-a-wave instantiation
    dev.close()


def test_smplh_default_size_through_the_staged_kernel():
    from moshpp_amd import capi
    case = nc.mesh_case('smplh', None)
    V = case['model']['v_template'].shape[0]
    assert V * 12 > 64 * 1024                                    # beyond the default LDS limit
    dev = nc.device_model(case)
    _staged_and_gather(dev, case, 9, 53, f64_frames=2)
    v = dev.lbs_forward(*nc.inputs(case, 2), dtype=np.float32)
    with nc.env(MOSHII_SD_KERNEL='lds'):
        dev.surface_distance(v, v[:, :53].copy())
    name, lds, threads = capi.last_launch_info()
    assert name == 'k_sd_lds' and lds >= V * 12 and threads == 1024
    dev.close()


def test_smplx_sized_body_through_the_staged_kernel():
    case = nc.mesh_case('smplx', None)
    V = case['model']['v_template'].shape[0]
    assert 100 * 1024 < V * 12 < 160 * 1024 - 256                # the largest frame the staged kernel takes
    dev = nc.device_model(case)
    _staged_and_gather(dev, case, 5, 89, f64_frames=0)
    dev.close()


def test_a_body_beyond_the_lds_budget_falls_back_to_the_gather_kernel():
    """normals_common.wide_body: 65 600 vertices (32-bit face ids, a 787 KB frame) under 4000 random triangles."""
    from moshpp_amd import capi
    model, faces, verts = nc.wide_body()
    dev = nc.device_model(dict(model=model), faces=faces)
    v32 = np.ascontiguousarray(verts, dtype=np.float32)
    rng = np.random.default_rng(3)
    tri = rng.integers(0, len(faces), (2, 21))
    # points 1 mm above random triangles' centroids: among random triangles the oracle decides what is nearest
    pts = np.stack([v32[f][faces[tri[f]]].astype(np.float64).mean(axis=1) + 0.001 for f in range(2)]).astype(np.float32)
    pts[1, 4] = np.nan
    res = dev.surface_distance(v32, pts)
    assert capi.last_launch_info()[0] == 'k_sd_gather<float>'
    _same(res, dev.surface_distance(v32, pts))
    from oracle import stagei_oracle as s1
    good = sd._good_faces(faces)
    for f in range(2):
        fin = np.isfinite(pts[f]).all(axis=1)
        d = s1.signed_surface_distance(pts[f][fin].astype(np.float64), v32[f].astype(np.float64), faces[good])[0]
        assert np.abs(np.abs(res.distance[f][fin]) - np.abs(d)).max() <= sd.bound_for(np.float32, v32[f:f + 1], pts[f:f + 1])[0]
    assert np.isnan(res.distance[1, 4]) and res.face[1, 4] == -1
    dev.close()


def test_fused_entry_on_smplh_batches_streams_and_device_buffers():
    from moshpp_amd import capi
    case = nc.mesh_case('smplh', None)
    F, N = 140, 53
    faces = case['faces']
    pose, trans = nc.inputs(case, F)
    # frames of every batch (64 + 64 + 12) are held to the oracle
    rows = np.array([0, 1, 63, 64, 65, 127, 128, 139])
    dev = nc.device_model(case)
    with nc.env(MOSHII_VM_BATCH='64'):                           # three batches, the last one of 12 frames
        host = {}
        for dt in (np.float32, np.float64):
            # the export of each batch, as the fused call makes it
            v = np.concatenate([dev.lbs_forward(pose[b:b + 64], trans[b:b + 64], dtype=dt) for b in range(0, F, 64)])
            pts = np.full((F, N, 3), np.nan)
            pts[rows], _ = sd.build_points(v[rows].astype(np.float64), faces, N)
            rest = np.setdiff1d(np.arange(F), rows)
            pts[rest] = v[rest][:, 7::130][:, :N] + 0.004       # the other frames: points near the skin, compared with the plain call
            pts = pts.astype(dt)
            res = dev.marker_surface_distance(pose, trans, pts, dtype=dt)
            _same(res, dev.surface_distance(v, pts))
            with nc.env(MOSHII_SD_KERNEL='lds'):                 # the staged search inside the fused call: the same bits
                _same(res, dev.marker_surface_distance(pose, trans, pts, dtype=dt))
            sub = capi.SurfaceDistance(*(getattr(res, k)[rows] for k in FIELDS))
            sd.check(sub, v[rows], pts[rows], faces, f'fused smplh {np.dtype(dt).name}')
            host[dt] = (pts, res)
        # device buffers on a stream of their own: the same bits as the host-buffer call
        hip = C.CDLL('libamdhip64.so')      # (the runtime libmoshii already brought into the process)
        stream = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
        try:
            for dt in (np.float32, np.float64):
                pts, res = host[dt]
                p, t = (np.ascontiguousarray(a, dtype=dt) for a in (pose, trans))
                isz = p.itemsize
                bufs = [capi.DeviceBuffer(n) for n in (p.nbytes, t.nbytes, pts.nbytes, F * N * isz, F * N * 4, F * N * 4, F * N * 3 * isz)]
                bufs[0].upload(p); bufs[1].upload(t); bufs[2].upload(pts)
                dev.marker_surface_distance_device(F, bufs[0].ptr, bufs[1].ptr, N, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr,
                                                   bufs[6].ptr, stream=stream, f32=dt == np.float32)
                assert hip.hipStreamSynchronize(stream) == 0
                np.testing.assert_array_equal(bufs[3].download(np.zeros((F, N), dtype=dt)), res.distance)
                np.testing.assert_array_equal(bufs[4].download(np.zeros((F, N), dtype=np.int32)), res.face)
                np.testing.assert_array_equal(bufs[5].download(np.zeros((F, N), dtype=np.int32)), res.part)
                np.testing.assert_array_equal(bufs[6].download(np.zeros((F, N, 3), dtype=dt)), res.nearest)
                # distances alone: the winners go to the handle's scratch
                dev.marker_surface_distance_device(F, bufs[0].ptr, bufs[1].ptr, N, bufs[2].ptr, bufs[3].ptr, stream=stream, f32=dt == np.float32)
                assert hip.hipStreamSynchronize(stream) == 0
                np.testing.assert_array_equal(bufs[3].download(np.zeros((F, N), dtype=dt)), res.distance)
                for bf in bufs:
                    bf.close()
        finally:
            hip.hipStreamDestroy(stream)
    dev.close()


def test_marker_skin_distance_of_a_solved_sequence():
    """StageIISolver.marker_skin_distance after a short real solve: on every observed marker |d| is at most the distance to the vertex
    of the label's vertex id on that frame (that vertex is part of the skin), and the distances are the oracle's on the exported mesh."""
    from moshpp_amd import synth, workload
    from oracle import stagei_oracle as s1
    dd = synth.synth_mesh_model('smpl', seed=1000, n_verts=1500)
    F, M = 24, 41
    job = workload.make_job('smpl', F, M, seed=1000, dd=dd)
    solver = workload.make_solver(job)
    obs, vis = np.asarray(job['obs'], dtype=np.float64), np.asarray(job['vis'], dtype=bool)
    out = solver.solve(obs, vis, chain_mode='sequential')
    assert (out['status'] != 1).all()
    res = solver.marker_skin_distance(out, obs=obs, vis=vis)
    assert res.distance.shape == (F, M) and res.distance.dtype == np.float32
    np.testing.assert_array_equal(np.isfinite(res.distance), vis)
    verts = solver.vertices(out)
    faces = np.asarray(dd['f'], dtype=np.int32)
    pts = np.where(vis[:, :, None], obs, np.nan).astype(np.float32)
    bound = sd.bound_for(np.float32, verts, pts)
    # one-sided data-term consistency: the vertex a label is attached to is part of the skin, so the skin is at least that close
    vids = np.array(list(job['seq']['marker_meta']['marker_vids'].values()))
    dv = np.linalg.norm(pts.astype(np.float64) - verts[:, vids].astype(np.float64), axis=2)
    print(f'|d| {np.nanmedian(np.abs(res.distance)) * 1e3:.2f} mm (median), distance to the labels\' vertices {np.nanmedian(dv) * 1e3:.2f} mm')
    assert (np.abs(res.distance[vis]) <= dv[vis] + np.broadcast_to(bound[:, None], vis.shape)[vis]).all()
    good = sd._good_faces(faces)
    for f in (0, 11, 23):
        d = s1.signed_surface_distance(pts[f][vis[f]].astype(np.float64), verts[f].astype(np.float64), faces[good])[0]
        err = np.abs(res.distance[f][vis[f]] - d).max()
        print(f'solved frame {f}: distance vs the oracle on the exported mesh {err:.3e} (bound {bound[f]:.3e}), median {np.median(d) * 1e3:.2f} mm')
        assert err <= bound[f]
