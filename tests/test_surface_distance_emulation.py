"""CPU: signed point-to-mesh distance (moshii_surface_distance_*, moshii_marker_surface_distance_*) in the emulation build --
lbs_forward.hip and moshii_api.hip compiled unchanged for the host.  Reference: oracle.stagei_oracle.signed_surface_distance in NumPy
f64 on the device's own inputs; points, checker and bounds: tests/surface_distance_common.py."""
import numpy as np
import pytest

from tests import normals_common as nc
from tests import surface_distance_common as sd
from tests.emu.emu_moshii import emulated_libmoshii


def _plain_calls(dev, case, F, N, require_all):
    """Both f32 kernels and the f64 kernel on F exported frames and N points a frame, each held to the checker; the two f32 kernels
    bit for bit; returns the f32 result."""
    from moshpp_amd import capi
    faces = case['faces']
    pose, trans = nc.inputs(case, F)
    v32 = dev.lbs_forward(pose, trans, dtype=np.float32)
    v64 = dev.lbs_forward(pose, trans)
    pts, seed = sd.build_points(v64, faces, N, require_all=require_all)
    print(f'{case["model_type"]} F={F} N={N}: points of seed {seed}')
    p32 = pts.astype(np.float32)
    with nc.env(MOSHII_SD_KERNEL='lds'):
        lds = dev.surface_distance(v32, p32)
        assert capi.last_launch_info()[0] == 'k_sd_lds' and lds.distance.dtype == np.float32
    gat = dev.surface_distance(v32, p32)                 # the default: the gather kernel
    assert capi.last_launch_info()[0] == 'k_sd_gather<float>'
    f64 = dev.surface_distance(v64, pts)
    assert capi.last_launch_info()[0] == 'k_sd_gather<double>' and f64.distance.dtype == np.float64
    sd.check(lds, v32, p32, faces, 'staged')
    sd.check(f64, v64, pts, faces, 'gather')
    for a, b in ((lds.distance, gat.distance), (lds.face, gat.face), (lds.part, gat.part), (lds.nearest, gat.nearest)):
        np.testing.assert_array_equal(a, b)
    return lds


@pytest.mark.parametrize('model_type,n_verts,F', [('mano', 778, 1), ('mano', 778, 5), ('smpl', 1500, 3)])
def test_surface_distance_of_exported_meshes_in_emulation(model_type, n_verts, F):
    from moshpp_amd import capi
    case = nc.mesh_case(model_type, n_verts)
    with emulated_libmoshii():
        dev = nc.device_model(case)
        _plain_calls(dev, case, F, 37, True)             # 37: not a multiple of a wavefront, nor of the four points a wave takes
        one = _plain_calls(dev, case, F, 1, False)       # one point a frame: the one-point-a-wave instantiation
        assert one.distance.shape == (F, 1)
        v = dev.lbs_forward(*nc.inputs(case, F), dtype=np.float32)
        none = dev.surface_distance(v, np.zeros((F, 0, 3), np.float32))
        assert none.distance.shape == (F, 0) and none.nearest.shape == (F, 0, 3)
        assert capi.last_launch_info()[0] == 'k_sd_gather<double>'        # nothing was launched: the call before it still stands
        dev.close()


def _fused(dev, case, pose, trans, faces, shape=None):
    """marker_surface_distance in both precisions with two frames a batch against (a) the plain call on the export's own vertices, bit
    for bit, and (b) the checker."""
    out = {}
    for dtype in (np.float32, np.float64):
        # (the export of a batch: the f32 kernels treat the joints that stay still within a CALL apart, so the last bits follow the batch)
        v = np.concatenate([dev.lbs_forward(pose[b:b + 2], trans[b:b + 2], dtype=dtype, shape=None if shape is None else shape[b:b + 2])
                            for b in range(0, len(pose), 2)])
        pts, _ = sd.build_points(v.astype(np.float64), faces, 37)
        pts = pts.astype(dtype)
        with nc.env(MOSHII_VM_BATCH='2'):
            res = dev.marker_surface_distance(pose, trans, pts, shape=shape, dtype=dtype)
        plain = dev.surface_distance(v, pts)
        for k in ('distance', 'face', 'part', 'nearest'):
            np.testing.assert_array_equal(getattr(res, k), getattr(plain, k))
        sd.check(res, v, pts, faces, 'fused')
        out[dtype] = res
    return out


def test_fused_entry_across_batches_in_emulation():
    case = nc.mesh_case('mano', 778)
    pose, trans = nc.inputs(case, 5)                     # batches of 2, 2 and 1 frames
    with emulated_libmoshii():
        dev = nc.device_model(case)
        _fused(dev, case, pose, trans, case['faces'])
        dev.close()


def test_fused_entry_with_a_free_shape_block_in_emulation():
    from tests.lbs_shape_common import block_case, block_device, export_inputs
    case = block_case('mano', 5, order='mesh')
    faces = nc.mesh_case('mano', 600)['faces']
    assert faces.max() < case['model']['v_template'].shape[0]
    pose, trans, shape = export_inputs(case, 5)
    # (those triangles were made for another body: on this one some are needles.  The faces whose k L / 2 stays below 2 m on every
    #  frame, with and without the coefficients, are the mesh of this test -- the condition C3 of the bound, decided by the oracle.)
    keep = np.ones(len(faces), dtype=bool)
    for v in (nc.oracle_verts(case['m'], pose, trans, shape), nc.oracle_verts(case['m'], pose, trans)):
        a, b, c = (v[:, faces[:, k]] for k in range(3))
        L = np.sqrt(np.maximum(((a - b) ** 2).sum(2), np.maximum(((b - c) ** 2).sum(2), ((c - a) ** 2).sum(2))))
        keep &= (L ** 3 / np.linalg.norm(np.cross(b - a, c - a), axis=2) <= 2.0).all(axis=0)
    print(f'{keep.sum()} of {len(faces)} faces kept')
    assert keep.sum() > len(faces) // 2
    faces = np.ascontiguousarray(faces[keep])
    with emulated_libmoshii():
        dev = block_device(case)['model']
        dev.set_faces(faces)
        with_shape = _fused(dev, case, pose, trans, faces, shape=shape)
        pts, _ = sd.build_points(dev.lbs_forward(pose, trans, shape=shape), faces, 37)
        plain = dev.marker_surface_distance(pose, trans, pts)
        moved = dev.marker_surface_distance(pose, trans, pts, shape=shape)
        dev.close()
    fin = np.isfinite(pts).all(axis=2)
    assert np.abs(plain.distance[fin] - moved.distance[fin]).max() > 1e-3      # the skin follows the coefficients
    assert with_shape[np.float64].distance.shape == (5, 37)


def test_degenerate_face_and_vertex_without_faces_in_emulation():
    """A face that names a vertex twice never wins (it sits first in the list, where every tie would go to it), and a vertex that
    lost all its faces is no part of the surface."""
    case = nc.mesh_case('smpl', 1500)
    faces = case['faces']
    V = case['model']['v_template'].shape[0]
    lone = V // 3
    cut = faces[~(faces == lone).any(axis=1)]
    cut = np.vstack([[[cut[0, 0], cut[0, 0], cut[0, 1]]], cut]).astype(np.int32)
    pose, trans = nc.inputs(case, 2)
    with emulated_libmoshii():
        dev = nc.device_model(case, faces=cut)
        v32 = dev.lbs_forward(pose, trans, dtype=np.float32)
        pts, _ = sd.build_points(v32.astype(np.float64), cut, 37)
        pts[:, 0] = v32[:, lone]                          # the lone vertex itself: some way off the remaining surface
        pts[:, 1] = v32[:, cut[0, 0]]                     # a vertex of the degenerate face
        pts = pts.astype(np.float32)
        with nc.env(MOSHII_SD_KERNEL='lds'):
            res = dev.surface_distance(v32, pts)
        gat = dev.surface_distance(v32, pts)
        r64 = dev.surface_distance(v32.astype(np.float64), pts.astype(np.float64))
        dev.close()
    sd.check(res, v32, pts, cut, 'cut')
    sd.check(r64, v32, pts, cut, 'cut')
    np.testing.assert_array_equal(res.distance, gat.distance)
    assert (res.face != 0).all() and (r64.face != 0).all()
    assert (np.abs(res.distance[:, 0]) > 1e-4).all() and (np.abs(res.distance[:, 1]) <= sd.bound_for(np.float32, v32, pts)).all()


def test_library_refusals_in_emulation():
    """The C ABI's own checks: no faces, null dist, negative sizes -> MOSHII_ERR_ARG with a message; F == 0 / N == 0 -> MOSHII_OK."""
    from moshpp_amd import capi
    case = nc.mesh_case('mano', 778)
    pose, trans = nc.inputs(case, 2)
    with emulated_libmoshii():
        lib = capi.load()
        dev = nc.device_model(case, faces=None)
        v = dev.lbs_forward(pose, trans, dtype=np.float32)
        p = v[:, :3].copy()
        d = np.zeros((2, 3), np.float32)
        args = (dev.handle, 2, v.ctypes.data, 3, p.ctypes.data, d.ctypes.data, None, None, None, capi.BUFFERS_HOST, None)
        assert lib.moshii_surface_distance_f32(*args) == -1 and b'moshii_model_set_faces' in lib.moshii_last_error()
        p32, t32 = pose.astype(np.float32), trans.astype(np.float32)
        assert lib.moshii_marker_surface_distance_f32(dev.handle, 2, p32.ctypes.data, t32.ctypes.data, None, 3, p.ctypes.data, d.ctypes.data,
                                                      None, None, None, capi.BUFFERS_HOST, None) == -1
        with pytest.raises(ValueError, match='no faces'):
            dev.surface_distance(v, p)
        dev.set_faces(case['faces'])
        assert lib.moshii_surface_distance_f32(*args) == 0                       # face / part / nearest may be null
        np.testing.assert_array_equal(d, dev.surface_distance(v, p).distance)
        bad = list(args); bad[5] = None
        assert lib.moshii_surface_distance_f32(*bad) == -1 and b'dist' in lib.moshii_last_error()
        for at in (1, 3):
            bad = list(args); bad[at] = -1
            assert lib.moshii_surface_distance_f32(*bad) == -1 and b'negative' in lib.moshii_last_error()
            zero = list(args); zero[at] = 0
            assert lib.moshii_surface_distance_f32(*zero) == 0
        dev.close()


def _stageii_data(case, T=6):
    """test_normals_emulation's synthetic Stage-II result with observed markers: the virtual markers of five labels on the oracle's
    meshes, each moved by up to 3 mm, label 'C' unobserved on frames 1 and 4."""
    from tests.test_normals_emulation import _stageii_result
    sm, data, orc = _stageii_result(case, T)
    labels = ['A', 'B', 'C', 'D', 'E']
    vids = np.array([30, 400, 651, 77, 500])
    rng = np.random.default_rng(4)
    mk = orc[:, vids] + 0.0095 * nc.ref_normals(orc, case['faces'])[:, vids] + rng.uniform(-0.003, 0.003, (T, 5, 3))
    keep = np.ones((T, 5), dtype=bool)
    keep[[1, 4], 2] = False
    dbg = data['stageii_debug_details']
    dbg['markers_obs'] = [mk[f][keep[f]] for f in range(T)]
    dbg['labels_obs'] = [[l for l, k in zip(labels, keep[f]) if k] for f in range(T)]
    data['latent_labels'] = labels
    return sm, data, orc, mk, keep, labels


def test_mosh_head_marker_skin_distance_in_emulation():
    from moshpp_amd import mosh_head
    case = nc.mesh_case('mano', 778)
    sm, data, orc, mk, keep, labels = _stageii_data(case)
    with emulated_libmoshii():
        res = mosh_head.stageii_marker_skin_distance(data, surface_model=sm, dtype=np.float64)
        sub = mosh_head.stageii_marker_skin_distance(data, surface_model=sm, frame_ids=[4, 0, 4])
    assert res['labels'] == labels and res['distance'].shape == (6, 5) and list(res['frame_ids']) == list(range(6))
    np.testing.assert_array_equal(np.isfinite(res['distance']), keep)
    assert (res['face'][~keep] == -1).all() and (res['part'][~keep] == -1).all()
    from oracle import stagei_oracle as s1
    for f in range(6):
        d = s1.signed_surface_distance(mk[f][keep[f]], orc[f], case['faces'])[0]
        assert np.abs(res['distance'][f][keep[f]] - d).max() < 1e-9           # (the f64 export against the oracle's vertices: 1e-12)
    assert (np.abs(res['distance'][keep]) <= 0.0095 + 0.003 * np.sqrt(3) + 1e-9).all()      # 9.5 mm off a vertex, moved by <= 3 sqrt(3) mm
    assert res['summary']['C']['count'] == 4 and res['summary']['A']['count'] == 6
    assert res['summary']['A']['negative_share'] == (res['distance'][:, 0] < 0).mean()
    assert abs(res['summary']['B']['median'] - np.median(res['distance'][:, 1])) < 1e-15
    assert sub['distance'].dtype == np.float32 and list(sub['frame_ids']) == [4, 0, 4]
    np.testing.assert_array_equal(sub['distance'][0], sub['distance'][2])
    assert np.isnan(sub['distance'][0, 2]) and np.isfinite(sub['distance'][1]).all()
    assert np.nanmax(np.abs(sub['distance'] - res['distance'][[4, 0, 4]])) < 2 * nc.F32_TOL


def test_virtual_markers_sit_their_distance_from_the_skin_in_emulation():
    """Round trip: a marker grown 9.5 mm from a vertex is at most that far from the skin -- the vertex is that close."""
    from moshpp_amd import mosh_head
    case = nc.mesh_case('mano', 778)
    sm, data, orc, _, _, _ = _stageii_data(case)
    layout = {f'M{i}': int(v) for i, v in enumerate(np.random.default_rng(2).choice(orc.shape[1], 24, replace=False))}
    with emulated_libmoshii():
        vm = mosh_head.stageii_virtual_markers(data, layout, surface_model=sm, dtype=np.float32)
        dbg = data['stageii_debug_details']
        dbg['markers_obs'] = list(vm['markers'])
        dbg['labels_obs'] = [vm['labels']] * len(vm['markers'])
        data['latent_labels'] = vm['labels']
        res = mosh_head.stageii_marker_skin_distance(data, surface_model=sm, dtype=np.float32)
        verts = mosh_head.stageii_vertices(data, surface_model=sm)
    bound = sd.bound_for(np.float32, verts, vm['markers'])[:, None]
    print(f'virtual markers at 9.5 mm: |d| in [{np.abs(res["distance"]).min():.6f}, {np.abs(res["distance"]).max():.6f}]')
    assert (np.abs(res['distance']) <= 0.0095 + bound).all()
    assert (res['distance'] > 0).mean() > 0.5                 # outside, but for markers that land in a neighbouring finger
