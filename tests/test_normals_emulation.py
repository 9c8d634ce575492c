"""CPU: vertex normals and virtual markers (moshii_model_set_faces, moshii_vertex_normals_*, moshii_virtual_markers_*) in the emulation
build -- lbs_forward.hip and moshii_api.hip compiled unchanged for the host.  Reference: oracle.stagei_oracle.vert_normals /
markers_latent_init in NumPy f64; bounds and bodies: tests/normals_common.py."""
import numpy as np
import pytest

from oracle import stageii_oracle as so
from oracle import stagei_oracle as s1
from tests import normals_common as nc
from tests.emu.emu_moshii import emulated_libmoshii


@pytest.mark.parametrize('model_type,n_verts,V,F', [('mano', 778, 817, 1), ('mano', 778, 817, 37), ('smpl', 1500, 1638, 19)])
def test_normals_of_exported_meshes_in_emulation(model_type, n_verts, V, F):
    """The LDS kernel, the gather kernel (MOSHII_VN_KERNEL) and the f64 kernel: SAME_* on every vertex, f64 end to end, repeat bits."""
    case = nc.mesh_case(model_type, n_verts)
    assert case['model']['v_template'].shape[0] == V
    with emulated_libmoshii():
        dev = nc.device_model(case)
        out = nc.check_body(dev, case, F)
        dev.close()
    np.testing.assert_array_equal(out['n32'], out['g32'])      # the two f32 kernels sum the same rows in the same order
    val = nc.valence(case['faces'], V)
    print(f'valence {val.min()} .. {val.max()}')
    assert val.max() >= 3 * val.min()                           # rows of very different lengths share waves


def _cut_faces(faces, V):
    """The face list with 40 faces removed -- every face of three vertices among them, which lose all their faces -- and two
    degenerate faces appended."""
    lone = np.array([10, V // 3, V - 7])
    touch = np.isin(faces, lone).any(axis=1)
    assert touch.sum() < 40
    drop = touch.copy()
    drop[np.flatnonzero(~touch)[:40 - touch.sum()]] = True
    assert drop.sum() == 40
    cut = np.vstack([faces[~drop], [[5, 5, 9], [20, 33, 20]]]).astype(np.int32)
    return cut, lone, np.unique(faces[drop])


def test_vertices_without_faces_and_degenerate_faces_in_emulation():
    case = nc.mesh_case('smpl', 1500)
    V = case['model']['v_template'].shape[0]
    cut, lone, touched = _cut_faces(case['faces'], V)
    with emulated_libmoshii():
        dev = nc.device_model(case, faces=cut)
        out = nc.check_body(dev, case, 3, faces=cut)
        dev.close()
    for key in ('n32', 'g32', 'n64'):
        assert (out[key][:, lone] == 0).all()
    # vertices none of whose faces were touched keep the normals of the full list
    full = nc.ref_normals(out['v32'], case['faces'])
    kept = np.setdiff1d(np.arange(V), np.concatenate([touched, [5, 9, 20, 33]]))
    assert len(kept) > V // 2
    assert np.abs(out['n32'][:, kept] - full[:, kept]).max() <= nc.SAME_F32


def test_set_faces_replaced_and_cleared_on_a_live_handle_in_emulation():
    from moshpp_amd import capi
    case = nc.mesh_case('mano', 778)
    V = case['model']['v_template'].shape[0]
    pose, trans = nc.inputs(case, 2)
    flipped = np.ascontiguousarray(case['faces'][:, ::-1])
    with emulated_libmoshii():
        dev = nc.device_model(case, faces=None)
        v = dev.lbs_forward(pose, trans, dtype=np.float32)
        out = np.zeros_like(v)
        lib = capi.load()
        rc = lib.moshii_vertex_normals_f32(dev.handle, 2, v.ctypes.data, out.ctypes.data, capi.BUFFERS_HOST, None)
        assert rc == -1 and b'moshii_model_set_faces' in lib.moshii_last_error()
        dev.set_faces(case['faces'])
        n0 = dev.vertex_normals(v)
        dev.set_faces(flipped)                                   # the next call follows the new table
        n1 = dev.vertex_normals(v)
        np.testing.assert_array_equal(n1, -n0)
        nc.check_same_input(n1, v, flipped)
        bad = case['faces'].copy(); bad[3, 1] = V
        assert lib.moshii_model_set_faces(dev.handle, len(bad), bad.ctypes.data) == -1      # an id outside [0, V): MOSHII_ERR_ARG
        np.testing.assert_array_equal(dev.vertex_normals(v), n1)                            # ... and the table in place stays
        dev.set_faces([])
        for fn, a in ((lib.moshii_vertex_normals_f32, v), (lib.moshii_vertex_normals_f64, v.astype(np.float64))):
            o = np.zeros_like(a)
            assert fn(dev.handle, 2, a.ctypes.data, o.ctypes.data, capi.BUFFERS_HOST, None) == -1
        mk = np.zeros((2, 1, 3), np.float32)
        p32, t32 = pose.astype(np.float32), trans.astype(np.float32)
        vid, dist = np.array([4], np.int32), np.array([0.01], np.float32)
        assert lib.moshii_virtual_markers_f32(dev.handle, 2, p32.ctypes.data, t32.ctypes.data, None, 1, vid.ctypes.data, dist.ctypes.data,
                                              mk.ctypes.data, None, capi.BUFFERS_HOST, None) == -1
        with pytest.raises(ValueError, match='no faces'):
            dev.vertex_normals(v)
        dev.close()


@pytest.fixture(scope='module')
def mano_markers():
    """M = 24 with a repeated vertex, a zero and a negative distance, on 37 frames of the MANO mesh body."""
    case = nc.mesh_case('mano', 778)
    pose, trans = nc.inputs(case, 37)
    b = nc.normal_bound(nc.oracle_verts(case['m'], pose, trans), case['faces'], nc.F32_TOL)
    vids = nc.pick_marker_vids(b, case['faces'], 24)
    vids[1] = vids[0]
    dist = np.full(24, 0.0095); dist[2] = 0.0; dist[3] = -0.012; dist[4] = 0.03
    return case, pose, trans, vids, dist


def test_virtual_markers_across_batches_in_emulation(mano_markers):
    case, pose, trans, vids, dist = mano_markers
    with emulated_libmoshii():
        dev = nc.device_model(case)
        with nc.env(MOSHII_VM_BATCH='16'):                       # three batches, the last one partial
            cut = nc.check_markers(dev, case, pose, trans, vids, dist)
        whole = {dt: dev.virtual_markers(pose, trans, vids, dist, dtype=dt) for dt in (np.float32, np.float64)}
        dev.close()
    for dt in whole:
        np.testing.assert_array_equal(cut[dt][0], whole[dt])
    np.testing.assert_array_equal(whole[np.float64][:, 0], whole[np.float64][:, 1])      # the repeated vertex
    assert np.abs(whole[np.float64][:, 3] - whole[np.float64][:, 4]).max() > 0.03        # either side of the skin


def test_zero_pose_markers_are_the_reference_placement_in_emulation(mano_markers):
    """prepare_mosh_markers_latent (chmosh.py:57-67): vertex + vertex normal x distance-from-skin on the canonical body."""
    case, _, _, vids, dist = mano_markers
    m = case['m']
    can_v = so.verts_forward(m, so.fullpose_from_pose(m, np.zeros(m['NP'])), np.zeros(3))
    ref = s1.markers_latent_init(can_v, case['faces'], vids, dist)
    with emulated_libmoshii():
        dev = nc.device_model(case)
        got = dev.virtual_markers(np.zeros((1, m['NP'])), np.zeros((1, 3)), vids, dist)[0]
        dev.close()
    b = nc.normal_bound(can_v[None], case['faces'], nc.F64_TOL)[0, vids]
    err = np.abs(got - ref).max(axis=1)
    print(f'zero pose: {err.max():.3e} (largest allowance {(b + 1e-12).max():.3e})')
    assert (err <= b + 1e-12).all()


def test_virtual_markers_with_a_free_shape_block_in_emulation():
    """lbs_shape_common.block_case's geometry with the triangles of a smaller mesh body: the markers follow the coefficients."""
    from tests.lbs_shape_common import block_case, block_device, export_inputs
    case = block_case('mano', 5, order='mesh')
    faces = nc.mesh_case('mano', 600)['faces']
    V = case['model']['v_template'].shape[0]
    assert faces.max() < V
    pose, trans, shape = export_inputs(case, 5)
    b = nc.normal_bound(nc.oracle_verts(case['m'], pose, trans, shape), faces, nc.F32_TOL)
    ok = np.flatnonzero((b < 0.1).all(0))
    vids = np.random.default_rng(1).choice(ok, 12, replace=False).astype(np.int32)
    dist = np.full(12, 0.0095)
    with emulated_libmoshii():
        dev = block_device(case)['model']
        dev.set_faces(faces)
        with_shape = nc.check_markers(dev, case, pose, trans, vids, dist, faces=faces, shape=shape)
        plain = dev.virtual_markers(pose, trans, vids, dist)
        dev.close()
    assert np.abs(with_shape[np.float64][0] - plain).max() > 1e-3


def test_exports_keep_their_bits_around_normals_calls_in_emulation():
    """One handle: what it exports before it has faces (plain and shape export, both precisions) it exports again, bit for bit, after
    set_faces and normals / marker calls on it -- they share the handle's per-call scratch."""
    from tests.lbs_shape_common import block_case, block_device, export_inputs
    case = block_case('mano', 5, order='mesh')
    faces = nc.mesh_case('mano', 600)['faces']
    pose, trans, shape = export_inputs(case, 17)
    with emulated_libmoshii():
        dev = block_device(case)['model']
        before = [dev.lbs_forward(pose, trans, dtype=np.float32), dev.lbs_forward(pose, trans, dtype=np.float32, shape=shape),
                  dev.lbs_forward(pose, trans), dev.lbs_forward(pose, trans, shape=shape)]
        dev.set_faces(faces)
        dev.vertex_normals(before[0])
        with nc.env(MOSHII_VM_BATCH='9'):
            dev.virtual_markers(pose, trans, [3, 4], [0.01, 0.01], dtype=np.float32, shape=shape)
            dev.virtual_markers(pose, trans, [3, 4], [0.01, 0.01], dtype=np.float64)
        after = [dev.lbs_forward(pose, trans, dtype=np.float32), dev.lbs_forward(pose, trans, dtype=np.float32, shape=shape),
                 dev.lbs_forward(pose, trans), dev.lbs_forward(pose, trans, shape=shape)]
        dev.close()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


def _stageii_result(case, T=5):
    from moshpp_amd.models import SurfaceModel
    md, m = case['model'], case['m']
    sm = SurfaceModel(case['model_type'], md['v_template'], md['shapedirs'], md['posedirs'], md['weights'], md['J_regressor'],
                      np.asarray(md['parents'], dtype=np.int32), md['body_dof'], md['hand_dof'], md['hands_mean'], md['selected_components'],
                      f=case['faces'])
    pose, trans = nc.inputs(case, T, seed=9)
    fullpose = np.stack([so.fullpose_from_pose(m, p) for p in pose])
    cfg = {'surface_model': {'type': case['model_type'], 'num_betas': 10, 'fname': None}, 'moshpp': {}}
    data = {'fullpose': fullpose, 'trans': trans, 'betas': np.zeros(10), 'stageii_debug_details': {'cfg': cfg, 'mocap_frame_rate': 100.0}}
    return sm, data, nc.oracle_verts(m, pose, trans)


def test_mosh_head_normals_and_virtual_markers_in_emulation(tmp_path):
    from moshpp_amd import mosh_head
    from moshpp_amd.mocap_interface import MocapSession
    case = nc.mesh_case('mano', 778)
    sm, data, orc = _stageii_result(case)
    layout = {'surface_model_type': 'mano',
              'markersets': [{'type': 'body', 'distance_from_skin': 0.0095, 'indices': {'A': 30, 'B': 400, 'C': 651}},
                             {'type': 'finger', 'distance_from_skin': 0.004, 'indices': {'D': 77, 'E': 500}}]}
    from moshpp_amd.marker_layout import marker_layout_load
    meta = marker_layout_load(layout, labels_map=None)
    with emulated_libmoshii():
        plain = mosh_head.stageii_vertices(data, surface_model=sm)
        verts, normals = mosh_head.stageii_vertices(data, surface_model=sm, return_normals=True)
        v64, n64 = mosh_head.stageii_vertices(data, surface_model=sm, return_normals=True, dtype=np.float64, frame_ids=[3, 1])
        res = mosh_head.stageii_virtual_markers(data, meta, surface_model=sm, dtype=np.float64, out_fname=str(tmp_path / 'vm.npz'))
        res32 = mosh_head.stageii_virtual_markers(data, {'A': 30, 'Z': 651}, surface_model=sm, frame_ids=[4, 0],
                                                  out_fname=str(tmp_path / 'sub' / 'vm.c3d'))
    np.testing.assert_array_equal(plain, verts)                   # return_normals changes nothing about the vertices
    assert normals.dtype == np.float32 and normals.shape == verts.shape
    nc.check_same_input(normals, verts, case['faces'])
    assert np.abs(v64 - orc[[3, 1]]).max() < 1e-9
    nc.check_same_input(n64, v64, case['faces'])
    labels = list(meta['marker_vids'])
    vids = np.array([meta['marker_vids'][l] for l in labels])
    m2b = np.array([0.004 if l in ('D', 'E') else 0.0095 for l in labels])
    assert res['labels'] == labels and list(res['vids']) == list(vids) and np.allclose(res['m2b'], m2b)
    ref = orc[:, vids] + m2b[None, :, None] * nc.ref_normals(orc, case['faces'])[:, vids]
    assert np.abs(res['markers'] - ref).max() < 1e-9
    back = MocapSession(str(tmp_path / 'vm.npz'), 'm')
    assert back.labels == labels and back.frame_rate == 100.0
    np.testing.assert_array_equal(back.markers, res['markers'])
    ref32 = orc[[4, 0]][:, [30, 651]] + 0.0095 * nc.ref_normals(orc[[4, 0]], case['faces'])[:, [30, 651]]
    assert res32['markers'].dtype == np.float32 and np.abs(res32['markers'] - ref32).max() < nc.F32_TOL * 2
    back = MocapSession(str(tmp_path / 'sub' / 'vm.c3d'), 'mm')
    assert back.labels == ['A', 'Z'] and abs(back.frame_rate - 100.0) < 1e-6
    mm = np.abs(res32['markers']).max() * 1000.0
    assert np.abs(back.markers - res32['markers']).max() <= 2.0 ** -23 * mm / 1000.0 * 2      # f32 millimetres in the file


def test_more_than_65535_vertices_in_emulation():
    """32-bit pairs in the face table, and an f32 frame beyond the LDS budget: the gather kernel without being asked."""
    with emulated_libmoshii():
        nc.check_wide_body()
