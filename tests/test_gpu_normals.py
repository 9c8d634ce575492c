"""GPU: vertex normals and virtual markers on the device -- the cases of tests/test_normals_emulation.py plus the full-size bodies
(SMPL-H: valence up to 34; an SMPL-X-sized body: the largest LDS footprint of the staged kernel), batches, streams and device
buffers.  Reference and bounds: tests/normals_common.py."""
import ctypes as C

import numpy as np
import pytest

from tests import normals_common as nc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('model_type,n_verts,F', [('mano', 778, 1), ('mano', 778, 37), ('smpl', 1500, 19)])
def test_small_bodies_all_three_kernels(model_type, n_verts, F):
    case = nc.mesh_case(model_type, n_verts)
    dev = nc.device_model(case)
    out = nc.check_body(dev, case, F)
    dev.close()
    np.testing.assert_array_equal(out['n32'], out['g32'])


def test_smplh_default_size_through_the_lds_kernel():
    case = nc.mesh_case('smplh', None)
    V = case['model']['v_template'].shape[0]
    val = nc.valence(case['faces'], V)
    print(f'{V} vertices, valence {val.min()} .. {val.max()}')
    assert V * 12 > 64 * 1024 and val.max() >= 30          # beyond the default LDS limit; pole vertices
    dev = nc.device_model(case)
    nc.check_body(dev, case, 33, e2e_frames=3)
    dev.close()


def test_smplx_sized_body_through_the_lds_kernel():
    case = nc.mesh_case('smplx', None)
    V = case['model']['v_template'].shape[0]
    assert 100 * 1024 < V * 12 < 160 * 1024 - 256            # the largest frame the staged kernel takes
    dev = nc.device_model(case)
    nc.check_body(dev, case, 17, kernels=('lds',))
    dev.close()


def test_virtual_markers_on_smplh_batches_streams_and_device_buffers():
    from moshpp_amd import capi
    case = nc.mesh_case('smplh', None)
    F, M = 140, 53
    pose, trans = nc.inputs(case, F)
    # frames of every batch (64 + 64 + 12) and of both 128-frame tiles of the f32 export are held to the oracle
    rows = np.array([0, 1, 2, 3, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 131, 139])
    b = nc.normal_bound(nc.oracle_verts(case['m'], pose[rows], trans[rows]), case['faces'], nc.F32_TOL)
    vids = nc.pick_marker_vids(b, case['faces'], M)
    dist = np.full(M, 0.0095); dist[5] = 0.0; dist[6] = -0.01
    dev = nc.device_model(case)
    with nc.env(MOSHII_VM_BATCH='64'):                        # three batches, the last one of 12 frames
        host = nc.check_markers(dev, case, pose, trans, vids, dist, rows=rows)
        # device buffers on a stream of their own: the same bits as the host-buffer call
        hip = C.CDLL('libamdhip64.so')      # (the runtime libmoshii already brought into the process)
        stream = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
        try:
            for dt in (np.float32, np.float64):
                p, t = (np.ascontiguousarray(a, dtype=dt) for a in (pose, trans))
                bufs = [capi.DeviceBuffer(n) for n in (p.nbytes, t.nbytes, F * M * 3 * p.itemsize, F * M * 3 * p.itemsize)]
                bufs[0].upload(p); bufs[1].upload(t)
                dev.virtual_markers_device(F, bufs[0].ptr, bufs[1].ptr, vids, dist, bufs[2].ptr, bufs[3].ptr, stream=stream,
                                           f32=dt == np.float32)
                assert hip.hipStreamSynchronize(stream) == 0
                np.testing.assert_array_equal(bufs[2].download(np.zeros((F, M, 3), dtype=dt)), host[dt][0])
                np.testing.assert_array_equal(bufs[3].download(np.zeros((F, M, 3), dtype=dt)), host[dt][1])
                for bf in bufs:
                    bf.close()
        finally:
            hip.hipStreamDestroy(stream)
    whole = dev.virtual_markers(pose, trans, vids, dist, dtype=np.float32)      # the default batch: one
    np.testing.assert_array_equal(whole, host[np.float32][0])
    dev.close()


def test_export_bits_before_and_after_normals_calls():
    case = nc.mesh_case('smpl', 1500)
    pose, trans = nc.inputs(case, 140)
    dev = nc.device_model(case, faces=None)
    before = dev.lbs_forward(pose, trans, dtype=np.float32), dev.lbs_forward(pose[:5], trans[:5])
    dev.set_faces(case['faces'])
    dev.vertex_normals(before[0])
    with nc.env(MOSHII_VM_BATCH='48'):
        dev.virtual_markers(pose, trans, [1, 2, 3], [0.01, 0.01, 0.01], dtype=np.float32)
    dev.virtual_markers(pose[:5], trans[:5], [1, 2, 3], [0.01, 0.01, 0.01], dtype=np.float64)
    after = dev.lbs_forward(pose, trans, dtype=np.float32), dev.lbs_forward(pose[:5], trans[:5])
    dev.close()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


def test_device_buffer_normals_follow_the_export_on_one_stream():
    """Model.lbs_forward_with_normals (mosh_head.stageii_vertices(return_normals=True)): export and normals chained on the device."""
    case = nc.mesh_case('mano', 778)
    pose, trans = nc.inputs(case, 9)
    dev = nc.device_model(case)
    v, n = dev.lbs_forward_with_normals(pose, trans, dtype=np.float32)
    np.testing.assert_array_equal(v, dev.lbs_forward(pose, trans, dtype=np.float32))
    np.testing.assert_array_equal(n, dev.vertex_normals(v))
    dev.close()


def test_more_than_65535_vertices():
    """32-bit pairs in the face table, and an f32 frame beyond the LDS budget: the gather kernel without being asked."""
    nc.check_wide_body()
