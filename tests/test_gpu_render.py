"""GPU: the shaded previews (moshii_render_*, moshii_render_posed_*) on the device -- every scene of tests/render_common.py against its
NumPy reference in both input types, run-to-run identity, the fused entry across a batch boundary with and without a free shape block,
device buffers on a stream, the launch report, and StageIISolver.render of a solved sequence."""
import ctypes as C

import numpy as np
import pytest

from tests import normals_common as nc
from tests import render_common as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_hand_made_scenes_against_the_reference(dtype):
    from moshpp_amd import capi
    dev = capi.Model(**rc.hand_model())
    for name, s in rc.hand_scenes().items():
        dev.set_faces(s['faces'])
        got, _ = rc.render_and_check(dev, s['verts'], s['faces'], [rc.HAND_CAM], rc.HAND_SIZE, s['points'], s['radius'], s['prgb'], dtype,
                                     f'{name} {np.dtype(dtype).name}')
        if name.startswith('quad'):
            assert (got['ids'] >= 0).sum() == rc.QUAD_PIXELS
    dev.close()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('model_type', sorted(rc.BODIES))
def test_body_scenes_against_the_reference_and_twice_the_same_bits(model_type, dtype):
    from moshpp_amd import capi
    b = rc.body_scene(model_type)
    dev = nc.device_model(b['case'])
    for cname, cams in b['cameras'].items():
        got, _ = rc.render_and_check(dev, b['verts'], b['faces'], cams, rc.BODY_SIZE, b['points'], b['radius'], b['prgb'], dtype,
                                     f'{model_type} {cname} {np.dtype(dtype).name}')
        again = dev.render(rc.as_input(b['verts'], dtype), [rc.capi_camera(c) for c in cams], rc.BODY_SIZE, points=rc.as_input(b['points'], dtype),
                           point_rgb=b['prgb'], point_radius=b['radius'], body_rgb=rc.BODY, bg_rgb=rc.BG, ambient=rc.AMBIENT)
        name, lds, threads = capi.last_launch_info()
        assert name == 'k_render_tiles' and threads == 1024 and 76 * 1024 <= lds <= 80 * 1024
        for k in ('rgb', 'ids', 'depth'):
            np.testing.assert_array_equal(again[k], got[k])
    dev.close()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_render_posed_equals_render_of_the_export_across_a_batch_boundary(dtype):
    b = rc.body_scene('smplh')
    cams = [rc.capi_camera(c) for c in b['cameras']['per_frame']]
    kw = dict(points=rc.as_input(b['points'], dtype), point_rgb=b['prgb'], point_radius=b['radius'])
    dev = nc.device_model(b['case'])
    verts = dev.lbs_forward(b['pose'], b['trans'], dtype=dtype)
    want = dev.render(verts, cams, rc.BODY_SIZE, **kw)
    # the export of each batch, as the fused call makes it (the f32 export's roundings depend on the frames of a call)
    split = np.concatenate([dev.lbs_forward(b['pose'][a:a + 2], b['trans'][a:a + 2], dtype=dtype) for a in (0, 2)])
    want_split = dev.render(split, cams, rc.BODY_SIZE, **kw)
    with nc.env(MOSHII_VM_BATCH='2'):                                    # F = 3: a batch of two frames, then one
        got = dev.render_posed(b['pose'], b['trans'], cams, rc.BODY_SIZE, dtype=dtype, **kw)
    whole = dev.render_posed(b['pose'], b['trans'], cams, rc.BODY_SIZE, dtype=dtype, **kw)
    dev.close()
    assert (want['ids'] >= len(b['faces'])).any() and ((want['ids'] >= 0) & (want['ids'] < len(b['faces']))).any()
    for k in ('rgb', 'ids', 'depth'):
        np.testing.assert_array_equal(got[k], want_split[k])
        np.testing.assert_array_equal(whole[k], want[k])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_render_posed_with_a_free_shape_block_across_a_batch_boundary(dtype):
    """The last three shapedirs columns of the SMPL-H body declared free: per-frame coefficients move rest positions and joints, and the
    fused entry still gives the bits of render(lbs_forward(..., shape))."""
    b = rc.body_scene('smplh')
    dev = nc.device_model(b['case'])
    NB = np.asarray(b['case']['model']['shapedirs']).shape[-1]
    dev.set_free_shape(NB - 3, 3)
    shape = np.random.default_rng(8).normal(0, 1.5, (rc.BODY_F, 3))
    cam = rc.capi_camera(b['cameras']['fitted'][0])
    verts = dev.lbs_forward(b['pose'], b['trans'], dtype=dtype, shape=shape)
    plain = dev.lbs_forward(b['pose'], b['trans'], dtype=dtype)
    moved = np.abs(verts - plain).max()
    print(f'the coefficients move the mesh by up to {moved:.3e} m')
    assert moved > 1e-3
    want = dev.render(verts, cam, rc.BODY_SIZE)
    # the export of each batch, as the fused call makes it: the f32 export scales the coefficients by a power of two chosen from the
    # frames of the call, so its roundings are those of the batch, not of the whole sequence
    split = np.concatenate([dev.lbs_forward(b['pose'][a:a + 2], b['trans'][a:a + 2], dtype=dtype, shape=shape[a:a + 2]) for a in (0, 2)])
    want_split = dev.render(split, cam, rc.BODY_SIZE)
    with nc.env(MOSHII_VM_BATCH='2'):
        got = dev.render_posed(b['pose'], b['trans'], cam, rc.BODY_SIZE, shape=shape, dtype=dtype)
    whole = dev.render_posed(b['pose'], b['trans'], cam, rc.BODY_SIZE, shape=shape, dtype=dtype)
    frozen = dev.render_posed(b['pose'], b['trans'], cam, rc.BODY_SIZE, dtype=dtype)
    dev.close()
    assert (want['ids'] >= 0).any()
    for k in ('rgb', 'ids', 'depth'):
        np.testing.assert_array_equal(got[k], want_split[k])
        np.testing.assert_array_equal(whole[k], want[k])
    assert (frozen['depth'] != want['depth']).any()


def test_device_pointer_path_equals_host_pointer_path():
    from moshpp_amd import capi
    b = rc.body_scene('smplh')
    W, H = rc.BODY_SIZE
    cams = [rc.capi_camera(c) for c in b['cameras']['fitted']]
    dev = nc.device_model(b['case'])
    hip = C.CDLL('libamdhip64.so')      # (the runtime libmoshii already brought into the process)
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        for dtype in (np.float32, np.float64):
            pose, trans = (np.ascontiguousarray(a, dtype=dtype) for a in (b['pose'], b['trans']))
            pts = rc.as_input(b['points'], dtype)
            F, N = len(pose), pts.shape[1]
            verts = dev.lbs_forward(pose, trans, dtype=dtype)
            kw = dict(point_rgb=b['prgb'], point_radius=b['radius'])
            want = dev.render(verts, cams, rc.BODY_SIZE, points=pts, **kw)
            bufs = [capi.DeviceBuffer(n) for n in (verts.nbytes, pts.nbytes, pose.nbytes, trans.nbytes, F * H * W * 3, F * H * W * 4, F * H * W * 4)]
            bufs[0].upload(verts); bufs[1].upload(pts); bufs[2].upload(pose); bufs[3].upload(trans)
            outs = (np.zeros((F, H, W, 3), np.uint8), np.zeros((F, H, W), np.int32), np.zeros((F, H, W), np.float32))
            f32 = dtype == np.float32
            dev.render_device(F, bufs[0].ptr, cams, rc.BODY_SIZE, N=N, points_ptr=bufs[1].ptr, rgb_ptr=bufs[4].ptr, ids_ptr=bufs[5].ptr,
                              depth_ptr=bufs[6].ptr, stream=stream, f32=f32, **kw)
            assert hip.hipStreamSynchronize(stream) == 0
            for k, buf, o in zip(('rgb', 'ids', 'depth'), bufs[4:], outs):
                np.testing.assert_array_equal(buf.download(o), want[k])
                buf.upload(np.zeros_like(o))
            # the fused entry on device buffers, the colour alone
            dev.render_posed_device(F, bufs[2].ptr, bufs[3].ptr, cams, rc.BODY_SIZE, N=N, points_ptr=bufs[1].ptr, rgb_ptr=bufs[4].ptr, stream=stream,
                                    f32=f32, **kw)
            assert hip.hipStreamSynchronize(stream) == 0
            np.testing.assert_array_equal(bufs[4].download(outs[0]), want['rgb'])
            assert (bufs[5].download(outs[1]) == 0).all()                # a null output is left alone
            for bf in bufs:
                bf.close()
    finally:
        hip.hipStreamDestroy(stream)
    dev.close()


def test_solver_render_of_a_solved_smplh_sequence():
    """One 512 x 512 x 8-frame StageIISolver.render after a short real solve: shape and dtype, a background share strictly between 5 %
    and 95 %, and both marker colours in the picture."""
    from moshpp_amd import preview, synth, workload
    dd = synth.synth_mesh_model('smplh', seed=1000, n_verts=1500)
    F, M = 8, 53
    job = workload.make_job('smplh', F, M, seed=1000, dd=dd)
    solver = workload.make_solver(job)
    obs, vis = np.asarray(job['obs'], dtype=np.float64), np.asarray(job['vis'], dtype=bool)
    out = solver.solve(obs, vis, chain_mode='sequential')
    res = solver.render(out, obs=obs, vis=vis, size=(512, 512), up='y')      # (the synthetic bodies stand along +y)
    rgb = res['rgb']
    assert rgb.shape == (F, 512, 512, 3) and rgb.dtype == np.uint8
    assert res['ids'].shape == (F, 512, 512) and res['ids'].dtype == np.int32
    assert res['depth'].shape == (F, 512, 512) and res['depth'].dtype == np.float32
    share = (res['ids'] < 0).mean()
    print(f'background share {100 * share:.1f} %')
    assert 0.05 < share < 0.95
    nf = len(np.asarray(dd['f']))
    assert ((res['ids'] >= nf) & (res['ids'] < nf + M)).any() and (res['ids'] >= nf + M).any()
    flat = rgb.reshape(-1, 3).astype(np.int32)                          # shading scales a colour, its channel ratios stay
    red = (flat[:, 0] > 2 * flat[:, 1]) & (flat[:, 0] > 2 * flat[:, 2])
    blue = (flat[:, 2] > 2 * flat[:, 0]) & (flat[:, 2] > 1.5 * flat[:, 1])
    print(f'{int(red.sum())} pixels in the observed markers\' colour, {int(blue.sum())} in the simulated markers\'')
    assert tuple(preview.OBSERVED_RGB) == (215, 48, 39) and tuple(preview.SIMULATED_RGB) == (44, 101, 201)
    assert red.any() and blue.any()
