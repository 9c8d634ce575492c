"""CPU: the shaded previews (moshii_render_*, moshii_render_posed_*) in the emulation build -- lbs_forward.hip and moshii_api.hip
compiled unchanged for the host, a tile's 1024 lanes run as fibers, its ballots as rendezvous, its list counter as an atomic.
Reference, scenes, checker and bounds: tests/render_common.py."""
import ctypes as C

import numpy as np
import pytest

from tests import normals_common as nc
from tests import render_common as rc
from tests.emu.emu_moshii import emulated_libmoshii


def _hand_device():
    from moshpp_amd import capi
    return capi.Model(**rc.hand_model())


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_hand_made_scenes_against_the_reference_in_emulation(dtype):
    with emulated_libmoshii():
        dev = _hand_device()
        for name, s in rc.hand_scenes().items():
            dev.set_faces(s['faces'])
            got, ref = rc.render_and_check(dev, s['verts'], s['faces'], [rc.HAND_CAM], rc.HAND_SIZE, s['points'], s['radius'], s['prgb'], dtype,
                                           f'{name} {np.dtype(dtype).name}')
            if name.startswith('quad'):
                assert (got['ids'] >= 0).sum() == rc.QUAD_PIXELS
        dev.close()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_mano_body_scene_against_the_reference_in_emulation(dtype):
    b = rc.body_scene('mano')
    with emulated_libmoshii():
        dev = nc.device_model(b['case'])
        for cname, cams in b['cameras'].items():
            rc.render_and_check(dev, b['verts'], b['faces'], cams, rc.BODY_SIZE, b['points'], b['radius'], b['prgb'], dtype,
                                f'mano {cname} {np.dtype(dtype).name}')
        dev.close()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_render_posed_equals_render_of_the_export_across_a_batch_boundary_in_emulation(dtype):
    from moshpp_amd import capi
    b = rc.body_scene('mano')
    cams = [rc.capi_camera(c) for c in b['cameras']['per_frame']]
    pts = rc.as_input(b['points'], dtype)
    kw = dict(points=pts, point_rgb=b['prgb'], point_radius=b['radius'])
    with emulated_libmoshii():
        dev = nc.device_model(b['case'])
        verts = dev.lbs_forward(b['pose'], b['trans'], dtype=dtype)
        want = dev.render(verts, cams, rc.BODY_SIZE, **kw)
        # the export of each batch, as the fused call makes it (the f32 export's roundings depend on the frames of a call)
        vsplit = np.concatenate([dev.lbs_forward(b['pose'][a:a + 2], b['trans'][a:a + 2], dtype=dtype) for a in (0, 2)])
        want_split = dev.render(vsplit, cams, rc.BODY_SIZE, **kw)
        whole = dev.render_posed(b['pose'], b['trans'], cams, rc.BODY_SIZE, dtype=dtype, **kw)
        with nc.env(MOSHII_VM_BATCH='2'):                                # F = 3: a batch of two frames, then one
            got = dev.render_posed(b['pose'], b['trans'], cams, rc.BODY_SIZE, dtype=dtype, **kw)
            split = dev.render(verts, cams, rc.BODY_SIZE, **kw)
        name, lds, threads = capi.last_launch_info()
        assert name == 'k_render_tiles' and threads == 1024 and 76 * 1024 <= lds <= 80 * 1024
        dev.close()
    assert (want['ids'] >= 0).any() and (want['ids'] >= len(b['faces'])).any()
    for k in ('rgb', 'ids', 'depth'):
        np.testing.assert_array_equal(got[k], want_split[k])
        np.testing.assert_array_equal(whole[k], want[k])
        np.testing.assert_array_equal(split[k], want[k])
    assert len({want['rgb'][f].tobytes() for f in range(3)}) == 3         # three cameras, three pictures


def test_library_refusals_in_emulation():
    """The C ABI's own checks, each with MOSHII_ERR_ARG and a message that names the fault; F == 0 launches nothing; null outputs are
    skipped."""
    from moshpp_amd import capi
    s = rc.hand_scenes()['markers']
    W, H = rc.HAND_SIZE
    v = rc.as_input(s['verts'], np.float32)
    p = rc.as_input(s['points'], np.float32)
    N = p.shape[1]
    with emulated_libmoshii():
        lib = capi.load()
        assert lib.moshii_version() >= 107
        dev = _hand_device()
        cam = (capi.Camera * 1)(rc.capi_camera(rc.HAND_CAM))
        prgb, prad = np.ascontiguousarray(s['prgb']), np.ascontiguousarray(s['radius'])

        def opts(**kw):
            o = capi.RenderOpts()
            o.width, o.height, o.n_cameras, o.cameras = W, H, 1, cam
            o.body_rgb[:] = rc.BODY; o.bg_rgb[:] = rc.BG
            o.ambient = rc.AMBIENT
            o.point_rgb = prgb.ctypes.data_as(C.POINTER(C.c_uint8)); o.point_radius = prad.ctypes.data_as(C.POINTER(C.c_double))
            for k, val in kw.items():
                setattr(o, k, val)
            return o
        rgb = np.zeros((1, H, W, 3), np.uint8); ids = np.zeros((1, H, W), np.int32); depth = np.zeros((1, H, W), np.float32)

        def call(o, F=1, verts=v.ctypes.data, n=N, points=p.ctypes.data, outs=(rgb, ids, depth), fn=lib.moshii_render_f32, handle=None):
            return fn(dev.handle if handle is None else handle, F, verts, n, points, C.byref(o) if o is not None else None,
                      *(a.ctypes.data if a is not None else None for a in outs), capi.BUFFERS_HOST, None)
        assert call(opts()) == -1 and b'moshii_model_set_faces' in lib.moshii_last_error()          # before the faces are set
        dev.set_faces(s['faces'])
        assert call(opts()) == 0
        want = {k: a.copy() for k, a in (('rgb', rgb), ('ids', ids), ('depth', depth))}
        py = dev.render(v, rc.capi_camera(rc.HAND_CAM), rc.HAND_SIZE, points=p, point_rgb=prgb, point_radius=prad, body_rgb=rc.BODY, bg_rgb=rc.BG,
                        ambient=rc.AMBIENT)
        for k in want:
            np.testing.assert_array_equal(py[k], want[k])
        for o, frag in ((None, b'opts is null'), (opts(cameras=None), b'cameras is null'), (opts(width=0), b'1 .. 4096'),
                        (opts(height=4097), b'1 .. 4096'), (opts(n_cameras=2), b'n_cameras must be 1 or F'), (opts(ambient=1.25), b'ambient'),
                        (opts(ambient=float('nan')), b'ambient'), (opts(point_rgb=None), b'point_rgb'), (opts(point_radius=None), b'point_radius')):
            assert call(o) == -1 and frag in lib.moshii_last_error(), frag
        assert call(opts(), points=None) == -1 and b'points' in lib.moshii_last_error()
        assert call(opts(), outs=(None, None, None)) == -1 and b'all null' in lib.moshii_last_error()
        assert call(opts(), F=-1) == -1 and b'negative F or N' in lib.moshii_last_error()
        assert call(opts(), n=-1) == -1 and b'negative F or N' in lib.moshii_last_error()
        assert call(opts(), verts=None) == -1 and b'verts is null' in lib.moshii_last_error()
        assert lib.moshii_render_f64(None, 1, None, 0, None, C.byref(opts()), rgb.ctypes.data, None, None, 0, None) == -1
        assert b'null model' in lib.moshii_last_error()
        posed = lib.moshii_render_posed_f32
        pose, trans = np.zeros((1, 6), np.float32), np.zeros((1, 3), np.float32)
        assert posed(dev.handle, 1, None, trans.ctypes.data, None, 0, None, C.byref(opts()), rgb.ctypes.data, None, None, 0, None) == -1
        assert b'pose or trans' in lib.moshii_last_error()
        assert posed(dev.handle, 1, pose.ctypes.data, trans.ctypes.data, pose.ctypes.data, 0, None, C.byref(opts()), rgb.ctypes.data, None, None, 0, None) == -1
        assert b'moshii_model_set_free_shape' in lib.moshii_last_error()
        # points are optional: N == 0 with everything about them null
        assert call(opts(point_rgb=None, point_radius=None), n=0, points=None) == 0
        assert set(np.unique(ids)) == {-1, 0}
        # F == 0: MOSHII_OK, nothing launched, nothing written (n_cameras = 1 is still in {1, F})
        dev.vertex_normals(v)
        assert capi.last_launch_info()[0] == 'k_vn_lds'
        rgb[:] = 7; ids[:] = 7; depth[:] = 7
        assert call(opts(), F=0, verts=None) == 0
        assert capi.last_launch_info()[0] == 'k_vn_lds' and (rgb == 7).all() and (ids == 7).all() and (depth == 7).all()
        # null outputs are skipped: each output alone equals its part of the full call
        for keep in range(3):
            outs = [None, None, None]
            bufs = (np.zeros_like(rgb), np.zeros_like(ids), np.zeros_like(depth))
            outs[keep] = bufs[keep]
            assert call(opts(), outs=tuple(outs)) == 0
            np.testing.assert_array_equal(bufs[keep], want[('rgb', 'ids', 'depth')[keep]])
        only = dev.render(v, rc.capi_camera(rc.HAND_CAM), rc.HAND_SIZE, points=p, point_rgb=prgb, point_radius=prad, outputs=('ids',))
        assert set(only) == {'ids'}
        np.testing.assert_array_equal(only['ids'], want['ids'])
        assert dev.render(np.zeros((0, rc.HAND_V, 3), np.float32), rc.capi_camera(rc.HAND_CAM), rc.HAND_SIZE)['rgb'].shape == (0, H, W, 3)
        dev.close()


def _preview_data(case, T):
    """A small Stage-II result with observed and simulated markers (ragged, as mosh_stageii stores them)."""
    from tests.test_normals_emulation import _stageii_result
    sm, data, _ = _stageii_result(case, T)
    rng = np.random.default_rng(1)
    pose, _ = nc.inputs(case, T, seed=9)                 # (_stageii_result's poses; its translations scatter the frames over metres)
    data['trans'] = rng.normal(0, 0.02, (T, 3))
    verts = nc.oracle_verts(case['m'], pose, data['trans'])
    vids = rng.choice(verts.shape[1], 5, replace=False)
    labels = [f'M{i}' for i in range(5)]
    nrm = rc.numpy_normals(verts, case['faces'])
    sim = verts[:, vids] + 0.0095 * nrm[:, vids]
    obs = sim + rng.normal(0, 0.004, sim.shape)
    seen = [[0, 1, 2, 3, 4], [0, 2, 4], [1, 2, 3, 4], [0, 1, 2, 3, 4]][:T]
    dbg = data['stageii_debug_details']
    dbg['markers_obs'] = [obs[f][s] for f, s in enumerate(seen)]
    dbg['markers_sim'] = [sim[f][s] for f, s in enumerate(seen)]
    dbg['labels_obs'] = [[labels[i] for i in s] for s in seen]
    data['latent_labels'] = labels
    return sm, data


def test_mosh_head_stageii_preview_in_emulation(tmp_path):
    from moshpp_amd import mosh_head, png_io, preview
    case = nc.mesh_case('mano', 300)
    sm, data = _preview_data(case, 4)
    out_dir = tmp_path / 'sub' / 'preview'
    with emulated_libmoshii(), nc.env(MOSHII_VM_BATCH='3'):
        old = mosh_head.PREVIEW_BATCH
        mosh_head.PREVIEW_BATCH = 3                      # four frames: two calls
        try:
            res = mosh_head.stageii_preview(data, out_dir=str(out_dir), surface_model=sm, size=(72, 56), view=(20.0, 15.0), up='y',
                                            contact_sheet_columns=3, marker_radius=0.006)
            sub = mosh_head.stageii_preview(data, surface_model=sm, frame_ids=[2, 0], size=(72, 56), view=(20.0, 15.0), up='y', marker_radius=0.006)
            with pytest.raises(FileExistsError, match='frame_000000.png'):
                mosh_head.stageii_preview(data, out_dir=str(out_dir), surface_model=sm, size=(72, 56))
        finally:
            mosh_head.PREVIEW_BATCH = old
    assert set(res) == {'images', 'camera', 'frame_ids', 'fnames', 'contact_sheet', 'contact_sheet_fname'}
    imgs = res['images']
    assert imgs.shape == (4, 56, 72, 3) and imgs.dtype == np.uint8 and list(res['frame_ids']) == [0, 1, 2, 3]
    assert [f.split('/')[-1] for f in res['fnames']] == ['frame_%06d.png' % i for i in range(4)]
    for fn, img in zip(res['fnames'], imgs):
        np.testing.assert_array_equal(png_io.read_png(fn), img)
    np.testing.assert_array_equal(png_io.read_png(res['contact_sheet_fname']), res['contact_sheet'])
    np.testing.assert_array_equal(res['contact_sheet'], preview.contact_sheet(imgs, 3))
    assert res['contact_sheet'].shape == (112, 216, 3)
    flat = imgs.reshape(4, -1, 3)
    for f in range(4):                                   # background, body, and both marker colours in every frame
        bg_share = (flat[f] == 255).all(-1).mean()
        assert 0.05 < bg_share < 0.95
        red = (flat[f][:, 0] > 1.5 * flat[f][:, 2]) & (flat[f][:, 0] > 2 * flat[f][:, 1])
        blue = (flat[f][:, 2] > 1.5 * flat[f][:, 0]) & (flat[f][:, 2] > 1.5 * flat[f][:, 1])
        assert red.any() and blue.any(), f
    # a subset is rendered with its own camera (the box of its own frames) and writes nothing
    assert sub['fnames'] == [] and sub['contact_sheet'] is None and list(sub['frame_ids']) == [2, 0] and sub['images'].shape == (2, 56, 72, 3)
    assert sorted(p.name for p in out_dir.iterdir()) == ['contact_sheet.png'] + ['frame_%06d.png' % i for i in range(4)]
