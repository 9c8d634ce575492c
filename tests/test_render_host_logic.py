"""CPU, no library kernels: the host side of the shaded previews -- the camera builder, the PNG writer / reader, contact sheets, the
library's version, symbols and struct layouts, the Python-side refusals -- and the self-checks of the tests' own rendering reference
(tests/render_common.py): its two input conditions on every committed scene, the quad's exact pixel count, the top-left rule."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from moshpp_amd import capi, png_io, preview
from tests import render_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- camera builder ----
def _joints(seed=0, up='z'):
    rng = np.random.default_rng(seed)
    j = rng.normal(0, 1, (7, 20, 3)) * np.array([0.3, 0.2, 0.8]) + np.array([0.4, -1.0, 0.9])
    return j if up == 'z' else j[..., [0, 2, 1]]


@pytest.mark.parametrize('up', ['z', 'y'])
@pytest.mark.parametrize('view', ['front', 'back', 'left', 'right', 'top', (30.0, 20.0), (-140.0, -35.0)])
@pytest.mark.parametrize('size', [(96, 80), (64, 128)])
def test_preview_camera_frames_every_joint(view, up, size):
    j = _joints(up=up)
    margin = 1.15
    cam = preview.preview_camera(j, size, view=view, up=up, margin=margin)
    c = cam.as_dict()
    R = c['R']
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
    u, v, z = preview.project(cam, j)
    W, H = size
    assert (z > c['znear']).all() and c['znear'] > 0
    # the box grown by `margin` fits, so the joints themselves keep clear of the border (perspective included: the grown box's corners
    # are the extremes of the joints' rays scaled about the centre)
    assert u.min() >= 0 and u.max() <= W and v.min() >= 0 and v.max() <= H
    # ... and the framing is tight: the grown box touches the border on one axis
    lo, hi = j.reshape(-1, 3).min(0), j.reshape(-1, 3).max(0)
    ctr, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * margin
    corners = ctr + half * np.array([[a, b, d] for a in (-1, 1) for b in (-1, 1) for d in (-1, 1)])
    cu, cv, cz = preview.project(cam, corners)
    assert cu.min() >= -1e-9 and cu.max() <= W + 1e-9 and cv.min() >= -1e-9 and cv.max() <= H + 1e-9
    assert min(cu.min(), W - cu.max(), cv.min(), H - cv.max()) < 1e-6
    assert abs(c['znear'] - 0.1 * cz.min()) < 1e-12
    # it looks at the centre, and the world's up axis points up in the image (for a level or tilted view)
    uc, vc, _ = preview.project(cam, ctr)
    assert abs(uc - 0.5 * W) < 1e-9 and abs(vc - 0.5 * H) < 1e-9
    if view != 'top':
        up_vec = np.array([0, 0, 1.0]) if up == 'z' else np.array([0, 1.0, 0])
        _, v_up, _ = preview.project(cam, ctr + 0.01 * up_vec)
        assert v_up < vc


def test_preview_camera_views_differ_and_refusals():
    j = _joints()
    front, back = preview.preview_camera(j, (64, 64), 'front').as_dict(), preview.preview_camera(j, (64, 64), 'back').as_dict()
    np.testing.assert_allclose(front['R'][2], -back['R'][2], atol=1e-12)          # opposite viewing directions
    np.testing.assert_allclose(front['R'][2], [0, 1, 0], atol=1e-12)              # up = 'z': the front camera looks along +y
    np.testing.assert_allclose(preview.preview_camera(j, (64, 64), 'top').as_dict()['R'][2], [0, 0, -1], atol=1e-12)
    np.testing.assert_allclose(preview.preview_camera(j[..., [0, 2, 1]], (64, 64), 'front', up='y').as_dict()['R'][2], [0, 0, -1], atol=1e-12)
    for kw, match in ((dict(view='side'), 'view'), (dict(up='x'), 'up'), (dict(margin=0.5), 'margin'), (dict(size=(0, 5)), 'size')):
        args = dict(joints=j, size=(64, 64)); args.update(kw)
        with pytest.raises(ValueError, match=match):
            preview.preview_camera(**args)
    with pytest.raises(ValueError, match='finite'):
        preview.preview_camera(np.full((2, 3, 3), np.nan), (64, 64))
    one = preview.preview_camera(np.zeros((1, 1, 3)), (64, 64))                 # a single point still gives a camera in front of it
    assert preview.project(one, np.zeros(3))[2] > one.znear > 0


# ---- PNG ----
def _chunks(data):
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack('>I', data[at:at + 4])
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n], struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0]))
        at += 12 + n
    return out


@pytest.mark.parametrize('shape', [(5, 7), (1, 1), (16, 33), (3, 2)])
@pytest.mark.parametrize('filter_type', [0, 1, 2, 3, 4])
def test_png_round_trip_is_bit_exact(tmp_path, shape, filter_type):
    rng = np.random.default_rng(shape[1] + filter_type)
    img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    fn = tmp_path / 'a.png'
    png_io.write_png(str(fn), img, filter_type=filter_type)
    data = fn.read_bytes()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    ch = _chunks(data)
    assert [k for k, _, _ in ch] == [b'IHDR', b'IDAT', b'IEND']
    for kind, body, crc in ch:
        assert crc == zlib.crc32(kind + body) & 0xffffffff
    assert struct.unpack('>IIBBBBB', ch[0][1]) == (shape[1], shape[0], 8, 2, 0, 0, 0)     # 8-bit truecolour, non-interlaced
    rows = np.frombuffer(zlib.decompress(ch[1][1]), dtype=np.uint8).reshape(shape[0], 1 + 3 * shape[1])
    assert (rows[:, 0] == filter_type).all()
    back = png_io.read_png(str(fn))
    assert back.dtype == np.uint8
    np.testing.assert_array_equal(back, img)


def test_png_refusals(tmp_path):
    with pytest.raises(ValueError, match='uint8'):
        png_io.write_png(str(tmp_path / 'x.png'), np.zeros((4, 4, 3)))
    with pytest.raises(ValueError, match='uint8'):
        png_io.write_png(str(tmp_path / 'x.png'), np.zeros((4, 4), dtype=np.uint8))
    good = png_io.encode_png(np.zeros((2, 2, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match='signature'):
        png_io.decode_png(b'JUNK' + good)
    broken = bytearray(good); broken[20] ^= 1                                     # inside IHDR: its CRC no longer matches
    with pytest.raises(ValueError, match='CRC'):
        png_io.decode_png(bytes(broken))
    with pytest.raises(ValueError, match='truncated|missing'):
        png_io.decode_png(good[:-6])


def test_no_imaging_library_is_imported():
    import sys
    for mod in ('moshpp_amd.png_io', 'moshpp_amd.preview'):
        src = open(sys.modules[mod].__file__).read()
        for lib in ('PIL', 'cv2', 'imageio', 'matplotlib', 'skimage'):
            assert f'import {lib}' not in src and f'from {lib}' not in src


# ---- contact sheet ----
def test_contact_sheet_layout():
    imgs = np.stack([np.full((4, 6, 3), 10 * (i + 1), dtype=np.uint8) for i in range(5)])
    sheet = preview.contact_sheet(imgs, 3)
    assert sheet.shape == (8, 18, 3) and sheet.dtype == np.uint8
    for i in range(5):
        r, c = divmod(i, 3)
        assert (sheet[4 * r:4 * r + 4, 6 * c:6 * c + 6] == 10 * (i + 1)).all()
    assert (sheet[4:, 12:] == 255).all()                                           # the empty cell
    assert preview.contact_sheet(imgs, 9).shape == (4, 30, 3)                      # fewer images than columns: one row of them
    assert preview.contact_sheet(imgs, 1).shape == (20, 6, 3)
    assert (preview.contact_sheet(imgs, 2, fill=0)[8:, 6:] == 0).all()
    with pytest.raises(ValueError, match='columns'):
        preview.contact_sheet(imgs, 0)
    with pytest.raises(ValueError, match='uint8'):
        preview.contact_sheet(imgs.astype(np.float32), 2)


# ---- the library ----
@pytest.fixture(scope='module')
def lib():
    from moshpp_amd import build
    build.build(force=False, verbose=False)
    return capi.load()


def test_library_version_and_render_symbols(lib):
    assert lib.moshii_version() >= 107
    for name in ('moshii_render_f32', 'moshii_render_f64', 'moshii_render_posed_f32', 'moshii_render_posed_f64'):
        assert name in capi.EXPORTS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, 'include', 'moshii.h')).read()
    assert 'tools/visualization.py:96-130' in hdr and 'THERE IS NO CLIPPING' in hdr


def test_render_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of moshii_camera and moshii_render_opts as gcc sees them equal the ctypes mirrors."""
    structs = {'moshii_camera': capi.Camera, 'moshii_render_opts': capi.RenderOpts}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "moshii.h"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('return 0;}')
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert C.sizeof(capi.Camera) == 17 * 8
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f'{cname}.{fname}']) == getattr(cls, fname).offset, (cname, fname)


def test_render_plan_layout(tmp_path):
    """export_plan::plan_render compiled on its own by g++: the parts of a render batch follow each other on 16-byte boundaries."""
    prog = r'''
#include "export_plan.h"
#include <cstdio>
static void row(size_t fb, long long F, long long V, long long N, long long nc, bool posed, int ov) {
    const export_plan::RenderBatch b = export_plan::plan_render(fb, F, V, N, nc, posed, ov);
    printf("%lld %zu %zu %zu %zu %zu %zu %zu\n", b.batch, b.off_normals, b.off_rec, b.off_mrec, b.off_cams, b.off_radius, b.off_prgb, b.bytes);
}
int main() {
    row(603 * 12, 3, 603, 8, 1, true, 2);
    row(603 * 12, 3, 603, 8, 3, false, 0);
    row(6890 * 12, 4000, 6890, 106, 1, true, 0);
    row(6890 * 24, 100000, 6890, 0, 1, false, 0);
    return 0;
}
'''
    src, exe = tmp_path / 'plan.cpp', tmp_path / 'plan'
    src.write_text(prog)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'moshpp_amd', 'csrc'), str(src), '-o', str(exe)])
    rows = [[int(x) for x in l.split()] for l in subprocess.check_output([str(exe)]).decode().splitlines()]
    a16 = lambda n: (n + 15) // 16 * 16
    # MANO-sized, posed, MOSHII_VM_BATCH = 2: meshes 2 * 7236 = 14472 -> 14480; normals end 28952 -> 28960; records 2 * 603 * 32
    fb = 603 * 12
    n0 = a16(2 * fb); r0 = a16(n0 + 2 * fb); m0 = a16(r0 + 2 * 603 * 32); c0 = a16(m0 + 2 * 8 * 40); d0 = a16(c0 + 136); p0 = a16(d0 + 64)
    assert rows[0] == [2, n0, r0, m0, c0, d0, p0, p0 + 24]
    # the caller's meshes: no mesh part, the normals lead; three cameras
    r1 = a16(3 * fb); m1 = a16(r1 + 3 * 603 * 32); c1 = a16(m1 + 3 * 8 * 40); d1 = a16(c1 + 3 * 136); p1 = a16(d1 + 64)
    assert rows[1] == [3, 0, r1, m1, c1, d1, p1, p1 + 24]
    # SMPL-H f32 posed: 268435456 / (2 * 82680 + 6890 * 32 + 106 * 40) = 689.6 -> 689 -> five 128-frame tiles
    assert rows[2][0] == 640
    # never more frames than the tile kernel's grid.z takes
    assert rows[3][0] == 128 * (268435456 // (6890 * 24 + 6890 * 32) // 128) and rows[3][0] <= 65535
    for r in rows:
        assert all(x % 16 == 0 for x in r[1:7])


# ---- Python-side refusals (no handle is needed to reach them) ----
def _bare_model(V=rc.HAND_V, n_faces=2):
    m = capi.Model.__new__(capi.Model)
    m.V, m.K, m.NP, m.handle, m.n_faces = V, 2, 6, None, n_faces
    return m


def test_python_side_refusals():
    m = _bare_model()
    cam = rc.capi_camera(rc.HAND_CAM)
    v = np.zeros((2, rc.HAND_V, 3), dtype=np.float32)
    with pytest.raises(ValueError, match='no faces'):
        _bare_model(n_faces=0).render(v, cam, (8, 8))
    with pytest.raises(ValueError, match='float32 or float64'):
        m.render(v.astype(np.float16), cam, (8, 8))
    with pytest.raises(ValueError, match=r'verts must be \[F, 16, 3\]'):
        m.render(v[:, :5], cam, (8, 8))
    with pytest.raises(ValueError, match='1 .. 4096'):
        m.render(v, cam, (0, 8))
    with pytest.raises(ValueError, match='1 .. 4096'):
        m.render(v, cam, (8, 5000))
    with pytest.raises(ValueError, match='size must be'):
        m.render(v, cam, 8)
    with pytest.raises(ValueError, match='one camera or one per frame'):
        m.render(v, [cam, cam, cam], (8, 8))
    with pytest.raises(ValueError, match='capi.Camera'):
        m.render(v, [rc.HAND_CAM], (8, 8))
    with pytest.raises(ValueError, match='ambient'):
        m.render(v, cam, (8, 8), ambient=1.5)
    with pytest.raises(ValueError, match='point_rgb and point_radius'):
        m.render(v, cam, (8, 8), points=np.zeros((2, 3, 3)))
    with pytest.raises(ValueError, match='points must be'):
        m.render(v, cam, (8, 8), points=np.zeros((5, 3, 3)), point_rgb=(1, 2, 3), point_radius=0.01)
    with pytest.raises(ValueError, match='outputs'):
        m.render(v, cam, (8, 8), outputs=('rgb', 'alpha'))
    with pytest.raises(ValueError, match='outputs'):
        m.render(v, cam, (8, 8), outputs=())
    with pytest.raises(ValueError, match='pose / trans'):
        m.render_posed(np.zeros((2, 5)), np.zeros((2, 3)), cam, (8, 8))
    with pytest.raises(ValueError, match='dtype'):
        m.render_posed(np.zeros((2, 6)), np.zeros((2, 3)), cam, (8, 8), dtype=np.float16)
    with pytest.raises(ValueError, match='no free shape block'):
        m.render_posed(np.zeros((2, 6)), np.zeros((2, 3)), cam, (8, 8), shape=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='no free shape block'):
        m.render_posed_device(2, 1, 2, cam, (8, 8), shape_ptr=3)


def test_solver_and_mosh_head_refusals(tmp_path):
    from moshpp_amd import chmosh, mosh_head
    s = chmosh.StageIISolver.__new__(chmosh.StageIISolver)
    s.n_shape, s.dev = 0, None
    with pytest.raises(KeyError, match=r"StageIISolver.render: the result has no 'trans'"):
        s.render(dict(pose=np.zeros((3, 72))))
    s.sm = type('SM', (), {'f': None})()
    with pytest.raises(ValueError, match='no faces'):
        s.render(dict(pose=np.zeros((3, 72)), trans=np.zeros((3, 3))))
    s.sm = type('SM', (), {'f': np.zeros((1, 3), dtype=int)})()
    out = dict(pose=np.zeros((3, 72)), trans=np.zeros((3, 3)))
    with pytest.raises(ValueError, match='observations are'):
        s.render(out, obs=np.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match='label order'):
        s.render(dict(out, markers_obs=[[]] * 3, labels_obs=[[]] * 3))
    with pytest.raises(IndexError, match='frame_ids'):
        s.render(out, frame_ids=[5])
    with pytest.raises(ValueError, match='marker_radius'):
        s.render(out, marker_radius=0.0)
    cfg = {'surface_model': {'type': 'mano', 'num_betas': 10, 'fname': None}, 'moshpp': {}}
    data = {'fullpose': np.zeros((3, 48)), 'trans': np.zeros((3, 3)), 'betas': np.zeros(10), 'stageii_debug_details': {'cfg': cfg}}
    with pytest.raises(KeyError, match="'trans'"):
        mosh_head.stageii_preview({k: v for k, v in data.items() if k != 'trans'})
    with pytest.raises(ValueError, match='1 .. 4096'):
        mosh_head.stageii_preview(data, size=(0, 10))
    with pytest.raises(ValueError, match='contact_sheet_columns'):
        mosh_head.stageii_preview(data, contact_sheet_columns=0)
    with pytest.raises(ValueError, match='no frame'):
        mosh_head.stageii_preview(data, frame_ids=np.zeros(0, dtype=int))
    with pytest.raises(ValueError, match='twice'):
        mosh_head.stageii_preview(data, out_dir=str(tmp_path), frame_ids=[1, 1])
    (tmp_path / 'frame_000002.png').write_bytes(b'x')
    with pytest.raises(FileExistsError, match='frame_000002.png'):
        mosh_head.stageii_preview(data, out_dir=str(tmp_path))
    assert (tmp_path / 'frame_000002.png').read_bytes() == b'x'


# ---- the reference's self-checks ----
def _hand_reference(name):
    s = rc.hand_scenes()[name]
    W, H = rc.HAND_SIZE
    return s, rc.reference(s['verts'], rc.numpy_normals(s['verts'], s['faces']), s['faces'], [rc.HAND_CAM], W, H, s['points'], s['radius'], s['prgb'])


@pytest.mark.parametrize('name', sorted(rc.hand_scenes()))
def test_input_conditions_hold_on_the_hand_made_scenes(name):
    s, ref = _hand_reference(name)
    for dtype in (np.float64, np.float32):
        v = rc.as_input(s['verts'], dtype)
        p = rc.as_input(s['points'], dtype)
        W, H = rc.HAND_SIZE
        rc.check_conditions(rc.reference(v, rc.numpy_normals(v, s['faces']), s['faces'], [rc.HAND_CAM], W, H, p, s['radius'], s['prgb']), v,
                            [rc.HAND_CAM], f'{name} {np.dtype(dtype).name}')


@pytest.mark.parametrize('model_type', sorted(rc.BODIES))
def test_input_conditions_hold_on_the_body_scenes(model_type):
    b = rc.body_scene(model_type)
    W, H = rc.BODY_SIZE
    for dtype in (np.float64, np.float32):
        v, p = rc.as_input(b['verts'], dtype), rc.as_input(b['points'], dtype)
        nrm = rc.numpy_normals(v, b['faces'])
        for cname, cams in b['cameras'].items():
            ref = rc.reference(v, nrm, b['faces'], cams, W, H, p, b['radius'], b['prgb'])
            rc.check_conditions(ref, v, cams, f'{model_type} {cname} {np.dtype(dtype).name}')
            covered = ref['ids'] >= 0
            assert covered.any() and (cname in ('close', 'far') or (ref['ids'] >= len(b['faces'])).any())   # a body and, at a fitting distance, markers are in the picture
            if cname == 'far':        # the whole body inside the tile [32, 64) x [32, 64), more faces than one list chunk of 1024
                _, jj, ii = np.nonzero(covered)
                assert ii.min() >= 32 and ii.max() < 64 and jj.min() >= 32 and jj.max() < 64 and len(b['faces']) > 1024
            if cname == 'close':      # vertices behind znear, and triangles that span tiles
                assert any((~rc.project_vertices(cams[0], v[f])[0]).any() for f in range(len(v)))
                f_, jj, ii = np.nonzero(covered)
                tiles = {}
                for fid, tile in zip(ref['ids'][covered], (f_ * 100 + (jj // 32) * 10 + ii // 32)):
                    tiles.setdefault(int(fid), set()).add(int(tile))
                spanning = sum(len(t) > 1 for t in tiles.values())
                print(f'{spanning} of {len(tiles)} visible faces lie in more than one tile')
                assert spanning >= 10


def test_quad_has_its_exact_pixel_count_and_every_pixel_once():
    for name in ('quad', 'quad_one_winding_reversed'):
        s, ref = _hand_reference(name)
        ids = ref['ids'][0]
        assert (ids >= 0).sum() == rc.QUAD_PIXELS
        jj, ii = np.nonzero(ids >= 0)
        assert (ii.min(), ii.max(), jj.min(), jj.max()) == (4, 19, 3, 14)          # left and top edges in, right and bottom out
        assert not np.isfinite(ref['z2'][0]).any()                                  # no pixel has a second candidate: covered once
        np.testing.assert_array_equal(ref['depth'][0][ids >= 0], np.float32(2.0))
        assert set(np.unique(ids)) == {-1, 0, 1}
        on_diag = [(3 + 3 * k, 4 + 4 * k) for k in range(4)]                        # centres on the shared edge
        assert len({int(ids[j, i]) for j, i in on_diag}) == 1 and ids[on_diag[0]] >= 0


def test_top_left_rule_union_of_two_triangles_is_the_quad():
    s = rc.hand_scenes()['quad']
    W, H = rc.HAND_SIZE
    nrm = rc.numpy_normals(s['verts'], s['faces'])
    both = rc.reference(s['verts'], nrm, s['faces'], [rc.HAND_CAM], W, H)['ids'][0] >= 0
    parts = [rc.reference(s['verts'], nrm, s['faces'][k:k + 1], [rc.HAND_CAM], W, H)['ids'][0] >= 0 for k in range(2)]
    assert not (parts[0] & parts[1]).any()
    np.testing.assert_array_equal(parts[0] | parts[1], both)
    assert both.sum() == rc.QUAD_PIXELS
    # the same holds for a random fan of triangles around a vertex that lies on a pixel centre
    rng = np.random.default_rng(4)
    ang = np.sort(rng.uniform(0, 2 * np.pi, 7))
    ring = [rc._at(20.5 + 14 * np.cos(a), 18.5 + 13 * np.sin(a)) for a in ang]
    verts = rc._pad([rc._at(20.5, 18.5)] + ring)
    faces = np.array([[0, 1 + k, 1 + (k + 1) % 7] for k in range(7)], dtype=np.int32)
    nrm = rc.numpy_normals(verts, faces)
    ref = rc.reference(verts, nrm, faces, [rc.HAND_CAM], W, H)
    assert not np.isfinite(ref['z2']).any() and ref['ids'][0, 18, 20] >= 0
    union = np.zeros((H, W), dtype=int)
    for k in range(7):
        union += rc.reference(verts, nrm, faces[k:k + 1], [rc.HAND_CAM], W, H)['ids'][0] >= 0
    assert union.max() == 1 and ((union == 1) == (ref['ids'][0] >= 0)).all()


def test_reference_scene_content():
    """The hand-made scenes show what they were made to show (in the reference)."""
    _, ref = _hand_reference('behind_znear')
    assert set(np.unique(ref['ids'])) == {-1, 0}                                    # the faces that name the vertex behind znear are gone
    _, ref = _hand_reference('degenerate')
    assert set(np.unique(ref['ids'])) == {-1, 2}
    _, ref = _hand_reference('outside')
    assert set(np.unique(ref['ids'])) == {-1, 0, 1}
    _, ref = _hand_reference('interpenetrating')
    assert set(np.unique(ref['ids'])) == {-1, 0, 1} and np.isfinite(ref['z2']).any()
    s, ref = _hand_reference('markers')
    ids = ref['ids'][0]
    assert set(np.unique(ids)) == {-1, 0, 1, 2, 3, 4}                               # markers 0 .. 3 carry 1 + k; NaN, r = 0, behind znear: absent
    assert (ids[:, 0] == 4).any()                                                   # the one partly outside reaches the border
    # the marker in front hides the triangle, the one behind shows only outside it
    assert ids[10, 12] == 1 and ids[24, 9] == 0 and ids[24, 5] == 2
    half = ref['depth'][0][ids == 3]
    np.testing.assert_array_equal(half, np.float32(2.0 - 0.06))
