"""Shared by the preview-rendering tests (tests/test_render_host_logic.py, test_render_emulation.py, test_gpu_render.py): a NumPy f64
reference of the rendering rules of include/moshii.h, the scenes and the checker.

The reference is a plain loop over faces, vectorised over the pixels of a face's bounding box.  Per pixel it keeps the best and the
second-best candidate under the order (f32 depth, id): id, depth, colour, and z2 / id2 (+inf / -1 when there is one candidate).

The checker holds a result to it like this
  * coverage is integer arithmetic on both sides, so OUTSIDE THE DEPTH GUARD BAND -- covered pixels with (z2 - z1) / z1 < 1e-6 in the
    reference -- the ids are equal at every pixel, the depth agrees within one f32 ulp and every colour channel within one level: both
    are the tie of ONE final rounding (the f64 values in front of it differ by a few 1e-16 relative between kernel and NumPy, by FMA
    contraction and the order of a three-term sum), nothing more;
  * inside the guard band the id is one of the reference's two nearest candidates.

Conditions on the inputs (asserted in the CPU tier on the reference alone for every scene here, and again on what a test passes in)
  * no projected vertex coordinate lies within 1e-9 of a snapping boundary in 1/16-pixel units, where kernel and reference could
    legitimately snap apart;
  * the guard band holds at most 1 % of the covered pixels.
Change the seed, not the cap.
"""
import functools

import numpy as np

from tests import normals_common as nc

GUARD = 1e-6
GUARD_SHARE = 0.01
SNAP_MARGIN = 1e-9
SNAP_MAX = 2.0 ** 24
BODY, BG, AMBIENT = (200, 170, 150), (250, 250, 245), 0.3


def camera(R=None, t=(0.0, 0.0, 0.0), fx=64.0, fy=64.0, cx=0.0, cy=0.0, znear=0.5):
    return dict(R=np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3), t=np.asarray(t, dtype=np.float64),
                fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), znear=float(znear))


def capi_camera(c):
    from moshpp_amd import capi
    return capi.Camera.make(c['R'], c['t'], c['fx'], c['fy'], c['cx'], c['cy'], c['znear'])


def _to_camera(c, p):
    """X_c = R X + t, each row summed left to right (the header's order)."""
    R, t = c['R'], c['t']
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([R[i, 0] * x + R[i, 1] * y + R[i, 2] * z + t[i] for i in range(3)], axis=-1)


def project_vertices(c, verts):
    """(ok[V], sx[V], sy[V] int64, z[V], fractional distance to the nearest snapping boundary [V, 2] (inf where not ok))."""
    with np.errstate(all='ignore'):
        xc = _to_camera(c, np.asarray(verts, dtype=np.float64))
        ok = np.isfinite(xc).all(-1) & (xc[..., 2] > c['znear'])
        zs = np.where(ok, xc[..., 2], 1.0)
        g = np.stack([16.0 * (c['fx'] * xc[..., 0] / zs + c['cx']) + 0.5, 16.0 * (c['fy'] * xc[..., 1] / zs + c['cy']) + 0.5], axis=-1)
        s = np.floor(g)
        ok &= np.isfinite(s).all(-1) & (np.abs(s) <= SNAP_MAX).all(-1)
        s = np.where(ok[..., None], s, 0.0)
        margin = np.where(ok[..., None], np.minimum(g - np.floor(g), np.ceil(g) - g), np.inf)
        # a value that IS an integer sits on the boundary
        margin = np.where(ok[..., None] & (g == np.floor(g)), 0.0, margin)
    return ok, s[..., 0].astype(np.int64), s[..., 1].astype(np.int64), xc[..., 2], margin


def _offer(state, sel, jj, ii, zf, cid, inten, rgbsrc):
    """Candidates (zf, cid) at the pixels (jj, ii)[sel] enter the per-pixel best / second-best lists."""
    z1, id1, z2, id2, I, src = state
    jj, ii, zf, inten = jj[sel], ii[sel], zf[sel], inten[sel]
    b1, bid1 = z1[jj, ii], id1[jj, ii]
    wins = (zf < b1) | ((zf == b1) & (cid < bid1))
    # the loser of (candidate, best) competes for second place
    lz = np.where(wins, b1, zf)
    lid = np.where(wins, bid1, cid)
    b2, bid2 = z2[jj, ii], id2[jj, ii]
    second = (lid >= 0) & ((lz < b2) | ((lz == b2) & ((lid < bid2) | (bid2 < 0))))
    z2[jj, ii] = np.where(second, lz, b2)
    id2[jj, ii] = np.where(second, lid, bid2)
    z1[jj, ii] = np.where(wins, zf, b1)
    id1[jj, ii] = np.where(wins, cid, bid1)
    I[jj, ii] = np.where(wins, inten, I[jj, ii])
    src[jj, ii] = np.where(wins, rgbsrc, src[jj, ii])


def reference_frame(verts, normals, faces, c, W, H, points=None, radius=None, prgb=None, body=BODY, bg=BG, ambient=AMBIENT):
    """One frame by the rules: dict(ids[H, W] int32, depth[H, W] f32, rgb[H, W, 3] u8, z2[H, W] f32, id2[H, W])."""
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces)
    NF = len(faces)
    ok, sx, sy, zc, _ = project_vertices(c, verts)
    ncam = np.stack([c['R'][i, 0] * normals[:, 0].astype(np.float64) + c['R'][i, 1] * normals[:, 1].astype(np.float64)
                     + c['R'][i, 2] * normals[:, 2].astype(np.float64) for i in range(3)], axis=-1).astype(np.float32).astype(np.float64)
    z1 = np.full((H, W), np.inf, dtype=np.float32); id1 = np.full((H, W), -1, dtype=np.int64)
    z2 = np.full((H, W), np.inf, dtype=np.float32); id2 = np.full((H, W), -1, dtype=np.int64)
    inten = np.full((H, W), float(ambient)); src = np.full((H, W), -1, dtype=np.int64)    # colour source: -1 body, k marker k
    state = (z1, id1, z2, id2, inten, src)
    for f in range(NF):
        a, b, cc = (int(x) for x in faces[f])
        if a == b or b == cc or a == cc or not (ok[a] and ok[b] and ok[cc]):
            continue
        tri = [a, b, cc]
        area2 = int((sx[b] - sx[a]) * (sy[cc] - sy[a]) - (sy[b] - sy[a]) * (sx[cc] - sx[a]))
        if area2 == 0:
            continue
        if area2 < 0:
            tri = [a, cc, b]
            area2 = -area2
        xs, ys = sx[tri], sy[tri]
        i0, i1 = max(0, -((-(int(xs.min()) - 8)) // 16)), min(W - 1, (int(xs.max()) - 8) // 16)
        j0, j1 = max(0, -((-(int(ys.min()) - 8)) // 16)), min(H - 1, (int(ys.max()) - 8) // 16)
        if i0 > i1 or j0 > j1:
            continue
        jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing='ij')
        px, py = 16 * ii.astype(np.int64) + 8, 16 * jj.astype(np.int64) + 8
        E, inside = [], np.ones(ii.shape, dtype=bool)
        for k in range(3):                        # the edge opposite corner k
            xa, ya, xb, yb = int(xs[(k + 1) % 3]), int(ys[(k + 1) % 3]), int(xs[(k + 2) % 3]), int(ys[(k + 2) % 3])
            dx, dy = xb - xa, yb - ya
            e = dx * (py - ya) - dy * (px - xa)
            top_left = dy < 0 or (dy == 0 and dx > 0)
            inside &= (e > 0) | ((e == 0) & top_left)
            E.append(e)
        if not inside.any():
            continue
        w = [E[k].astype(np.float64) / float(area2) for k in range(3)]
        zk = zc[tri]
        z = 1.0 / (w[0] / zk[0] + w[1] / zk[1] + w[2] / zk[2])
        n = sum((w[k] / zk[k])[..., None] * ncam[tri[k]] for k in range(3))
        l2 = (n * n).sum(-1)
        with np.errstate(all='ignore'):
            lit = np.where((l2 > 0) & np.isfinite(l2), ambient + (1.0 - ambient) * np.maximum(0.0, -(n[..., 2] / np.sqrt(l2))), ambient)
        _offer(state, inside, jj, ii, z.astype(np.float32), f, lit, -1)
    if points is not None:
        points = np.asarray(points, dtype=np.float64)
        with np.errstate(all='ignore'):
            pc = _to_camera(c, points)
        for k in range(len(points)):
            r = float(radius[k])
            x, y, zk = pc[k]
            if not np.isfinite(pc[k]).all() or not r > 0.0 or not zk - r > c['znear']:
                continue
            uc, vc = c['fx'] * x / zk + c['cx'], c['fy'] * y / zk + c['cy']
            rx, ry = c['fx'] * r / zk, c['fy'] * r / zk
            if not (np.isfinite([uc, vc, rx, ry]).all() and rx > 0 and ry > 0):
                continue
            i0, i1 = max(0, int(np.floor(uc - rx)) - 1), min(W - 1, int(np.ceil(uc + rx)) + 1)
            j0, j1 = max(0, int(np.floor(vc - ry)) - 1), min(H - 1, int(np.ceil(vc + ry)) + 1)
            if i0 > i1 or j0 > j1:
                continue
            jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing='ij')
            tx, ty = (ii + 0.5 - uc) / rx, (jj + 0.5 - vc) / ry
            d2 = tx * tx + ty * ty
            cov = d2 <= 1.0
            if not cov.any():
                continue
            lit = ambient + (1.0 - ambient) * np.sqrt(np.maximum(0.0, 1.0 - d2))
            _offer(state, cov, jj, ii, np.full(ii.shape, np.float32(zk - r), dtype=np.float32), NF + k, lit, k)
    col = np.empty((H, W, 3), dtype=np.float64)
    col[:] = np.asarray(body, dtype=np.float64)
    if points is not None and len(points):
        m = src >= 0
        col[m] = np.asarray(prgb, dtype=np.float64)[src[m]]
    rgb = np.floor(255.0 * (col / 255.0) * inten[..., None] + 0.5).astype(np.uint8)
    rgb[id1 < 0] = np.asarray(bg, dtype=np.uint8)
    return dict(ids=id1.astype(np.int32), depth=z1, rgb=rgb, z2=z2, id2=id2.astype(np.int32))


def reference(verts, normals, faces, cams, W, H, points=None, radius=None, prgb=None, **kw):
    """All frames: the dict of reference_frame with a leading frame axis.  cams: one camera or one a frame."""
    F = len(verts)
    fr = [reference_frame(verts[f], normals[f], faces, cams[f if len(cams) > 1 else 0], W, H, None if points is None else points[f],
                          radius, prgb, **kw) for f in range(F)]
    return {k: np.stack([r[k] for r in fr]) for k in fr[0]}


def guard_band(ref):
    """(covered, in the guard band) pixel masks of a reference result."""
    covered = ref['ids'] >= 0
    z1, z2 = ref['depth'].astype(np.float64), ref['z2'].astype(np.float64)
    with np.errstate(all='ignore'):
        band = covered & np.isfinite(z2) & ((z2 - z1) / z1 < GUARD)
    return covered, band


def snap_margin(verts, cams):
    """The smallest distance of a projected coordinate to a snapping boundary over all frames (1/16-pixel units)."""
    verts = np.asarray(verts, dtype=np.float64)
    return min(project_vertices(cams[f if len(cams) > 1 else 0], verts[f])[4].min() for f in range(len(verts)))


def check_conditions(ref, verts, cams, name=''):
    covered, band = guard_band(ref)
    share = band.sum() / max(int(covered.sum()), 1)
    margin = snap_margin(verts, cams)
    print(f'{name}: {int(covered.sum())} covered pixels, {int(band.sum())} in the guard band ({100 * share:.3f} %), snapping margin {margin:.3e}')
    assert margin >= SNAP_MARGIN, (name, margin)
    assert share <= GUARD_SHARE, (name, share)


def check(got, ref, name=''):
    """A rendering result (dict of rgb / ids / depth, any subset) against the reference; returns the figures it printed."""
    covered, band = guard_band(ref)
    free = ~band
    out = {}
    if 'ids' in got:
        bad = (got['ids'] != ref['ids']) & free
        inband = band & (got['ids'] != ref['ids']) & (got['ids'] != ref['id2'])
        out['ids_wrong'] = int(bad.sum()); out['band_wrong'] = int(inband.sum())
    if 'depth' in got:
        g, r = got['depth'], ref['depth']
        assert g.dtype == np.float32
        fin = np.isfinite(r) & free
        with np.errstate(all='ignore'):
            ulps = np.abs(g[fin].astype(np.float64) - r[fin].astype(np.float64)) / np.spacing(np.abs(r[fin])).astype(np.float64)
        out['depth_ulps'] = float(ulps.max()) if ulps.size else 0.0
        out['depth_inf_wrong'] = int(((g != r) & ~np.isfinite(r) & free).sum())
    if 'rgb' in got:
        d = np.abs(got['rgb'].astype(np.int32) - ref['rgb'].astype(np.int32)).max(-1)
        out['rgb_levels'] = int(d[free].max()) if free.any() else 0
    print(f'{name}: {out} ({int(covered.sum())} covered, {int(band.sum())} in the guard band)')
    assert out.get('ids_wrong', 0) == 0 and out.get('band_wrong', 0) == 0, (name, out)
    assert out.get('depth_ulps', 0.0) <= 1.0 and out.get('depth_inf_wrong', 0) == 0, (name, out)
    assert out.get('rgb_levels', 0) <= 1, (name, out)
    return out


# ---- hand-made scenes (V = 16; the meshes go to render() as given, the model only lends its vertex count) ------------------------
HAND_V = 16
HAND_SIZE = (40, 36)                      # two tiles each way, neither a whole number of them
HAND_CAM = camera()                       # identity, fx = fy = 64, znear 0.5: at z = 2 a pixel is 1 / 32 m, exact in f32 and f64


def hand_model():
    """Model arrays of a two-joint body with HAND_V vertices (capi.Model(**...)); the scenes bring their own vertices."""
    rng = np.random.default_rng(2)
    V = HAND_V
    w = rng.random((V, 2)); w /= w.sum(1, keepdims=True)
    jr = np.zeros((2, V)); jr[0, :4] = 0.25; jr[1, 4:8] = 0.25
    return dict(v_template=rng.normal(0, 0.3, (V, 3)), shapedirs=np.zeros((V, 3, 1)), posedirs=np.zeros((V, 3, 9)), weights=w, J_regressor=jr,
                parents=np.array([-1, 0]), body_dof=6, hand_dof=0, hands_mean=None, selected_components=None)


def _at(u, v, z=2.0):
    """The world point that HAND_CAM sees at pixel position (u, v) and depth z."""
    return [u * z / 64.0, v * z / 64.0, z]


def _pad(rows):
    v = np.full((HAND_V, 3), 5.0)          # unused vertices: somewhere in front of the camera, named by no face
    v[:len(rows)] = rows
    return v[None]


QUAD_PIXELS = 16 * 12                      # centres in [4.5, 20.5) x [3.5, 15.5)


@functools.lru_cache(maxsize=None)
def hand_scenes():
    """name -> dict(verts[1, 16, 3] f64, faces, points[1, N, 3] | None, radius, prgb).  Shared, never modified."""
    q = [_at(4.5, 3.5), _at(20.5, 3.5), _at(20.5, 15.5), _at(4.5, 15.5)]
    sc = {}
    # the diagonal (4.5, 3.5) - (20.5, 15.5) passes through the centres (4.5 + 4 k, 3.5 + 3 k); the outer edges lie on rows / columns of centres
    sc['quad'] = dict(verts=_pad(q), faces=[[0, 1, 2], [0, 2, 3]])
    sc['quad_one_winding_reversed'] = dict(verts=_pad(q), faces=[[0, 1, 2], [0, 3, 2]])
    sc['interpenetrating'] = dict(verts=_pad([_at(3.3, 4.2, 1.5), _at(33.7, 6.1, 3.0), _at(12.4, 30.2, 2.2),
                                              _at(35.1, 3.3, 1.5), _at(5.2, 8.4, 3.0), _at(25.6, 31.3, 2.2)]), faces=[[0, 1, 2], [3, 4, 5]])
    sc['behind_znear'] = dict(verts=_pad([_at(5.2, 5.3), _at(30.1, 8.2), _at(12.3, 28.4), [0.01, 0.02, 0.4], _at(2.2, 20.3), _at(8.1, 33.2)]),
                              faces=[[0, 1, 2], [3, 4, 5], [0, 3, 1]])
    sc['degenerate'] = dict(verts=_pad([_at(2.5, 2.5), _at(6.5, 6.5), _at(10.5, 10.5), _at(20.3, 4.1), _at(34.2, 9.3), _at(22.4, 25.2)]),
                            faces=[[0, 1, 2], [3, 3, 4], [3, 4, 5], [5, 4, 5]])
    sc['outside'] = dict(verts=_pad([_at(-20.3, -10.2), _at(25.2, 5.1), _at(-5.4, 30.3),            # partly outside, left and top
                                     _at(30.2, 20.1), _at(70.3, 25.2), _at(35.4, 60.1),               # partly outside, right and bottom
                                     _at(100.2, 100.1), _at(140.3, 100.2), _at(120.1, 150.3),         # wholly outside
                                     [1.0e7, 0.0, 2.0], _at(10.2, 10.1), _at(12.3, 20.2),             # a snapped coordinate beyond 2^24
                                     [np.nan, 0.0, 2.0]]), faces=[[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 10, 11]])
    tri = [_at(4.2, 4.3), _at(36.1, 6.2), _at(10.3, 33.1)]
    pts = [_at(12.3, 10.2, 1.5),           # in front of the triangle
           _at(6.1, 24.2, 3.0),            # behind it, showing where it passes the triangle's edge
           _at(22.2, 12.4, 2.0),           # half inside: its centre lies in the triangle's plane
           _at(1.2, 34.9, 1.8),            # partly outside the image
           [np.nan, 0.1, 2.0],             # absent
           _at(30.1, 30.2, 1.7),           # no radius
           _at(20.0, 20.0, 0.55)]          # z - r behind znear
    sc['markers'] = dict(verts=_pad(tri), faces=[[0, 1, 2]], points=np.array(pts)[None],
                         radius=np.array([0.05, 0.2, 0.06, 0.08, 0.05, 0.0, 0.1]),
                         prgb=np.array([[215, 48, 39], [44, 101, 201], [20, 160, 60], [240, 200, 30], [0, 0, 0], [9, 9, 9], [90, 90, 90]], dtype=np.uint8))
    for s in sc.values():
        s['faces'] = np.asarray(s['faces'], dtype=np.int32)
        s.setdefault('points', None); s.setdefault('radius', None); s.setdefault('prgb', None)
        s['verts'].setflags(write=False)
    return sc


def numpy_normals(verts, faces):
    """Vertex normals in NumPy (the CPU tier's stand-in for the normals kernel), faces that name a vertex twice left out."""
    faces = np.asarray(faces)
    good = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    with np.errstate(all='ignore'):
        return np.nan_to_num(nc.ref_normals(np.asarray(verts, dtype=np.float64), faces[good]), nan=0.0)


# ---- body scenes -------------------------------------------------------------------------------------------------------------
BODY_SIZE = (96, 80)                       # 3 x 3 tiles, partial on both axes
BODY_F = 3
BODIES = {'smplh': 600, 'mano': 300}
BODY_SEED = {'smplh': 5, 'mano': 5}


def _moved(c, dz, znear=None, cx=None, cy=None):
    """Camera c moved by dz along its own viewing direction (negative: back)."""
    t = c['t'].copy(); t[2] -= dz
    return dict(c, t=t, znear=c['znear'] if znear is None else znear, cx=c['cx'] if cx is None else cx, cy=c['cy'] if cy is None else cy)


@functools.lru_cache(maxsize=None)
def body_scene(model_type):
    """dict(case, pose, trans, verts[3, V, 3] (the oracle's, f64), faces, points, radius, prgb, cameras: name -> list of cameras).
    Shared, never modified."""
    from moshpp_amd import preview
    case = nc.mesh_case(model_type, BODIES[model_type])
    rng = np.random.default_rng(BODY_SEED[model_type])
    pose, trans = rng.normal(0, 0.35, (BODY_F, case['m']['NP'])), rng.normal(0, 0.05, (BODY_F, 3))
    verts = nc.oracle_verts(case['m'], pose, trans)
    faces = case['faces']
    W, H = BODY_SIZE
    fit = preview.preview_camera(verts, BODY_SIZE, view=(25.0, 10.0)).as_dict()
    dist = float(_to_camera(fit, verts.reshape(-1, 3))[:, 2].mean())
    cams = {'fitted': [fit],
            # 3.2 times as far: the body is under a third of the image and lies inside the tile [32, 64) x [32, 64)
            'far': [_moved(fit, -2.2 * dist, cx=48.0, cy=48.0)],
            # the eye inside the body's bounding box: huge triangles, vertices behind znear, snapped coordinates beyond 2^24
            'close': [_moved(fit, dist - 0.06, znear=0.02)],
            'per_frame': [preview.preview_camera(verts, BODY_SIZE, view=(az, el)).as_dict() for az, el in ((0.0, 0.0), (40.0, 20.0), (-75.0, -10.0))]}
    nrm = numpy_normals(verts, faces)
    vids = rng.choice(verts.shape[1], 8, replace=False)
    extent = float(np.ptp(verts.reshape(-1, 3), axis=0).max())
    r = 0.012 * extent
    points = verts[:, vids] + r * nrm[:, vids]
    points[1, 2] = np.nan
    radius = np.full(8, r); radius[5] = 0.5 * r
    prgb = np.array([[215, 48, 39]] * 4 + [[44, 101, 201]] * 4, dtype=np.uint8)
    for a in (verts, points):
        a.setflags(write=False)
    return dict(case=case, pose=pose, trans=trans, verts=verts, faces=faces, points=points, radius=radius, prgb=prgb, cameras=cams)


def as_input(a, dtype):
    """What a test passes to the library for the reference array `a`: the same values in `dtype` (f32: rounded once, and the reference
    then works on the rounded values)."""
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def render_and_check(dev, verts, faces, cams, size, points, radius, prgb, dtype, name, outputs=('rgb', 'ids', 'depth')):
    """render() on a live handle against the reference on the very same inputs and the normals kernel's own normals."""
    v, p = as_input(verts, dtype), as_input(points, dtype)
    got = dev.render(v, [capi_camera(c) for c in cams], size, points=p, point_rgb=prgb, point_radius=radius, body_rgb=BODY, bg_rgb=BG,
                     ambient=AMBIENT, outputs=outputs)
    ref = reference(v, dev.vertex_normals(v), faces, cams, size[0], size[1], p, radius, prgb)
    check_conditions(ref, v, cams, name)
    check(got, ref, name)
    return got, ref
