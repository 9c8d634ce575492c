"""Shared by the signed point-to-mesh distance tests (tests/test_surface_distance_emulation.py, tests/test_gpu_surface_distance.py):
points that reach every branch of the nearest-point query, the checker against oracle.stagei_oracle.signed_surface_distance evaluated
in f64 ON THE VERY vertices and points the device saw (f32 values converted exactly), and the derived bounds.  Bodies:
normals_common.mesh_case.

Bounds
  F64_TOL = 1e-12 m   the f64 entries: the oracle's formula in the same precision, only the order of operations differs.
  B32 = C32 * 2^-24 * R for the f32 entries, R = the largest |coordinate - first vertex| over the frame's vertices and finite points
        (every difference the kernel forms is at most 2R per coordinate, D <= 2 sqrt(3) R in length), u = 2^-24.  From the kernel's
        operations (lbs_forward.hip, sd_search / sd_closest / k_sd_finish):
          * the search forms ab, ac, ap by one subtraction each (relative error u, whatever the frame's position), the coefficients
            (s, t) of the closest point q = a + s ab + t ac, the residual p - q = ap - s ab - t ac by two fmas per coordinate and d^2 by
            a three-term fma dot.  With (s, t) held fixed the residual's error is at most u (|ap| + 2 |s ab| + 2 |t ac|) <= 5 u D in
            length, the dot and what sqrt would undo add 2 u D: E1 <= 7 u D <= 7 * 2 sqrt(3) u R = 24.3 u R per (point, triangle).
          * (s, t) and the region are solved for the point's foot on the triangle's plane, ap - h n with n = ab x ac and
            h = ap.n / n.n.  The foot carries an error e <= 3 u D + d u k / 2 (three roundings of values <= D = d + L, and the height
            d times the tilt u k / 2 of a cross product with cancellation; d the distance, L the triangle's longest edge,
            k = L^2 / area).  Above the interior the search takes d^2 = h^2 n.n, the height alone: the tilt acts on the foot's in-plane
            offset <= L, E3 <= u k L / 2 -- a property of the mesh, T = max over faces of k L / 2 <= C3 R, C3 = 16 (asserted;
            posed bodies fold needles of up to T = 13 m into the elbows and armpits of these meshes).
          * the region tests multiply dot products with errors L (e + 6 u D_p), D_p <= 2 L the foot's in-plane offset from a nearest
            triangle: the line between two regions is displaced in the plane by b <= k (D_p / L) (e + 6 u D_p)
            <= k u ((6 + k) d + 30 L), and so is q along an edge.  Such a displacement is at right angles to p - q at the true
            closest point: it changes the distance only at second order, E2 <= min(b, b^2 / 2d).  Only the NEAREST triangle's E2
            counts: an over-estimate of any other triangle cannot make it win.  E2 depends on the mesh, so the builder below evaluates
            it for every point from the oracle's nearest triangle and does not use a seed where it passes C2 u R, C2 = 48.
          * the search's winner can therefore be a triangle whose true distance exceeds the minimum by at most 2 (E1 + E3) + E2; the
            f64 re-evaluation of that triangle from the f32 inputs is exact to ~1e-16, and the store rounds once:
            u |d| <= 2 sqrt(3) u R.
        C32 = 2 * (24.3 + 16) + 48 + 3.5 = 132.1 -> 132: B32 = 132 * 2^-24 * R = 7.9e-6 R, 1.6e-5 m at R = 2 m, below F32_TOL = 2e-5 m,
        the export's own per-coordinate bound (asserted for every frame).
"""
import numpy as np

from oracle import stagei_oracle as s1
from tests.lbs_shape_common import F32_TOL, F64_TOL   # noqa: F401

U32 = 2.0 ** -24
C32 = 132.0
C2 = 48.0
C3 = 16.0
SIGN_COS = 1e-3          # the sign is compared where the oracle's |cos(p - nearest, n)| is at least this ...
SIGN_CAP = 0.02          # ... and at most this share of a case's finite points may fall outside that condition
KINDS = ('out 9.5 mm', 'in 5 mm', 'centroid +3 mm', 'centroid -3 mm', 'edge midpoint', 'vertex', 'beyond an edge', 'beyond a vertex',
         'far', 'absent')


def frame_radius(verts, points):
    """R per frame [F]: the largest |coordinate - first vertex| over vertices and finite points."""
    v = np.asarray(verts, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64)
    c = v[:, :1]
    with np.errstate(invalid='ignore'):
        rp = np.where(np.isfinite(p), np.abs(p - c), 0.0).reshape(len(v), -1).max(axis=1) if p.shape[1] else np.zeros(len(v))
    return np.maximum(np.abs(v - c).reshape(len(v), -1).max(axis=1), rp)


def bound_for(dtype, verts, points):
    """The distance bound per frame [F] for entries of `dtype` on these inputs."""
    if np.dtype(dtype) == np.float64:
        return np.full(len(verts), F64_TOL)
    b = C32 * U32 * frame_radius(verts, points)
    assert (b <= F32_TOL).all(), b.max()
    return b


def _good_faces(faces):
    return (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])


def _build_points(verts, faces, N, seed, require_all):
    """points[F, N, 3] f64 on the meshes verts[F, V, 3]: the ten KINDS dealt in turn over the N slots (slot i of frame f has kind
    (i + f) % 10), so that the vertex / edge / interior branches, both sides of the skin, exact zeros, far points and absent points all
    occur.  require_all (every case with enough points): asserts that the oracle's answers hold all seven part codes and both signs
    and that every point's second-order term stays within its allowance (module docstring); otherwise the seed is not used."""
    v = np.asarray(verts, dtype=np.float64)
    F, V = v.shape[:2]
    rng = np.random.default_rng(seed)
    faces = np.asarray(faces)
    fg = faces[_good_faces(faces)]
    used = np.unique(fg)
    pts = np.full((F, N, 3), np.nan)
    for f in range(F):
        vn = s1.vert_normals(v[f], fg)
        tn = s1._normalize_rows(s1.tri_normals_scaled(v[f], fg))
        cen = v[f][fg].mean(axis=1)
        for i in range(N):
            kind = (i + f) % 10
            vid = rng.choice(used)
            t = rng.integers(len(fg))
            e = rng.integers(3)
            i0, i1 = fg[t, e], fg[t, (e + 1) % 3]
            if kind == 0:
                pts[f, i] = v[f, vid] + 0.0095 * vn[vid]
            elif kind == 1:
                pts[f, i] = v[f, vid] - 0.005 * vn[vid]
            elif kind in (2, 3):
                w = rng.dirichlet([4, 4, 4])
                pts[f, i] = w @ v[f][fg[t]] + (0.003 if kind == 2 else -0.003) * tn[t]
            elif kind == 4:
                pts[f, i] = 0.5 * (v[f, i0] + v[f, i1])
            elif kind == 5:
                pts[f, i] = v[f, vid]
            elif kind == 6:
                n2 = vn[i0] + vn[i1]
                pts[f, i] = 0.5 * (v[f, i0] + v[f, i1]) + rng.uniform(0.002, 0.003) * n2 / max(np.linalg.norm(n2), 1e-12)
            elif kind == 7:
                pts[f, i] = v[f, vid] + rng.uniform(0.002, 0.003) * vn[vid]
            elif kind == 8:
                d = rng.normal(size=3)
                pts[f, i] = v[f].mean(axis=0) + rng.uniform(0.5, 1.0) * d / np.linalg.norm(d)
    if require_all:
        parts, signs = set(), set()
        for f in range(F):
            a, b, c = (v[f][fg[:, k]] for k in range(3))
            L = np.sqrt(np.maximum(((a - b) ** 2).sum(1), np.maximum(((b - c) ** 2).sum(1), ((c - a) ** 2).sum(1))))
            T = (L ** 3 / np.linalg.norm(np.cross(b - a, c - a), axis=1)).max()       # k L / 2 = L^3 / (2 area)
            assert T <= C3 * frame_radius(v[f:f + 1], pts[f:f + 1])[0], (f, T)
            fin = np.isfinite(pts[f]).all(axis=1)
            d, tri, part = s1.signed_surface_distance(pts[f][fin], v[f], fg)
            parts |= set(part.tolist())
            signs |= set(np.sign(d[np.abs(d) > 1e-6]).tolist())
            a, b, c = (v[f][fg[tri, k]] for k in range(3))
            L = np.sqrt(np.maximum(((a - b) ** 2).sum(1), np.maximum(((b - c) ** 2).sum(1), ((c - a) ** 2).sum(1))))
            area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
            k = L * L / area
            x = k * U32 * ((6 + k) * np.abs(d) + 30 * L)
            with np.errstate(divide='ignore'):
                e2 = np.minimum(x, x * x / (2 * np.abs(d)))
            R = frame_radius(v[f:f + 1], pts[f:f + 1])[0]
            assert (e2 <= C2 * U32 * R).all(), (seed, f, (e2 / (U32 * R)).max())
        assert parts == set(range(7)) and signs == {-1.0, 1.0}, (seed, parts, signs)
    return pts


def build_points(verts, faces, N, seed=0, require_all=True):
    """_build_points with the first of the seeds seed, seed + 1, ... whose points meet its conditions (decided by the oracle and the
    mesh alone); (points, the seed used)."""
    last = None
    for s in range(seed, seed + 40):
        try:
            return _build_points(verts, faces, N, s, require_all), s
        except AssertionError as e:
            last = e
    raise AssertionError(f'no seed in [{seed}, {seed + 40}) gives points that meet the conditions: {last}')


def all_distances(p, v, faces):
    """|p - closest point| of every point to every face [n, NF] in f64 (a face that names a vertex twice: inf)."""
    n, nf = len(p), len(faces)
    good = _good_faces(faces)
    out = np.full((n, nf), np.inf)
    g = np.flatnonzero(good)
    a, b, c = v[faces[g, 0]], v[faces[g, 1]], v[faces[g, 2]]
    for i in range(n):
        q, _ = s1._closest_on_triangles(np.broadcast_to(p[i], (len(g), 3)), a, b, c)
        out[i, g] = np.sqrt(((q - p[i]) ** 2).sum(axis=1))
    return out


def _feature_point(p, a, b, c, part):
    """The closest point to p ON THE FEATURE of triangle (a, b, c) that `part` names: the plane's foot (0), a segment (1-3), a vertex."""
    tri = (a, b, c)
    if part >= 4:
        return tri[part - 4]
    if part >= 1:
        s, e = tri[part - 1], tri[part % 3]
        t = np.clip(((p - s) @ (e - s)) / ((e - s) @ (e - s)), 0.0, 1.0)
        return s + t * (e - s)
    n = np.cross(b - a, c - a)
    return p - ((p - a) @ n) / (n @ n) * n


def check(res, verts, points, faces, label=''):
    """A device result (capi.SurfaceDistance) against the oracle on the same inputs; prints the measured maxima beside the bounds and
    returns them as a dict."""
    dtype = res.distance.dtype
    v = np.asarray(verts, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64)
    faces = np.asarray(faces)
    good = _good_faces(faces)
    gid = np.flatnonzero(good)                    # the oracle sees the faces that can win; its ids map back through gid
    fg = faces[good]
    F, N = p.shape[:2]
    assert res.distance.shape == (F, N) and res.face.shape == (F, N) and res.part.shape == (F, N) and res.nearest.shape == (F, N, 3)
    bound = bound_for(dtype, v, p)
    worst = dict(dist=0.0, eval=0.0, nearest=0.0)
    n_fin = n_sign_skipped = n_strict = 0
    for f in range(F):
        fin = np.isfinite(p[f]).all(axis=1)
        assert np.isnan(res.distance[f][~fin]).all() and (res.face[f][~fin] == -1).all() and (res.part[f][~fin] == -1).all()
        assert np.isnan(res.nearest[f][~fin]).all()
        assert np.isfinite(res.distance[f][fin]).all() and np.isfinite(res.nearest[f][fin]).all()
        if not fin.any():
            continue
        pf = p[f][fin]
        bd = bound[f]
        d, tri, part = s1.signed_surface_distance(pf, v[f], fg)
        tri = gid[tri]
        got_d = res.distance[f][fin].astype(np.float64)
        got_f, got_p, got_q = res.face[f][fin], res.part[f][fin], res.nearest[f][fin].astype(np.float64)
        assert ((got_f >= 0) & (got_f < len(faces))).all() and good[got_f].all() and ((got_p >= 0) & (got_p <= 6)).all()
        worst['dist'] = max(worst['dist'], np.abs(np.abs(got_d) - np.abs(d)).max())
        assert (np.abs(np.abs(got_d) - np.abs(d)) <= bd).all(), (label, f, np.abs(np.abs(got_d) - np.abs(d)).max(), bd)
        # the device's (face, part) evaluated in f64 gives the minimum, and `nearest` is that point
        alld = all_distances(pf, v[f], faces)
        srt = np.sort(alld, axis=1)
        for i in range(len(pf)):
            a, b, c = (v[f][faces[got_f[i], k]] for k in range(3))
            q = _feature_point(pf[i], a, b, c, int(got_p[i]))
            worst['eval'] = max(worst['eval'], abs(np.linalg.norm(pf[i] - q) - abs(d[i])))
            assert abs(np.linalg.norm(pf[i] - q) - abs(d[i])) <= bd, (label, f, i, got_f[i], got_p[i])
            qo, _ = s1._closest_on_triangles(pf[i][None], a[None], b[None], c[None])
            worst['nearest'] = max(worst['nearest'], np.abs(got_q[i] - qo[0]).max())
            assert np.abs(got_q[i] - qo[0]).max() <= bd, (label, f, i)
            if srt[i, 1] - srt[i, 0] > 2 * bd:
                n_strict += 1
                assert got_f[i] == tri[i] and got_p[i] == part[i], (label, f, i, got_f[i], tri[i], got_p[i], part[i])
        # the sign, where it is decided
        near = s1.nearest_on_mesh(pf, v[f], fg)[2]
        vn = s1.vert_normals(v[f], fg)
        fv = faces[tri]
        nn = np.zeros_like(pf)
        A, B, C = v[f][fv[:, 0]], v[f][fv[:, 1]], v[f][fv[:, 2]]
        it, vt, ed = part == 0, part > 3, (part > 0) & (part <= 3)
        nn[it] = np.cross(B - A, C - A)[it]
        nn[vt] = vn[fv[vt, part[vt] - 4]]
        nn[ed] = vn[fv[ed, part[ed] - 1]] + vn[fv[ed, np.mod(part[ed], 3)]]
        diff = pf - near
        with np.errstate(divide='ignore', invalid='ignore'):
            cos = np.abs((diff * nn).sum(1)) / (np.linalg.norm(diff, axis=1) * np.linalg.norm(nn, axis=1))
        decided = (np.abs(d) > bd) & (np.nan_to_num(cos) >= SIGN_COS)
        n_fin += len(pf)
        n_sign_skipped += int((~decided).sum() - (np.abs(d) <= bd).sum())
        assert (np.sign(got_d[decided]) == np.sign(d[decided])).all(), (label, f)
    worst['bound'] = float(bound.max())
    worst['undecided_signs'] = n_sign_skipped / max(n_fin, 1)
    print(f'{label} {np.dtype(dtype).name}: |d| error {worst["dist"]:.3e}, (face, part) re-evaluated {worst["eval"]:.3e}, nearest {worst["nearest"]:.3e} '
          f'(bound {worst["bound"]:.3e}); ids compared strictly on {n_strict} of {n_fin} points; signs left undecided by the oracle: '
          f'{100 * worst["undecided_signs"]:.2f} %')
    # (points ON the surface have no sign to compare; the cap is on those the oracle's own normal leaves undecided)
    assert worst['undecided_signs'] <= SIGN_CAP
    return worst
