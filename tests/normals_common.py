"""Shared by the vertex-normal / virtual-marker tests (tests/test_normals_emulation.py, tests/test_gpu_normals.py): triangulated
synthetic bodies, export inputs, the NumPy f64 reference (oracle.stagei_oracle.vert_normals / markers_latent_init) and the derived
bounds.

Bounds
  SAME_F32   f32 normals against vert_normals evaluated in f64 ON THE VERY f32 VERTICES the export returned: the kernel accumulates in
             f64 and rounds once, one rounding of a value <= 1 is 2^-24; doubled for slack.
  SAME_F64   f64 normals against vert_normals on the f64 kernel's own vertices: same formula, same precision, only summation order and
             FMA contraction differ -- ~1e-16 relative to |e1||e2|, amplified by the sliver ratio (<= ~1e3) and the vertex's
             conditioning (<= 25) on these bodies.
  b(v; eps)  first-order bound on a unit normal's error when every vertex coordinate moves by at most eps:
             2 * sum_{faces at v} 2 sqrt(3) eps (|e1| + |e2|) / |sum tn|.
"""
import functools

import numpy as np

from oracle import stageii_oracle as so
from oracle import stagei_oracle as s1
from tests.helpers import stagei_case
from tests.lbs_shape_common import F32_TOL, F64_TOL   # noqa: F401  (1e-12 / 2e-5: the per-coordinate vertex bounds of the two exports)

SAME_F32 = 2.0 ** -23
SAME_F64 = 1e-10


@functools.lru_cache(maxsize=None)
def mesh_case(model_type, n_verts):
    """stagei_case's body with faces: dict(model, faces, m) -- shared between tests, never modified."""
    c = stagei_case(model_type, n_verts=n_verts, F=1, M=8)
    return dict(model=c['model'], faces=np.ascontiguousarray(c['faces'], dtype=np.int32), m=c['m'], model_type=model_type)


def device_model(case, faces='case'):
    from moshpp_amd import capi
    mdl = case['model']
    dev = capi.Model(mdl['v_template'], mdl['shapedirs'], mdl['posedirs'], mdl['weights'], mdl['J_regressor'], mdl['parents'],
                     mdl['body_dof'], mdl['hand_dof'], mdl['hands_mean'], mdl['selected_components'])
    if faces is not None:
        dev.set_faces(case['faces'] if isinstance(faces, str) else faces)
    return dev


def inputs(case, F, seed=5):
    """pose N(0, 0.35), trans N(0, 1): the export tests' inputs."""
    rng = np.random.default_rng(seed)
    return rng.normal(0, 0.35, (F, case['m']['NP'])), rng.normal(0, 1, (F, 3))


def oracle_verts(m, pose, trans, shape=None):
    return np.stack([so.verts_forward(m, so.fullpose_from_pose(m, pose[f]), trans[f], shp=None if shape is None else shape[f])
                     for f in range(pose.shape[0])])


def ref_normals(verts, faces):
    """vert_normals in f64, frame by frame, on whatever vertices are given (f32 vertices are converted exactly)."""
    v = np.asarray(verts, dtype=np.float64)
    return np.stack([s1.vert_normals(v[f], faces) for f in range(v.shape[0])])


def normal_bound(verts, faces, eps):
    """b(v; eps) per vertex [F, V] (inf where the summed normal vanishes)."""
    v = np.asarray(verts, dtype=np.float64)
    out = np.zeros(v.shape[:2])
    for f in range(v.shape[0]):
        a, b, c = v[f][faces[:, 0]], v[f][faces[:, 1]], v[f][faces[:, 2]]
        tn = np.cross(b - a, c - a)
        l01, l12, l20 = (np.linalg.norm(x, axis=1) for x in (b - a, c - b, a - c))
        num = np.zeros(v.shape[1])
        den = np.zeros((v.shape[1], 3))
        # the two edges that meet at each corner
        for col, e in ((0, l01 + l20), (1, l01 + l12), (2, l12 + l20)):
            np.add.at(num, faces[:, col], 2 * np.sqrt(3.0) * eps * e)
            np.add.at(den, faces[:, col], tn)
        d = np.linalg.norm(den, axis=1)
        with np.errstate(divide='ignore', invalid='ignore'):
            out[f] = np.where(d > 0, 2 * num / d, np.inf)
    return out


def valence(faces, V):
    return np.bincount(np.asarray(faces).ravel(), minlength=V)


def pick_marker_vids(bound, faces, M, seed=3, limit=0.1):
    """M marker vertices among those whose bound stays below `limit` in EVERY frame, the highest-valence one among them included.
    Condition: in each frame at least 90 % of the body's vertices qualify (the bound is a per-frame quantity)."""
    frac = (bound < limit).mean(axis=1)
    print(f'vertices with b < {limit}: {100 * frac.min():.1f} .. {100 * frac.max():.1f} % per frame')
    assert frac.min() >= 0.9, frac.min()
    ok = np.flatnonzero((bound < limit).all(axis=0))
    val = valence(faces, bound.shape[1])
    rng = np.random.default_rng(seed)
    vids = rng.choice(ok, size=M - 1, replace=False)
    return np.concatenate([vids, [ok[np.argmax(val[ok])]]]).astype(np.int32)


def check_same_input(got, verts, faces):
    """Normals of the kernel against vert_normals on the same vertices, every vertex; returns the largest deviation."""
    tol = SAME_F32 if got.dtype == np.float32 else SAME_F64
    err = np.abs(got.astype(np.float64) - ref_normals(verts, faces)).max()
    print(f'{got.dtype} normals vs vert_normals on the same vertices: {err:.3e} (bound {tol:.3e})')
    assert err <= tol
    return err


def check_f64_end_to_end(dev, case, pose, trans, faces=None):
    """The f64 export + f64 normals against the oracle's verts_forward -> vert_normals, vertex by vertex within b(v; 1e-12) + 1e-12."""
    faces = case['faces'] if faces is None else faces
    orc = oracle_verts(case['m'], pose, trans)
    v64 = dev.lbs_forward(pose, trans)
    assert np.abs(v64 - orc).max() < F64_TOL
    n64 = dev.vertex_normals(v64)
    b = normal_bound(orc, faces, F64_TOL)
    fin = np.isfinite(b)
    print(f'f64 end to end: largest bound {b[fin].max():.3e}, largest error {np.abs(n64 - ref_normals(orc, faces)).max():.3e}')
    assert b[fin].max() < 1e-6          # the check is not vacuous
    err = np.abs(n64 - ref_normals(orc, faces)).max(axis=2)
    assert (err[fin] <= b[fin] + 1e-12).all()
    return v64, n64


class env:
    """with env(NAME='value'): ... -- set for the block, restored after."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        import os
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_body(dev, case, F, e2e_frames=3, faces=None, kernels=('lds', 'gather', 'f64')):
    """One body on a live handle: the f32 normals through the LDS kernel and through the gather kernel and the f64 normals, each
    against vert_normals on its own input (every vertex), the f64 path end to end against the oracle, and a repeat call bit for bit."""
    faces = case['faces'] if faces is None else faces
    pose, trans = inputs(case, F)
    v32 = dev.lbs_forward(pose, trans, dtype=np.float32)
    out = dict(pose=pose, trans=trans, v32=v32)
    from moshpp_amd import capi
    if 'lds' in kernels:
        out['n32'] = dev.vertex_normals(v32)
        assert capi.last_launch_info()[0] == 'k_vn_lds'
        check_same_input(out['n32'], v32, faces)
        np.testing.assert_array_equal(out['n32'], dev.vertex_normals(v32))
    if 'gather' in kernels:
        with env(MOSHII_VN_KERNEL='gather'):
            out['g32'] = dev.vertex_normals(v32)
            assert capi.last_launch_info()[0] == 'k_vn_gather<float>'      # the switch was seen (the two kernels give the same bits)
        check_same_input(out['g32'], v32, faces)
    if 'f64' in kernels:
        out['v64'], out['n64'] = check_f64_end_to_end(dev, case, pose[:e2e_frames], trans[:e2e_frames], faces)
        check_same_input(out['n64'], out['v64'], faces)
        np.testing.assert_array_equal(out['n64'], dev.vertex_normals(out['v64']))
        assert capi.last_launch_info()[0] == 'k_vn_gather<double>'
    return out


def check_markers(dev, case, pose, trans, vids, dist, faces=None, shape=None, rows=None):
    """virtual_markers in both precisions on a live handle, ALL frames in one call; then, on the frames `rows` (default: all) -- the
    oracle costs a frame at a time --: the same-input check (against the export's own vertices of those frames), the f64 markers
    against the oracle within F64_TOL sqrt(3) + |dist| b(v; 1e-12), and the f32 wiring check
    |marker - oracle marker| <= 2e-5 sqrt(3) + |dist| b(vid; 2e-5).  marker_normals equal the rows of the full normals call on every
    frame.  Returns {dtype: (markers, marker_normals)}."""
    faces = case['faces'] if faces is None else faces
    rows = np.arange(len(pose)) if rows is None else np.asarray(rows)
    orc = oracle_verts(case['m'], pose[rows], trans[rows], None if shape is None else shape[rows])
    orc_mk = orc[:, vids] + dist[None, :, None] * ref_normals(orc, faces)[:, vids]
    res = {}
    for dtype, eps in ((np.float64, F64_TOL), (np.float32, F32_TOL)):
        mk, mn = dev.virtual_markers(pose, trans, vids, dist, dtype=dtype, shape=shape, return_normals=True)
        assert mk.dtype == dtype and mk.shape == (len(pose), len(vids), 3)
        v = dev.lbs_forward(pose, trans, dtype=dtype, shape=shape)
        np.testing.assert_array_equal(mn, dev.vertex_normals(v)[:, vids])
        same = v[rows][:, vids].astype(np.float64) + dist[None, :, None] * ref_normals(v[rows], faces)[:, vids]
        err = np.abs(mk[rows].astype(np.float64) - same).max()
        tol = 2 * 2.0 ** -23 * np.abs(same).max() if dtype == np.float32 else SAME_F64
        print(f'{np.dtype(dtype).name} markers vs the same vertices + dist x vert_normals, {len(rows)} frames: {err:.3e} (bound {tol:.3e})')
        assert err <= tol
        b = normal_bound(orc, faces, eps)[:, vids]
        wire = np.linalg.norm(mk[rows].astype(np.float64) - orc_mk, axis=2)
        lim = eps * np.sqrt(3.0) + np.abs(dist)[None] * b
        print(f'{np.dtype(dtype).name} markers vs the oracle, {len(rows)} frames: {wire.max():.3e} m (largest allowance {lim.max():.3e})')
        assert (wire <= lim).all()
        res[dtype] = (mk, mn)
    return res


def wide_body(V=65600, n_faces=4000, seed=11):
    """A two-joint body with more than 65 535 vertices -- the face table then holds 32-bit pairs, and an f32 frame (787 KB) is beyond
    the LDS budget -- and random triangles over all of them; (model arrays for capi.Model, faces, verts[2, V, 3] f64)."""
    rng = np.random.default_rng(seed)
    vt = rng.normal(0, 0.3, (V, 3))
    w = rng.random((V, 2)); w /= w.sum(1, keepdims=True)
    jr = np.zeros((2, V)); jr[0, :10] = 0.1; jr[1, 10:20] = 0.1
    model = dict(v_template=vt, shapedirs=np.zeros((V, 3, 1)), posedirs=np.zeros((V, 3, 9)), weights=w, J_regressor=jr,
                 parents=np.array([-1, 0]), body_dof=6, hand_dof=0, hands_mean=None, selected_components=None)
    faces = rng.integers(0, V, (n_faces, 3)).astype(np.int32)
    faces[0] = [V - 1, V - 2, 65536]                          # ids that need more than 16 bits, whatever the draw
    verts = np.stack([vt, vt + rng.normal(0, 0.01, (V, 3))])
    return model, faces, verts


def check_wide_body():
    """On a live library: both precisions on the wide body against vert_normals on the same vertices."""
    model, faces, verts = wide_body()
    dev = device_model(dict(model=model), faces=faces)
    from moshpp_amd import capi
    for dtype in (np.float32, np.float64):
        v = np.ascontiguousarray(verts, dtype=dtype)
        check_same_input(dev.vertex_normals(v), v, faces)
        assert capi.last_launch_info()[0] == ('k_vn_gather<float>' if dtype == np.float32 else 'k_vn_gather<double>')
    mk = dev.virtual_markers(np.zeros((1, 6)), np.zeros((1, 3)), faces[0], [0.01, 0.01, 0.01])[0]
    vt = model['v_template']
    assert np.abs(mk - (vt[faces[0]] + 0.01 * s1.vert_normals(vt, faces)[faces[0]])).max() < 1e-10
    dev.close()
