"""Shared by the posed-joint tests (tests/test_joints_emulation.py, tests/test_gpu_joints.py): the bodies, the export inputs with their
edge frames, the NumPy f64 reference (oracle.stageii_oracle: fullpose_from_pose -> _shaped -> joint_transforms) and the bounds.

Bounds
  F64_TOL   1e-12 m: the project's figure for "same formula, other order of operations" (tests/lbs_shape_common.py); the unitless
            rotation entries are held to the same value.
  f32       moshii_joints_f32 computes in f64 from its f32 inputs and rounds once on the store: every value within
            2^-24 max(|oracle value|, 2^-126) + F64_TOL of the oracle on the same f32 inputs (converted exactly); and, bit for bit,
            _f32 == _f64(on the f32 inputs).astype(float32).
  ORTHO     every f64 rot[f][k] is orthonormal to 1e-12: a product of at most 64 rotations, each orthonormal to a few 1e-16.
"""
import functools

import numpy as np

from moshpp_amd import synth
from oracle import stageii_oracle as so
from tests import normals_common as nc
from tests.lbs_shape_common import F32_TOL, F64_TOL, block_case   # noqa: F401

ORTHO_TOL = 1e-12
NAMES = {(np.float32, False): 'k_joints<float>', (np.float64, False): 'k_joints<double>',
         (np.float32, True): 'k_joints_shape<float>', (np.float64, True): 'k_joints_shape<double>'}


# ---- bodies ---------------------------------------------------------------------------------------------------------------------
def _body(model, m, betas=None, E=0, start=0, name=''):
    return dict(model=model, m=m, betas=betas, E=E, start=start, name=name)


def tree_model(parents, seed, E=0, NB0=4):
    """A random small model (V = 2 K) over the kinematic tree `parents`: (model arrays for capi.Model, betas); the last E shapedirs
    columns are meant as a free block."""
    rng = np.random.default_rng(seed)
    parents = np.asarray(parents, dtype=np.int64)
    K = len(parents)
    V = 2 * K
    w = rng.random((V, K)) + 0.01
    jr = rng.random((K, V)) + 0.01
    model = dict(v_template=rng.normal(0, 0.3, (V, 3)), shapedirs=rng.normal(0, 0.01, (V, 3, NB0 + E)),
                 posedirs=rng.normal(0, 0.001, (V, 3, 9 * (K - 1))), weights=w / w.sum(1, keepdims=True),
                 J_regressor=jr / jr.sum(1, keepdims=True), parents=parents, body_dof=3 * K, hand_dof=0, hands_mean=None,
                 selected_components=None)
    betas = np.concatenate([rng.normal(0, 1, NB0), np.zeros(E)])
    return model, betas


@functools.lru_cache(maxsize=None)
def body(name):
    """dict(model, m (the oracle's prepared model), betas | None, E, start, name) -- shared between tests, never modified.
    mano / smpl / smplh (hand PCA: body_dof 66, hand_dof 24): normals_common.mesh_case; smplx: lbs_shape_common.block_case with E = 5
    coefficients; horse: the SMAL horse of tests/animal_oracle.py; one / chain / star: hand-made trees of K = 1 and K = 64 (the
    deepest tree the ABI admits, and depth 1 with every lane fetching from lane 0); pinned: see pinned_body."""
    if name in ('mano', 'smpl', 'smplh'):
        c = nc.mesh_case(name, {'mano': 778, 'smpl': 1500, 'smplh': 1500}[name])
        if name == 'smplh':
            assert (c['model']['body_dof'], c['model']['hand_dof']) == (66, 24)
        return _body(c['model'], c['m'], name=name)
    if name == 'smplx':
        c = block_case('smplx', 5)
        return _body(c['model'], c['m'], betas=c['s']['betas'], E=c['E'], start=c['start'], name=name)
    if name == 'horse':
        from tests.animal_oracle import animal_case
        c = animal_case('animal_horse', F=1, M=40)
        return _body(c['model'], c['m'], betas=c['s']['betas'], name=name)
    if name in ('one', 'chain', 'star'):
        parents = {'one': [-1], 'chain': list(range(-1, 63)), 'star': [-1] + [0] * 63}[name]
        model, betas = tree_model(parents, seed=len(name) + 20)
        return _body(model, so.prepare_model(model, betas), betas=betas, name=name)
    if name == 'pinned':
        return pinned_body()
    raise KeyError(name)


PINNED_E = 3


def pinned_body():
    """A body whose joints ARE vertices: for every joint k the vertex v_k = k has J_regressor[k, v_k] = 1 (the row's only entry),
    weights[v_k, k] = 1 and a zero posedirs row; shapedirs is arbitrary, so J_k == v_shaped[v_k] with any betas and any coefficients of
    the free block (the last PINNED_E columns).  The full-mesh export then puts vertex v_k where the chain puts joint k."""
    parents = [-1, 0, 1, 1, 3, 0, 5, 6, 6]
    model, betas = tree_model(parents, seed=77, E=PINNED_E)
    K, V = len(parents), 2 * len(parents)
    jr = np.zeros((K, V)); jr[np.arange(K), np.arange(K)] = 1.0
    w = model['weights'].copy(); w[:K] = np.eye(K)
    pd = model['posedirs'].copy(); pd[:K] = 0.0
    model = dict(model, J_regressor=jr, weights=w, posedirs=pd)
    m = so.prepare_model(model, betas)
    start = model['shapedirs'].shape[2] - PINNED_E
    so.set_free_shape(m, start, PINNED_E)
    return _body(model, m, betas=betas, E=PINNED_E, start=start, name='pinned')


def device(b):
    """A live handle for a body: betas and free block as the oracle's model has them."""
    from moshpp_amd import capi
    mdl = b['model']
    dev = capi.Model(mdl['v_template'], mdl['shapedirs'], mdl['posedirs'], mdl['weights'], mdl['J_regressor'], mdl['parents'],
                     mdl['body_dof'], mdl['hand_dof'], mdl['hands_mean'], mdl['selected_components'])
    if b['betas'] is not None:
        dev.set_betas(b['betas'])
    if b['E']:
        dev.set_free_shape(b['start'], b['E'])
    return dev


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def inputs(b, F, dtype, seed=5):
    """(pose[F, NP], trans[F, 3], shape[F, E] | None) as arrays of `dtype`: the export tests' N(0, 0.35) / N(0, 1) / N(0, 1.2) draws
    (normals_common.inputs, lbs_shape_common.export_inputs), with
      frame 0        two body joints at |r| = 1e-3 (1 -+ 4 ulp of dtype): t^2 on either side of the 1e-6 switch (a body with one free
                     body joint has the lower side only)
      frame 1        all zeros: the series branch of every joint
      frame 2        |r| = pi - 1e-9 on the root
    as far as F reaches."""
    m = b['m']
    rng = np.random.default_rng(seed)
    pose = rng.normal(0, 0.35, (F, m['NP']))
    trans = rng.normal(0, 1, (F, 3))
    shape = rng.normal(0, 1.2, (F, b['E'])) if b['E'] else None
    if F >= 2:
        pose[1] = 0.0
    if F >= 3:
        d = rng.normal(0, 1, 3)
        pose[2, :3] = d / np.linalg.norm(d) * (np.pi - 1e-9)
    pose, trans = np.ascontiguousarray(pose, dtype=dtype), np.ascontiguousarray(trans, dtype=dtype)
    if shape is not None:
        shape = np.ascontiguousarray(shape, dtype=dtype)
    nb = m['body_dof'] // 3
    eps = np.finfo(dtype).eps
    sides = [(nb - 1, -1)] + ([(nb // 2, +1)] if nb >= 3 else [])
    for j, sign in sides:
        r = (np.array([0.6, 0.0, 0.8]) * (1e-3 * (1 + sign * 4 * eps))).astype(dtype)
        pose[0, 3 * j:3 * j + 3] = r
        t2 = (r.astype(np.float64) ** 2).sum()
        assert (t2 < 1e-6) == (sign < 0) and abs(t2 - 1e-6) < 1e-6 * 32 * eps, (t2, sign)
    return pose, trans, shape


# ---- reference and checker ------------------------------------------------------------------------------------------------------
def oracle(m, pose, trans, shape=None):
    """(joints[F, K, 3], rot[F, K, 3, 3]) in NumPy f64: joint_transforms(...)[3] + trans and its Rw."""
    pose, trans = np.asarray(pose, dtype=np.float64), np.asarray(trans, dtype=np.float64)
    joints, rot = [], []
    for f in range(pose.shape[0]):
        _, J = so._shaped(m, slice(0, 0), None if shape is None else np.asarray(shape[f], dtype=np.float64))
        _, _, Rw, tw = so.joint_transforms(m, so.fullpose_from_pose(m, pose[f]), J)
        joints.append(tw + trans[f]); rot.append(Rw)
    return np.stack(joints), np.stack(rot)


def check(joints, rot, m, pose, trans, shape, dtype, ref=None):
    """joints (and rot, or None) of the library against the oracle on the very inputs the device saw; returns the oracle's pair."""
    K = m['K']
    F = pose.shape[0]
    assert joints.dtype == dtype and joints.shape == (F, K, 3)
    assert pose.dtype == dtype and trans.dtype == dtype and (shape is None or shape.dtype == dtype)
    oj, orot = oracle(m, pose, trans, shape) if ref is None else ref
    pairs = [('joints', joints, oj)]
    if rot is not None:
        assert rot.dtype == dtype and rot.shape == (F, K, 3, 3)
        pairs.append(('rot', rot, orot))
    for what, got, want in pairs:
        err = np.abs(got.astype(np.float64) - want)
        if dtype == np.float64:
            bound = np.full(want.shape, F64_TOL)
        else:
            bound = 2.0 ** -24 * np.maximum(np.abs(want), 2.0 ** -126) + F64_TOL
        print(f'{np.dtype(dtype).name} {what} vs the oracle, F={F} K={K}: largest error {err.max():.3e}, '
              f'largest error / bound {(err / bound).max():.3f} (bound at that value {bound.ravel()[np.argmax(err / bound)]:.3e})')
        assert np.isfinite(got).all()
        assert (err <= bound).all()
    if rot is not None and dtype == np.float64:
        dev = np.abs(np.einsum('fkab,fkcb->fkac', rot, rot) - np.eye(3)).max()
        print(f'rot rot^T - I: {dev:.3e} (bound {ORTHO_TOL:.0e})')
        assert dev <= ORTHO_TOL
    return oj, orot


def run_body(dev, b, F, seed=5):
    """One body on a live handle, both precisions: the call with rotations held to the checker, the launch name, the call without
    rotations bit for bit, and _f32 == _f64(on the f32 inputs) rounded.  Returns {dtype: (pose, trans, shape, joints, rot)}."""
    from moshpp_amd import capi
    out = {}
    for dtype in (np.float64, np.float32):
        pose, trans, shape = inputs(b, F, dtype, seed)
        joints, rot = dev.posed_joints(pose, trans, shape=shape, dtype=dtype, return_rotations=True)
        assert capi.last_launch_info()[0] == NAMES[(dtype, shape is not None)]
        assert capi.last_launch_info()[1] == 0            # no LDS
        check(joints, rot, b['m'], pose, trans, shape, dtype)
        np.testing.assert_array_equal(joints, dev.posed_joints(pose, trans, shape=shape, dtype=dtype))
        if dtype == np.float32:
            j64, r64 = dev.posed_joints(pose.astype(np.float64), trans.astype(np.float64), dtype=np.float64, return_rotations=True,
                                        shape=None if shape is None else shape.astype(np.float64))
            np.testing.assert_array_equal(joints, j64.astype(np.float32))
            np.testing.assert_array_equal(rot, r64.astype(np.float32))
        out[dtype] = (pose, trans, shape, joints, rot)
    return out


def check_pinned(dev, b, F, with_shape, dtype=np.float64, tol=2 * F64_TOL):
    """On the pinned body: vertex v_k = k of the full-mesh export is joint k of posed_joints."""
    pose, trans, shape = inputs(b, F, dtype)
    if not with_shape:
        shape = None
    K = b['m']['K']
    verts = dev.lbs_forward(pose, trans, dtype=dtype, shape=shape)
    joints = dev.posed_joints(pose, trans, shape=shape, dtype=dtype)
    err = np.abs(verts[:, :K].astype(np.float64) - joints.astype(np.float64)).max()
    print(f'pinned body, {np.dtype(dtype).name}, shape row {with_shape}: export vertex vs joint {err:.3e} (bound {tol:.1e})')
    assert err <= tol
    if with_shape:        # ... and the coefficients do move them
        assert np.abs(joints - dev.posed_joints(pose, trans, dtype=dtype)).max() > 1e-4
