"""The Stage-II chain kernel at the edges of its size classes: one table of cases, one cached case builder and one checker, shared by
tests/test_chain_edges_emulation.py (the kernels compiled by g++, CPU fibers) and tests/test_gpu_chain_edges.py (the hipcc build on
the device).

k_chain_solve is built in 17 instantiations (NBLK register blocks of 16 rows; plain 2 / 4 / 5 / 7 / 8, extended `xt` 5 / 8 / 10 / 13,
cooperative forms of all but plain 2) and inside one of them the number of unknowns n = 3 + free pose ids + free shape coefficients
is a run-time value that steers the panel loop of the LDL^T factorisation (last panel full / partial, the border row n that carries
the right-hand side, rows beyond it), the number of row slots, the square / packed / global-memory factor and the tile count of the
cooperative exchange.  The model families give only a handful of n; here the free-id lists of moshii_solve_opts (and of the oracle:
stageii_chain(..., id_sets=...)) put n on 16 k - 1, 16 k, 16 k + 1, on the largest n of every class, and Step 1 on a panel boundary
inside a larger instantiation.  The marker side gets the same treatment: marker counts on and next to the tile height, MOSHII_TM,
tiles without a visible marker, cooperative ranks with an empty or one-marker share.

Families (CASES below; `python -m tests.chain_edges` lists them with the conditioning guard's figures):
  A  plain variant, SMPL-H with 30 PCA coefficients per hand (126 pose variables), 53 markers over body and hands:
     step1 = root + the first k body ids (+ the first h1 hand coefficients where n1 > 69), step2 = step1 + hand coefficients from id
     66 up to h in all.  n2 = 15 ... 127; four cases whose Step 1 ends on a panel boundary inside a larger instantiation.
  B  the n2 = 16 and n2 = 63 problems of A forced into every larger instantiation (MOSHII_FORCE_NBLK).
  C  extended variant, SMPL-X with jaw + E expression coefficients: n = 79, 80 (no fingers), 127, 128, 159, 160, 207 (fingers).
  D  cooperative chains at the same edges (each also against its plain chain), and rank-share edges: 6 / 12 markers over 8 ranks.
  E  marker tiles: M = 40, 41, 80, 81; M = 15 with MOSHII_TM = 1, 5, 7, 15 (and M = 81 with 16, 20, 27); hidden tiles, one marker per tile, only the last tile.

To add a case: add a row to CASES (a `_case(...)` call: family, how the inputs are built, the free-id lists or the model's own, the
environment, the cooperative group size and the kernel name EXPECTED -- written out by hand from the tables NBLK_PLAIN / NBLK_XT
below, never computed from product code), run `python -m tests.chain_edges NAME` and keep the seed only if the guard passes: the
oracle, run again on observations perturbed by 1e-13 m Gaussian noise, keeps every iteration count and moves its solution by less
than guard()'s limit (below), and the last free pose variable / shape coefficient leaves its start value by more than 1e-3 in some
frame.  Both test files pick the case up from the table.

The checker (check_case): status as the oracle's frame_ids say; the kernel name; dogleg iteration counts equal to the oracle's frame
by frame; pose / trans / shape within the tier's bound (emulation: 1e-9 rad / 1e-10 m plain, 1e-8 xt, 2e-8 beyond 127 unknowns, as
tests/test_chain_emulation.py; device: 1e-7, TIGHT of tests/test_gpu_parity.py); error columns to rtol 1e-6; every pose variable free
in neither step bitwise at its start value; on the device every solve runs twice and every output must have the same bits.

Conditioning guard.  The limit asked of a case is 1/100 of its bound, and a case has two bounds.  Against the device bound (1e-7)
that is 1e-9 rad, which every case below meets with two decades to spare.  Against the plain variant's emulation bound (1e-9 rad) it
is 1e-11 rad, and that is below what the geometry allows: 1e-13 m at a marker that sits 0.5 - 1 cm from a finger's or a wrist's axis
is 1 - 2e-11 rad.  Five seeds of every case of family A and of the 15-marker body solves of family E moved by 1.1e-11 ... 3e-11 rad
at best (5e-12 with 40 and more markers on the body alone), so no choice of seed gets there and dropping is not an answer for half
the table.  guard() therefore enforces min(1/100 of the device bound, 1/10 of the emulation bound) -- 1e-10 rad / 1e-11 m for the
plain variant, 1e-9 for xt -- and prints whether a case meets 1/100 of the emulation bound as well: all of C, the xt cases of D,
D-share-*, D-smpl-M41 and E-M40 ... E-M81 do; A, B, the plain n2 cases of D and E-M15-* (1.4e-11 ... 7.3e-11 rad) do not.  Seeds:
family A's default seed 1 moved up to 1e-9 rad at n2 = 31 ... 49 (and came within 4 % of the emulation bound there), seed 2 is the
best of five over the whole sweep; A-n80-n113 (Step 1 with eleven hand coefficients and no finger term) is ill-conditioned at seeds
1, 2, 3, 5 (1.6e-8 ... 2.3e-4 rad) and well at 4; C-n207 failed at seed 5 (3.6e-10 against 2e-10) and passes at 6; D-share-M12
passes 1/100 of the emulation bound at seed 4.  No case was dropped.

Worst deviation from the oracle per family, max over pose (rad) and shape (RESULTS at the end of this module has the cases):
    family   emulation   device (MI355X)
    A        5.7e-11     7.7e-11
    B        4.9e-12     5.8e-12
    C        3.5e-11     6.1e-11
    D        6.8e-11     7.4e-11
    E        7.3e-13     1.4e-12
The emulation column is what `python -m tests.chain_edges --deviations` prints, the device column what the last test of
tests/test_gpu_chain_edges.py prints.  Teeth, shown once on a scratch copy in emulation: without the right-hand side's row q1 == n
in the last register block of ldl_factor, 17 of family A's 26 cases fail (every one whose n lies in the last block of its
instantiation); `c0 + 16 < c.n` for `<=` in ldl_panels fails none -- it only sends a full last panel down the general path."""
import contextlib
import functools
import os

import numpy as np

from oracle import stageii_oracle as so
from tests.helpers import device_case, oracle_case, shape_case

# The smallest instantiation whose 16 NBLK rows hold the n unknowns and the right-hand side's row (n + 1 <= 16 NBLK), written out:
# (largest n, NBLK) per class.
NBLK_PLAIN = ((31, 2), (63, 4), (79, 5), (111, 7), (127, 8))
NBLK_XT = ((79, 5), (127, 8), (159, 10), (207, 13))
# every instantiation of chain_solve.hip's MOSHII_INSTANTIATE list, as last_launch_info() spells it with the group size cut off
INSTANTIATIONS = (['k_chain_solve<%d,1>' % b for b in (2, 4, 5, 7, 8)] + ['k_chain_solve<%d,1,xt>' % b for b in (5, 8, 10, 13)] +
                  ['k_chain_solve<%d,1,coop>' % b for b in (4, 5, 7, 8)] + ['k_chain_solve<%d,1,xt,coop>' % b for b in (5, 8, 10, 13)])

BODY = list(range(3, 66))      # SMPL-H / SMPL-X body pose ids (the prior sees all 63, free or not)
CASES = {}


def _case(name, family, kernel, **kw):
    c = dict(name=name, family=family, kernel=kernel, model='smplh', seed=2, M=53, F=3, dph=30, body_only=False, dropout=None, ids=None,
             fingers=False, E=0, G=0, env={}, vis=None)
    assert name not in CASES and not set(kw) - set(c), (name, kw)
    c.update(kw)
    CASES[name] = c
    return c


def sweep_ids(n1, n2):
    """Family A's free sets for n1 / n2 unknowns in Step 1 / Step 2: (k body ids, h1 hand coefficients in Step 1, h in Step 2)."""
    h = max(6, n2 - 69) if n1 is None else n2 - min(n1, 69)
    h1 = 0 if n1 is None else max(0, n1 - 69)
    k = n2 - 6 - h
    assert 0 <= k <= 63 and 0 <= h1 <= h <= 60 and 6 + k + h == n2 and (n1 is None or 6 + k + h1 == n1)
    return k, h1, h


def id_sets_of(c):
    if c['ids'] is None:
        return None
    k, h1, h = c['ids']
    step1 = [0, 1, 2] + BODY[:k] + list(range(66, 66 + h1))
    finger = list(range(66, 66 + h))
    return BODY, finger, step1, sorted(set(step1 + finger))


# ---- A: the unknown-count sweep of the plain variant ------------------------------------------------------------------------------
A_KERNEL = {15: 2, 16: 2, 17: 2, 31: 2, 32: 4, 33: 4, 47: 4, 48: 4, 49: 4, 63: 4, 64: 5, 65: 5, 79: 5, 80: 7, 81: 7, 95: 7, 96: 7, 97: 7,
            111: 7, 112: 8, 113: 8, 127: 8}
for _n2, _b in A_KERNEL.items():
    _case(f'A-n{_n2}', 'A', f'k_chain_solve<{_b},1>', ids=sweep_ids(None, _n2))
for _n1, _n2, _b in ((64, 97, 7), (48, 81, 7), (16, 33, 4), (80, 113, 8)):      # Step 1 ends on a panel boundary inside a larger instantiation
    _case(f'A-n{_n1}-n{_n2}', 'A', f'k_chain_solve<{_b},1>', ids=sweep_ids(_n1, _n2), seed=4 if _n1 == 80 else 2)

# ---- B: one problem through every larger instantiation ----------------------------------------------------------------------------
for _n2, _forced in ((16, (4, 5, 7, 8)), (63, (4, 5, 7, 8))):
    for _b in _forced:
        _case(f'B-n{_n2}-force{_b}', 'B', f'k_chain_solve<{_b},1>', ids=sweep_ids(None, _n2), env={'MOSHII_FORCE_NBLK': str(_b)})

# ---- C: the extended variant (SMPL-X, jaw free, E expression coefficients; n = 66 + E without, 114 + E with fingers) ---------------
for _E, _n, _b in ((13, 79, 5), (14, 80, 8)):
    _case(f'C-n{_n}', 'C', f'k_chain_solve<{_b},1,xt>', model='smplx', seed=3, M=40, E=_E)
for _E, _n, _b in ((13, 127, 8), (14, 128, 10), (45, 159, 10), (46, 160, 13), (93, 207, 13)):
    _case(f'C-n{_n}', 'C', f'k_chain_solve<{_b},1,xt>', model='smplx', seed=6 if _n == 207 else 5, M=60, F=2, E=_E, fingers=True)

# ---- D: cooperative chains at the same edges --------------------------------------------------------------------------------------
for _n2, _b, _G in ((48, 4, 3), (64, 5, 3), (80, 7, 3), (112, 8, 3), (127, 8, 8)):
    _case(f'D-n{_n2}-coop{_G}', 'D', f'k_chain_solve<{_b},1,coop{_G}>', ids=sweep_ids(None, _n2), G=_G)
_case('D-xt-n79-coop3', 'D', 'k_chain_solve<5,1,xt,coop3>', model='smplx', seed=3, M=40, E=13, G=3)
_case('D-xt-n80-coop3', 'D', 'k_chain_solve<8,1,xt,coop3>', model='smplx', seed=3, M=40, E=14, G=3)     # (the cooperative xt 8 of no other case)
_case('D-xt-n128-coop3', 'D', 'k_chain_solve<10,1,xt,coop3>', model='smplx', seed=5, M=60, F=2, E=14, fingers=True, G=3)
_case('D-xt-n160-coop5', 'D', 'k_chain_solve<13,1,xt,coop5>', model='smplx', seed=5, M=60, F=2, E=46, fingers=True, G=5)
_case('D-xt-n207-coop8', 'D', 'k_chain_solve<13,1,xt,coop8>', model='smplx', seed=6, M=60, F=2, E=93, fingers=True, G=8)
# rank shares: seven marker ranks + the prior's rank over 6 / 12 markers (empty and one-marker shares); SMPL, 69 unknowns: cooperative NBLK 5
_case('D-share-M6-coop8', 'D', 'k_chain_solve<4,1,coop8>', seed=4, M=6, dph=24, body_only=True, dropout=0.0, G=8)
_case('D-share-M12-coop8', 'D', 'k_chain_solve<4,1,coop8>', seed=4, M=12, dph=24, body_only=True, dropout=0.0, G=8)
_case('D-smpl-M41-coop8', 'D', 'k_chain_solve<5,1,coop8>', model='smpl', seed=3, M=41, dph=24, body_only=True, dropout=0.0, G=8)

# ---- E: marker tiles (SMPL-H body solve, 63 unknowns, no dropout) ------------------------------------------------------------------
for _M in (40, 41, 80, 81):
    _case(f'E-M{_M}', 'E', 'k_chain_solve<4,1>', seed=3, M=_M, dph=24, body_only=True, dropout=0.0)
# MOSHII_TM.  The tile buffers share their LDS with the LDL^T factor (make_layout: max(tile area, factor, 16 x 256 exchange tile)), so the
# launch's LDS size shows the tile height only once the tile area is the largest of the three: at 63 unknowns from 15 markers a tile
# on.  Of MOSHII_TM = 1, 5, 7, 15 on 15 markers the last one alone can differ from the others in LDS bytes (and does); the second group,
# 81 markers in tiles of 16 / 20 / 27 (5 + 1, 4 + 1, 3 tiles), is where every setting gives an LDS size of its own.
TM_CASES = {15: [], 81: []}
for _M, _tms in ((15, (1, 5, 7, 15)), (81, (16, 20, 27))):
    for _tm in _tms:
        TM_CASES[_M].append(_case(f'E-M{_M}-tm{_tm}', 'E', 'k_chain_solve<4,1>', seed=3, M=_M, dph=24, body_only=True, dropout=0.0,
                                  env={'MOSHII_TM': str(_tm)})['name'])
TM_NAMES = TM_CASES[15] + TM_CASES[81]
# visibility patterns of frame 1 (tiles of 5: markers 0-4, 5-9, 10-14): one whole tile hidden; three markers, one per tile; only the last tile
VIS = {'tilehidden': [0, 1, 2, 3, 4, 10, 11, 12, 13, 14], 'onepertile': [0, 7, 14], 'lasttile': [10, 11, 12, 13, 14]}
for _p in VIS:
    _case(f'E-M15-tm5-{_p}', 'E', 'k_chain_solve<4,1>', seed=3, M=15, dph=24, body_only=True, dropout=0.0, env={'MOSHII_TM': '5'}, vis=_p)
    _case(f'E-M15-{_p}-coop3', 'E', 'k_chain_solve<4,1,coop3>', seed=3, M=15, dph=24, body_only=True, dropout=0.0, vis=_p, G=3)


def names(family=None):
    return [n for n, c in CASES.items() if family is None or c['family'] == family]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pose_inputs(model, seed, M, dph, F, body_only, dropout):
    kw = {} if dropout is None else dict(dropout=dropout, n_gaps=0)
    return oracle_case(model, F=F, M=M, seed=seed, dof_per_hand=dph, body_only_markers=body_only, **kw)


@functools.lru_cache(maxsize=None)
def _shape_inputs(seed, M, E, F):
    return shape_case('smplx', F=F, M=M, E=E, seed=seed, kind='expr')


def inputs(c):
    """(case dict of tests/helpers.py, vis[F, M]) -- shared between the cases built on the same model, never written to."""
    if c['E']:
        case = _shape_inputs(c['seed'], c['M'], c['E'], c['F'])
    else:
        case = _pose_inputs(c['model'], c['seed'], c['M'], c['dph'], c['F'], c['body_only'], c['dropout'])
    vis = case['vis']
    if c['vis'] is not None:
        vis = vis.copy()
        vis[1] = False
        vis[1, VIS[c['vis']]] = True
    return case, vis


def n_unknowns(c):
    """(n1, n2) of the case, from its own id lists."""
    case, _ = inputs(c)
    ids = id_sets_of(c)
    if ids is None:
        _, _, _, st1, st2 = so.pose_id_sets(c['model'], case['m']['NP'], c['fingers'], optimize_face=bool(c['E']))
    else:
        st1, st2 = ids[2], ids[3]
    return 3 + len(st1), 3 + len(st2) + c['E']


def _oracle_kw(c):
    ids = id_sets_of(c)
    kw = dict(optimize_fingers=c['fingers'] or bool(ids and ids[1]), id_sets=ids)
    if c['E']:
        kw.update(optimize_face=True, free_shape='expr')
    return kw


def run_oracle(c, obs=None):
    case, vis = inputs(c)
    return so.stageii_chain(case['m'], case['prior'], case['closest'], case['coef'], case['obs'] if obs is None else obs, vis, c['model'],
                            **_oracle_kw(c))


@functools.lru_cache(maxsize=None)
def reference(name):
    return run_oracle(CASES[name])


def free_ids(c):
    """(step1, step2) as both sides get them."""
    case, _ = inputs(c)
    ids = id_sets_of(c)
    if ids is not None:
        return ids[2], ids[3]
    _, _, _, st1, st2 = so.pose_id_sets(c['model'], case['m']['NP'], c['fingers'], optimize_face=bool(c['E']))
    return st1, st2


# ---- the device side ------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def environment(env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bounds(c, tier):
    """(pose / shape bound in rad, trans bound in m) of the case in `tier` ('emulation' | 'gpu')."""
    if tier == 'gpu':
        return 1e-7, 1e-7
    if not c['E']:
        return 1e-9, 1e-10
    b = 2e-8 if n_unknowns(c)[1] > 127 else 1e-8
    return b, b


OUT_KEYS = ('pose', 'fullpose', 'trans', 'markers_sim', 'errs', 'iters', 'status', 'shape')
ERR_COLS = (('data', 0), ('poseB', 1), ('velo', 2), ('poseH', 3), ('poseF', 4), ('shape', 5))
ASSERTED_KERNELS = set()       # every kernel name a check_case of this process has asserted
DEVIATIONS = {}                # (tier, case) -> max|pose - oracle|


def check_case(capi, name, tier):
    """Solve case `name` through `capi` (the loaded library: emulation or device) and hold it to the oracle.  Returns
    (kernel name, LDS bytes) of the launch."""
    c = CASES[name]
    case, vis = inputs(c)
    ref = reference(name)
    ids = id_sets_of(c)
    tol, tol_t = bounds(c, tier)
    with environment(c['env']):
        dev = device_case(case, optimize_fingers=c['fingers'] or bool(ids and ids[1]), optimize_face=bool(c['E']),
                          shape_kind='expr' if c['E'] else None, id_sets=ids)
        ch = [dict(attach=dev['attach'], obs=case['obs'], vis=vis, first=True)]

        def solve(g):
            out = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], ch, coop=g)[0]
            return out, capi.last_launch_info()

        out, (kernel, lds, _) = solve(c['G'] or 1)
        again = solve(c['G'] or 1)[0] if tier == 'gpu' else None
        plain = solve(1) if c['G'] else None
    F, NP = out['pose'].shape
    assert out['status'].tolist() == [0 if t in set(ref['frame_ids'].tolist()) else 1 for t in range(F)]
    solved = ref['frame_ids']
    assert kernel == c['kernel'], (kernel, c['kernel'])
    ASSERTED_KERNELS.add(kernel)
    dp = float(np.abs(out['pose'][solved] - ref['pose']).max())
    dt = float(np.abs(out['trans'][solved] - ref['trans']).max())
    ds = float(np.abs(out['shape'][solved] - ref['shape']).max()) if c['E'] else 0.0
    DEVIATIONS[(tier, name)] = max(dp, ds)
    print(f'{name}: {kernel} lds {lds} iters {out["iters"][:, 0].tolist()} oracle {ref["iters"].tolist()} '
          f'max|dpose| {dp:.2e} |dtrans| {dt:.2e} |dshape| {ds:.2e} (bound {tol:.0e} / {tol_t:.0e})')
    np.testing.assert_array_equal(out['iters'][solved, 0], ref['iters'])
    assert dp < tol and dt < tol_t and ds < tol, (dp, dt, ds)
    assert float(np.abs(out['fullpose'][solved] - ref['fullpose']).max()) < tol
    for key, col in ERR_COLS:
        if key in ref['errs']:
            r = ref['errs'][key]                      # (the velocity term: the frames that have one -- the last ones)
            np.testing.assert_allclose(out['errs'][solved[len(solved) - len(r):], col], r, rtol=1e-6, atol=1e-12 if key == 'velo' else 0.0,
                                       err_msg=key)
    st1, st2 = free_ids(c)
    fixed = sorted(set(range(NP)) - set(st1) - set(st2))
    if fixed:                                         # never free: bitwise the start value (zero) on every frame
        np.testing.assert_array_equal(out['pose'][:, fixed].view(np.uint64), np.zeros((F, len(fixed)), np.uint64))
    if again is not None:                             # the chain solve is deterministic, plain and cooperative: not a bit may move
        for k in OUT_KEYS:
            assert out[k].tobytes() == again[k].tobytes(), f'{name}: {k} differs between two runs'
    if plain is not None:                             # the cooperative chain against the plain chain of the same inputs
        p_out, (p_kernel, _, _) = plain
        assert ',coop' not in p_kernel, p_kernel
        ASSERTED_KERNELS.add(p_kernel)
        np.testing.assert_array_equal(out['iters'], p_out['iters'])
        for k in ('pose', 'fullpose', 'shape'):
            assert float(np.abs(out[k] - p_out[k]).max(initial=0.0)) < tol, k
        assert float(np.abs(out['trans'] - p_out['trans']).max()) < tol_t
    return kernel, lds


def check_tile_switch(capi, tier):
    """MOSHII_TM = 1, 5, 7, 15 on 15 markers and 16, 20, 27 on 81: every setting held to the oracle, and the launches' LDS sizes
    different wherever the layout lets the tile height show (see TM_CASES) -- the switch is known to have acted."""
    small = [check_case(capi, n, tier)[1] for n in TM_CASES[15]]
    large = [check_case(capi, n, tier)[1] for n in TM_CASES[81]]
    assert small[3] > max(small[:3]), small
    assert len(set(large)) == len(large) and large == sorted(large), large


def instantiation(kernel):
    """The kernel name without the cooperative group's size: k_chain_solve<5,1,xt,coop3> -> k_chain_solve<5,1,xt,coop>."""
    head, sep, _ = kernel.partition(',coop')
    return head + (',coop>' if sep else '')


# ---- the guard on the table's own inputs (CPU; `python -m tests.chain_edges [--deviations] [NAME ...]`) --------------------------------
def guard(name, noise=1e-13):
    """The oracle on observations perturbed by `noise` m Gaussian noise must keep every iteration count and move the solution by less
    than min(1/100 of the device bound, 1/10 of the emulation bound) (module docstring: why not 1/100 of the latter); the last free
    pose variable (and shape coefficient) must leave its start value by more than 1e-3 in some frame.  Returns (ok, text)."""
    c = CASES[name]
    case, _ = inputs(c)
    ref = reference(name)
    rng = np.random.default_rng(12345)
    per = run_oracle(c, case['obs'] + rng.normal(0, noise, case['obs'].shape))
    (emu, emu_t), (gpu, gpu_t) = bounds(c, 'emulation'), bounds(c, 'gpu')
    lim, lim_t = min(gpu / 100, emu / 10), min(gpu_t / 100, emu_t / 10)
    same = np.array_equal(per['iters'], ref['iters'])
    moved = float(np.abs(per['pose'] - ref['pose']).max())
    moved_t = float(np.abs(per['trans'] - ref['trans']).max())
    if c['E']:
        moved = max(moved, float(np.abs(per['shape'] - ref['shape']).max()))
    last = free_ids(c)[1][-1]
    teeth = float(np.abs(ref['pose'][:, last]).max())
    teeth_s = float(np.abs(ref['shape'][:, -1]).max()) if c['E'] else None
    ok = same and moved < lim and moved_t < lim_t and teeth > 1e-3 and (teeth_s is None or teeth_s > 1e-3)
    strict = moved < emu / 100 and moved_t < emu_t / 100
    return ok, (f'{name}: seed {c["seed"]} n {n_unknowns(c)} iters {ref["iters"].tolist()} rerun {"same" if same else per["iters"].tolist()} '
                f'moved {moved:.1e} rad {moved_t:.1e} m (limit {lim:.0e} / {lim_t:.0e}; 1/100 of the emulation bound: {"met" if strict else "not met"}) '
                f'last pose var {teeth:.2e}' + ('' if teeth_s is None else f' last shape coeff {teeth_s:.2e}') + ('' if ok else '   <-- FAILS'))


def worst_per_family(tier):
    out = {}
    for (t, name), d in DEVIATIONS.items():
        if t == tier:
            f = CASES[name]['family']
            out[f] = max(out.get(f, 0.0), d)
    return dict(sorted(out.items()))


# Worst deviation from the oracle per family: max over the family's cases of max(|pose - oracle| in rad, |shape - oracle|), and the
# case it came from; 'gpu': the hipcc build on an MI355X.
RESULTS = {
    'emulation': {'A': (5.7e-11, 'A-n79'), 'B': (4.9e-12, 'B-n16-force4'), 'C': (3.5e-11, 'C-n207'), 'D': (6.8e-11, 'D-n80-coop3'),
                  'E': (7.3e-13, 'E-M15-onepertile-coop3')},
    'gpu': {'A': (7.7e-11, 'A-n81'), 'B': (5.8e-12, 'B-n16-force4'), 'C': (6.1e-11, 'C-n207'), 'D': (7.4e-11, 'D-xt-n207-coop8'),
            'E': (1.4e-12, 'E-M15-tm5-onepertile')},
}


if __name__ == '__main__':
    import sys
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    if '--deviations' in sys.argv:
        from tests.emu.emu_moshii import emulated_libmoshii
        os.environ['HIPEMU_CONCURRENT'] = '1'
        with emulated_libmoshii() as _capi:
            for _n in args or names():
                check_case(_capi, _n, 'emulation')
        print(worst_per_family('emulation'))
    else:
        _bad = 0
        for _n in args or names():
            _ok, _txt = guard(_n)
            _bad += not _ok
            print(_txt, flush=True)
        sys.exit(1 if _bad else 0)
