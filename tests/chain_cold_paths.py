"""The Stage-II chain kernel's cold paths, which chain_solve.hip keeps out of line (rigid_init_fn with its cooperative marker gather,
column_tables_fn, vconst_fn, and at the frame head coop_lead_verdict_fn, carry_on_fn, chunk_boundary_fn, territory_request_fn): cases
and checker shared by tests/test_chain_cold_paths_emulation.py (g++ build, CPU fibers) and tests/test_gpu_chain_cold_paths.py (the
hipcc build on the device).  What can go wrong there is a moved pointer or an outlined block that reads the wrong LDS word, so the
cases make every one of those functions run:

  chains from a COLD start (first-frame schedule: the rigid branch and, cooperative, its gather of the ranks' markers), as one
  workgroup and as 3 and 6 ranks; the same with optimize_fingers, where Step 2 has another free set than Step 1, so that the column
  tables and the fixed joints' correctives are rebuilt twice a frame (8-block instantiation);
  a chunked solve with a 2-frame warm-up, so that hand-offs miss, pass-1 chains carry on, sweeps cross chunk boundaries and meet other
  chains' territories -- with MOSHII_COOP_GROUP(1) (plain repair chains), MOSHII_COOP_GROUP(3) (cooperative sweeps) and the library's default.

Bounds: tests/chain_edges.py's (emulation 1e-9 rad / 1e-10 m, device 1e-7), equal iteration counts, never-free variables bitwise
untouched; the chunked solve also against the same library's sequential chain within its verify_tol (a chunk stands if its entry state
is within verify_tol of its predecessor's end state, and a frame's solve does not move two starts apart)."""
import numpy as np

from tests import chain_edges as ce

VERIFY_TOL = 1e-9


def _c(**kw):
    c = dict(model='smplh', seed=4, M=53, F=6, dph=24, body_only=True, dropout=None, ids=None, fingers=False, E=0, G=0, env={}, vis=None)
    c.update(kw)
    return c


def chain_case(fingers, G, F):
    return _c(fingers=fingers, body_only=not fingers, G=G, F=F, dph=30 if fingers else 24)   # (30 coefficients per hand: 3 + 63 + 60 unknowns in Step 2, 8 blocks)


CHAIN_PARAMS = [(False, 0), (False, 3), (False, 6), (True, 0), (True, 3), (True, 6)]   # (optimize_fingers, ranks; 0: one workgroup)
_REF = {}


def reference(c):
    """The oracle's chain for the case's inputs (computed once per set of inputs)."""
    key = (c['fingers'], c['F'], c['seed'])
    if key not in _REF:
        _REF[key] = ce.run_oracle(c)
    return _REF[key]


def held_to_oracle(out, c, tier, what):
    ref = reference(c)
    tol, tol_t = ce.bounds(c, tier)
    F, NP = out['pose'].shape
    solved = ref['frame_ids']
    assert out['status'].tolist() == [0 if t in set(solved.tolist()) else 1 for t in range(F)], what
    dp = float(np.abs(out['pose'][solved] - ref['pose']).max())
    dt = float(np.abs(out['trans'][solved] - ref['trans']).max())
    print(f'{what}: iters {out["iters"][:, 0].tolist()} oracle {ref["iters"].tolist()} max|dpose| {dp:.2e} |dtrans| {dt:.2e} (bound {tol:.0e} / {tol_t:.0e})')
    np.testing.assert_array_equal(out['iters'][solved, 0], ref['iters'], err_msg=what)
    assert dp < tol and dt < tol_t, (what, dp, dt)
    assert float(np.abs(out['fullpose'][solved] - ref['fullpose']).max()) < tol, what
    for key, col in ce.ERR_COLS:                      # the error columns, as chain_edges.check_case holds them
        if key in ref['errs']:
            r = ref['errs'][key]                      # (the velocity term: the frames that have one -- the last ones)
            np.testing.assert_allclose(out['errs'][solved[len(solved) - len(r):], col], r, rtol=1e-6, atol=1e-12 if key == 'velo' else 0.0,
                                       err_msg=f'{what}: {key}')
    st1, st2 = ce.free_ids(c)
    fixed = sorted(set(range(NP)) - set(st1) - set(st2))
    if fixed:
        np.testing.assert_array_equal(out['pose'][:, fixed].view(np.uint64), np.zeros((F, len(fixed)), np.uint64), err_msg=what)


def device(c):
    from tests.helpers import device_case
    case, vis = ce.inputs(c)
    return case, vis, device_case(case, optimize_fingers=c['fingers'])


def check_chain(capi, fingers, G, F, tier):
    """One chain from a cold start; returns the kernel's name."""
    c = chain_case(fingers, G, F)
    case, vis, dev = device(c)
    ch = [dict(attach=dev['attach'], obs=case['obs'], vis=vis, first=True)]
    out = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], ch, coop=G or 1)[0]
    kernel = capi.last_launch_info()[0]
    held_to_oracle(out, c, tier, f'fingers={fingers} G={G} {kernel}')
    if tier == 'gpu':   # the chain solve is deterministic: not a bit may move between two runs
        again = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], ch, coop=G or 1)[0]
        for k in ce.OUT_KEYS:
            assert out[k].tobytes() == again[k].tobytes(), f'{k} differs between two runs'
    return kernel


def check_chunked(capi, coop, F, num_chunks, tier):
    """coop = 1: plain repair chains (chunk_boundary_fn, territory_request_fn; carry_on_fn in pass 1); coop = 3: repair rounds of
    three-rank sweeps (coop_lead_verdict_fn); coop = 0: the library's own choice of the two.  The repair launches are the last ones of
    the call: their kernel's name says which ran."""
    c = _c(F=F, body_only=True)
    case, vis, dev = device(c)
    seq = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], [dict(attach=dev['attach'], obs=case['obs'], vis=vis, first=True)], coop=1)[0]
    outs, rep = capi.sequence_solve_host(dev['model'], dev['prior'], dev['opts'], [dict(attach=dev['attach'], obs=case['obs'], vis=vis)],
                                         num_chunks=num_chunks, warmup=2, verify_tol=VERIFY_TOL, coop=coop)
    out = outs[0]
    kernel = capi.last_launch_info()[0]
    print(rep, kernel)
    assert rep['n_chunks'] == num_chunks
    # (a 2-frame warm-up from a cold start does not reach the sequential state: chunks were repaired, by launches of their own when cooperative)
    assert rep['n_repaired'] >= 1, rep
    if coop == 1:
        assert kernel == 'k_chain_solve<4,1>', kernel
    elif coop >= 2:
        assert rep['repair_rounds'] >= 1 and kernel == f'k_chain_solve<4,1,coop{coop}>', (rep, kernel)
    else:   # (the library's choice: plain chains in the emulated build and where the groups would not all be resident)
        assert kernel == 'k_chain_solve<4,1>' or kernel.startswith('k_chain_solve<4,1,coop'), kernel
    held_to_oracle(out, c, tier, f'chunked coop={coop}')
    np.testing.assert_array_equal(out['status'], seq['status'])
    np.testing.assert_array_equal(out['iters'], seq['iters'])
    dv = max(float(np.abs(out['pose'] - seq['pose']).max()), float(np.abs(out['trans'] - seq['trans']).max()))
    print(f'chunked coop={coop}: max deviation from the sequential chain {dv:.2e} (verify_tol {VERIFY_TOL:.0e})')
    assert dv <= VERIFY_TOL, dv
