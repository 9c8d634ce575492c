"""The hipcc build of the assembly's re-ordered prologue and of the normal-equation exchange that leaves out the own slot and a
marker-less prior rank's zeros (chain_solve.hip: assemble; CPU twin: tests/test_chain_serial_path_emulation.py): 24 frames of the SMPL-H
body with 53 markers, cooperative against one-workgroup chain.  Group sizes: 3 (the smallest whose prior rank owns no markers), 6 (what
the library picks for this problem) and 2 (the prior rank has markers: every slot's accumulators count).  Tolerance and criteria of
tests/test_gpu_fullsize.py's cooperative / one-workgroup comparisons."""
import numpy as np
import pytest

F = 24
KEYS = ('pose', 'fullpose', 'trans', 'markers_sim', 'errs', 'iters', 'status')


@pytest.fixture(scope='module')
def problem(gpu_lib):
    from moshpp_amd import capi, workload
    job = workload.make_job('smplh', F, 53, seed=2024)
    solver = workload.make_solver(job)
    ch = [dict(attach=solver.attach, obs=job['obs'], vis=job['vis'], first=True)]
    plain = capi.chain_solve_host(solver.dev, solver.prior, solver.opts, ch, coop=1)[0]
    assert capi.last_launch_info()[0] == 'k_chain_solve<4,1>'
    return dict(solver=solver, ch=ch, plain=plain)


def _coop(problem, G):
    from moshpp_amd import capi
    s = problem['solver']
    out = capi.chain_solve_host(s.dev, s.prior, s.opts, problem['ch'], coop=G)[0]
    assert capi.last_launch_info()[0] == f'k_chain_solve<4,1,coop{G}>', capi.last_launch_info()
    return out


def _hold_to_plain(out, plain):
    assert np.array_equal(out['iters'], plain['iters']) and np.array_equal(out['status'], plain['status'])
    dp, dt = np.abs(out['fullpose'] - plain['fullpose']).max(), np.abs(out['trans'] - plain['trans']).max()
    print(f'cooperative vs one-workgroup: max|dfullpose| {dp:.2e} rad, max|dtrans| {dt:.2e} m')
    assert dp < 1e-8 and dt < 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize('G', [3, 6, 2])
def test_cooperative_chain_equals_one_workgroup_chain_and_repeats_bit_for_bit(problem, G):
    out = _coop(problem, G)
    again = _coop(problem, G)
    for k in KEYS:
        np.testing.assert_array_equal(again[k], out[k], err_msg=k)
    _hold_to_plain(out, problem['plain'])


@pytest.mark.gpu
def test_cooperative_chain_with_skewed_arrivals_moves_no_bit(problem, monkeypatch):
    """MOSHII_COOP_SKEW: every rank held back a pseudo-random 0 .. 10 us before each exchange."""
    out = _coop(problem, 6)
    monkeypatch.setenv('MOSHII_COOP_SKEW', '5')
    skewed = _coop(problem, 6)
    monkeypatch.delenv('MOSHII_COOP_SKEW')
    for k in KEYS:
        np.testing.assert_array_equal(skewed[k], out[k], err_msg=k)
    _hold_to_plain(skewed, problem['plain'])
