"""The assembly's re-ordered prologue (per-joint chain on wavefront 0 beside T0 of the first tile) and the normal-equation exchange that
leaves out the own slot and a marker-less prior rank's zeros (chain_solve.hip: assemble), on the CPU fiber emulation: six frames of the
SMPL-H body, the first one with its five phases, one frame with a marker invisible.  As a one-workgroup chain and as cooperative chains
of three ranks (the smallest group whose prior rank owns no markers) and six.  Held to what tests/test_chain_emulation.py holds its
chains to; two cooperative runs must agree bit for bit."""
import numpy as np
import pytest

from oracle import stageii_oracle as so
from tests.emu.emu_moshii import emulated_libmoshii
from tests.helpers import device_case, oracle_case

F = 6
KEYS = ('pose', 'fullpose', 'trans', 'markers_sim', 'errs', 'iters', 'status')


@pytest.fixture(scope='module')
def case():
    c = oracle_case('smplh', F=F, M=53, seed=11, body_only_markers=True, dropout=0.0, n_gaps=0)
    vis = c['vis'].copy()
    assert vis.all()
    vis[3, 17] = False            # one frame with a marker invisible; the first frame (five phases) sees every marker
    obs = np.where(vis[..., None], c['obs'], 0.0)
    c = dict(c, vis=vis, obs=obs)
    c['ref'] = so.stageii_chain(c['m'], c['prior'], c['closest'], c['coef'], obs, vis, 'smplh')
    return c


def _hold_to_oracle(out, ref):
    solved = np.flatnonzero(out['status'] == 0)
    assert list(solved) == list(ref['frame_ids']) and len(solved) == F
    assert np.abs(out['fullpose'][solved] - ref['fullpose']).max() < 1e-9 and np.abs(out['trans'][solved] - ref['trans']).max() < 1e-10
    np.testing.assert_array_equal(out['iters'][solved, 0], ref['iters'])


def test_one_workgroup_chain_matches_oracle_in_emulation(case):
    with emulated_libmoshii() as capi:
        dev = device_case(case)
        out = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'],
                                    [dict(attach=dev['attach'], obs=case['obs'], vis=case['vis'], first=True)], coop=1)[0]
        assert capi.last_launch_info()[0] == 'k_chain_solve<4,1>'
    _hold_to_oracle(out, case['ref'])


@pytest.mark.parametrize('G', [3, 6])
def test_cooperative_chain_matches_oracle_and_repeats_bit_for_bit_in_emulation(monkeypatch, case, G):
    monkeypatch.setenv('HIPEMU_CONCURRENT', '1')
    with emulated_libmoshii() as capi:
        dev = device_case(case)
        ch = [dict(attach=dev['attach'], obs=case['obs'], vis=case['vis'], first=True)]
        plain = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], ch, coop=1)[0]
        out = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], ch, coop=G)[0]
        assert capi.last_launch_info()[0] == f'k_chain_solve<4,1,coop{G}>'
        again = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], ch, coop=G)[0]
    for k in KEYS:
        np.testing.assert_array_equal(again[k], out[k], err_msg=k)
    _hold_to_oracle(out, case['ref'])
    np.testing.assert_array_equal(out['iters'], plain['iters'])
    np.testing.assert_array_equal(out['status'], plain['status'])
    for k in ('pose', 'fullpose', 'trans', 'markers_sim'):
        assert np.abs(out[k] - plain[k]).max() < 1e-9, k
