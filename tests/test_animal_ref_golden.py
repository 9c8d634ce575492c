"""CPU: the animal Stage-II path pinned to the reference's own mosh_stageii EXECUTED on SMAL-sized quadrupeds
(tests/golden/ref_stageii_animal.npz, made by tests/golden/make_ref_stageii_animal_golden.py with the reference's load_moshpp_models,
smal_horse_prior, smal_horse_joint_angle_prior and MaxMixtureDog): the animal oracle and the product's kernels in CPU emulation are
held to the recorded trajectories, and the host's dog prior constants to MaxMixtureDog.get_gmm_prior's."""
import os

import numpy as np
import pytest

from moshpp_amd import prior as mprior, synth
from tests import animal_oracle as ao
from tests.emu.emu_moshii import emulated_libmoshii

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_stageii_animal.npz')
CASES = {'horse': 'animal_horse', 'horse_toes': 'animal_horse', 'horse_dropouts': 'animal_horse', 'dog': 'animal_dog'}
# fullpose bars (rad).  Every solve takes the reference's dogleg iteration count and every error term agrees to 1e-6 relative, but the
# states agree to 2e-8 (horse) / 3e-7 (dog) rather than the 5e-9 of the human cases -- with the analytic Jacobian and with the
# fixture's own central-difference one alike (AnimalObjectiveFD), so the Jacobian is not the cause; not yet explained.
BAR = {'animal_horse': 3e-8, 'animal_dog': 1e-6}


def _load():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


def _case(g, name):
    a = g[f'{name}_args']
    F, M, seed, V, toes, drop = (int(x) for x in a[:6])
    return ao.animal_ref_case(CASES[name], F, M, seed, V, empty_frames=tuple(int(x) for x in a[6:]), dropout=drop / 100.0), bool(toes)


def _iters_per_frame(calls, n_frames):
    """dogleg iterations per solved frame from the reference's ch.minimize calls: five on the first frame (three rounds, Step 1, Step 2),
    two on every later one"""
    it = calls[:, 2]
    return np.array([it[:5].sum()] + [it[5 + 2 * i:7 + 2 * i].sum() for i in range(n_frames - 1)])


@pytest.mark.parametrize('name', list(CASES))
def test_animal_oracle_matches_executed_reference(name):
    g = _load()
    case, toes = _case(g, name)
    mt = CASES[name]
    ref = ao.animal_chain(case['m'], case['prior'], case['closest'], case['coef'], case['obs'], case['vis'], mt, optimize_toes=toes)
    fp = g[f'{name}_fullpose']
    assert ref['fullpose'].shape == fp.shape
    assert np.abs(ref['fullpose'] - fp).max() <= BAR[mt]
    assert np.abs(ref['trans'] - g[f'{name}_trans']).max() <= BAR[mt]
    np.testing.assert_array_equal(ref['iters'], _iters_per_frame(g[f'{name}_minimize_calls'], len(fp)))
    assert list(ref['errs']) == list(g[f'{name}_err_keys'])
    for k in ref['errs']:
        np.testing.assert_allclose(ref['errs'][k], g[f'{name}_err_{k}'], rtol=1e-6, err_msg=k)
    assert ('poseB_jangles' in ref['errs']) == (mt == 'animal_horse')
    if name == 'horse_dropouts':
        assert not case['vis'].all() and (~case['vis'].any(1)).any()   # annealed weights and an empty frame


@pytest.mark.parametrize('name', ['horse', 'horse_toes', 'dog'])
def test_chain_kernel_matches_executed_reference_in_emulation(name):
    g = _load()
    case, toes = _case(g, name)
    with emulated_libmoshii() as capi:
        dev = ao.animal_device_case(case, optimize_toes=toes)
        out = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'],
                                    [dict(attach=dev['attach'], obs=case['obs'], vis=case['vis'], first=True)], coop=1)[0]
    solved = np.flatnonzero(out['status'] == 0)
    fp = g[f'{name}_fullpose']
    assert np.abs(out['fullpose'][solved] - fp).max() <= BAR[CASES[name]]
    np.testing.assert_array_equal(out['iters'][solved, 0], _iters_per_frame(g[f'{name}_minimize_calls'], len(fp)))
    np.testing.assert_allclose(out['errs'][solved, 1], g[f'{name}_err_poseB'], rtol=1e-6)
    if CASES[name] == 'animal_horse':
        np.testing.assert_allclose(out['errs'][solved, 7], g[f'{name}_err_poseB_jangles'], rtol=1e-6)


def test_dog_prior_constants_equal_max_mixture_dog_as_executed():
    g = _load()
    seed = int(g['dog_args'][2])
    got = mprior.create_dog_gmm_prior(synth.synth_dog_prior(seed))
    np.testing.assert_allclose(got['means'], g['dog_prior_means'], rtol=0, atol=0)
    np.testing.assert_allclose(got['chols'], g['dog_prior_chols'], rtol=1e-12, atol=1e-12 * np.abs(g['dog_prior_chols']).max())
    np.testing.assert_allclose(got['weights'], np.ravel(g['dog_prior_weights']), rtol=1e-12)
