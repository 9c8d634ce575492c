"""CPU: Stage-II for the SMAL animal types (animal_horse, animal_dog): loader, free-variable sets, the host's prior constants, and the
product's chain kernels in CPU emulation (tests/emu: the .hip sources compiled unchanged) against the animal oracle
(tests/animal_oracle.py) -- one workgroup, a cooperative chain, a chunked sequence -- plus the full-mesh export of both models."""
import pickle

import numpy as np
import pytest

from moshpp_amd import chmosh, models, prior as mprior, synth
from oracle import stageii_oracle as so
from tests import animal_oracle as ao
from tests.emu.emu_moshii import emulated_libmoshii

ANIMALS = ('animal_horse', 'animal_dog')


@pytest.mark.parametrize('model_type', ANIMALS)
def test_synthetic_animal_pickles_load_and_the_type_is_detected_from_posedirs(tmp_path, model_type):
    dd = synth.synth_model(model_type, seed=3)
    keep = {k: v for k, v in dd.items() if not k.startswith('_') and k != 'model_type'}
    fn = tmp_path / f'{model_type}.pkl'
    with open(fn, 'wb') as fh:
        pickle.dump(keep, fh)
    sm = models.load_surface_model(str(fn))
    V, K = synth.MODEL_DIMS[model_type]
    assert sm.model_type == model_type and sm.V == V == 3889 and sm.K == K
    assert sm.NP == 3 * K == {'animal_horse': 108, 'animal_dog': 105}[model_type]
    assert sm.posedirs.shape[2] == {'animal_horse': 315, 'animal_dog': 306}[model_type]
    assert sm.hand_dof == 0 and list(sm.parents) == list(synth.kintree_parents(model_type))


@pytest.mark.parametrize('toes', [False, True])
def test_stageii_pose_ids_of_the_animals_are_the_references(toes):
    horse = chmosh.stageii_pose_ids('animal_horse', 108, False, toes)
    assert horse['body'] == list(range(3, 84)) and horse['finger'] == [] and horse['face'] == []
    dog = chmosh.stageii_pose_ids('animal_dog', 105, False, toes)
    joints = [1, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 30, 31, 32, 33, 34]
    assert dog['body'] == list(np.arange(105).reshape(-1, 3)[joints].reshape(-1)) and len(dog['body']) == 93
    for ids, nb in ((horse, 81), (dog, 93)):
        want = sorted(set([0, 1, 2] + ids['body']) - (set() if toes else set(range(30, 36))))   # the toe quirk (:645-647)
        assert ids['step1'] == want and ids['step2'] == want
        assert 3 + len(ids['step1']) == (3 + 3 + nb if toes else 3 + 3 + nb - 6)


def test_horse_prior_factor_reproduces_the_references_value_and_gradient():
    """L = chol(2 P P^T), w = 1: |sqrt(1/2) L^T (x - mu)|^2 - log 1 = |(x - mu) . P|^2, gradient and J^T J the same."""
    pkl = synth.synth_horse_prior(seed=5)
    p = mprior.smal_horse_prior(pkl)
    assert p['npose'] == 81 and p['chols'].shape == (1, 81, 81) and np.all(np.triu(p['chols'][0], 1) == 0.0)
    np.testing.assert_array_equal(p['weights'], [1.0])
    P, mu = np.asarray(pkl['pic'])[:81, :81], np.asarray(pkl['mean_pose'])[:81]
    rng = np.random.default_rng(0)
    for _ in range(5):
        x = mu + rng.normal(0, 0.3, 81)
        r_ref = (x - mu).dot(P)
        r, k, Jp = so.gmm_prior_eval(p, x, want_jac=True)
        assert k == 0 and r[-1] == 0.0
        v_ref, v = r_ref.dot(r_ref), r.dot(r)
        assert abs(v - v_ref) <= 1e-12 * v_ref
        g_ref, g = 2 * P.dot(r_ref), 2 * Jp.T.dot(r)
        assert np.abs(g - g_ref).max() <= 1e-12 * np.abs(g_ref).max()
        assert np.abs(Jp.T.dot(Jp) - P.dot(P.T)).max() <= 1e-12 * np.abs(P.dot(P.T)).max()


def test_dog_prior_constants_equal_the_oracles_restatement():
    """Host against the oracle's restatement; against MaxMixtureDog as executed: tests/test_animal_ref_golden.py."""
    pkl = synth.synth_dog_prior(seed=2)
    got = mprior.create_dog_gmm_prior(pkl)
    want = ao.dog_prior_prepared(pkl)
    assert got['npose'] == 93
    for k in ('means', 'chols', 'weights'):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    bad = dict(pkl, gmm_covs=np.array(pkl['gmm_covs']))
    bad['gmm_covs'][1][:, 3] = 0.0
    bad['gmm_covs'][1][3, :] = 0.0
    with pytest.raises(ValueError, match='determinant'):
        mprior.create_dog_gmm_prior(bad)


def test_create_body_prior_picks_the_prior_by_type():
    assert mprior.create_body_prior('animal_horse', synth.synth_horse_prior(0))['npose'] == 81
    assert mprior.create_body_prior('animal_dog', synth.synth_dog_prior(0))['npose'] == 93
    assert mprior.create_body_prior('mano', None) is None


def test_stagei_refuses_animals():
    class Node(dict):
        __getattr__ = dict.__getitem__
    cfg = Node(surface_model=Node(type='animal_horse'))
    with pytest.raises(NotImplementedError, match='Stage-II'):
        chmosh.mosh_stagei([], cfg)


def _check_against_oracle(out, ref, horse, tol=1e-9):
    solved = np.flatnonzero(out['status'] == 0)
    assert list(solved) == list(ref['frame_ids'])
    assert np.abs(out['fullpose'][solved] - ref['fullpose']).max() < tol
    assert np.abs(out['trans'][solved] - ref['trans']).max() < tol
    np.testing.assert_array_equal(out['iters'][solved, 0], ref['iters'])
    np.testing.assert_allclose(out['errs'][solved, 1], ref['errs']['poseB'], rtol=1e-9)
    if horse:
        np.testing.assert_allclose(out['errs'][solved, 7], ref['errs']['poseB_jangles'], rtol=1e-9)
    else:
        assert np.all(out['errs'][:, 7] == 0.0)


@pytest.mark.parametrize('model_type,toes', [('animal_horse', False), ('animal_horse', True), ('animal_dog', False)])
def test_chain_kernel_matches_animal_oracle_in_emulation(model_type, toes):
    case = ao.animal_case(model_type, F=4, M=40, seed=1)
    with emulated_libmoshii() as capi:
        dev = ao.animal_device_case(case, optimize_toes=toes)
        out = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'],
                                    [dict(attach=dev['attach'], obs=case['obs'], vis=case['vis'], first=True)], coop=1)[0]
        assert ',coop' not in capi.last_launch_info()[0]
    ref = ao.animal_chain(case['m'], case['prior'], case['closest'], case['coef'], case['obs'], case['vis'], model_type, optimize_toes=toes)
    assert not np.all(case['vis'])          # dropouts: annealed weights
    _check_against_oracle(out, ref, model_type == 'animal_horse')


@pytest.mark.parametrize('model_type,G', [('animal_horse', 3), ('animal_dog', 4)])
def test_cooperative_chain_matches_animal_oracle_in_emulation(monkeypatch, model_type, G):
    monkeypatch.setenv('HIPEMU_CONCURRENT', '1')
    case = ao.animal_case(model_type, F=3, M=40, seed=4)
    with emulated_libmoshii() as capi:
        dev = ao.animal_device_case(case)
        out = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'],
                                    [dict(attach=dev['attach'], obs=case['obs'], vis=case['vis'], first=True)], coop=G)[0]
        assert capi.last_launch_info()[0].endswith(f',coop{G}>'), capi.last_launch_info()
    ref = ao.animal_chain(case['m'], case['prior'], case['closest'], case['coef'], case['obs'], case['vis'], model_type)
    _check_against_oracle(out, ref, model_type == 'animal_horse')


@pytest.mark.parametrize('model_type', ANIMALS)
def test_chunked_sequence_solve_matches_animal_oracle_in_emulation(model_type):
    case = ao.animal_case(model_type, F=16, M=40, seed=2)
    with emulated_libmoshii() as capi:
        dev = ao.animal_device_case(case)
        outs, report = capi.sequence_solve_host(dev['model'], dev['prior'], dev['opts'],
                                                [dict(attach=dev['attach'], obs=case['obs'], vis=case['vis'])],
                                                num_chunks=3, warmup=4, verify_tol=1e-9)
    assert report['n_chunks'] == 3
    ref = ao.animal_chain(case['m'], case['prior'], case['closest'], case['coef'], case['obs'], case['vis'], model_type)
    out = outs[0]
    _check_against_oracle(out, ref, model_type == 'animal_horse')


@pytest.mark.parametrize('model_type', ANIMALS)
def test_full_mesh_export_of_the_animals_equals_the_oracle_in_emulation(model_type):
    case = ao.animal_case(model_type, F=2, M=40, seed=6)
    rng = np.random.default_rng(9)
    F = 5
    pose = rng.normal(0, 0.3, (F, case['m']['NP']))
    trans = rng.normal(0, 1, (F, 3))
    with emulated_libmoshii():
        dev = ao.animal_device_case(case)
        got64 = dev['model'].lbs_forward(pose, trans)
        got32 = dev['model'].lbs_forward(pose, trans, dtype=np.float32)
    m = case['m']
    for f in range(F):
        ref = so.verts_forward(m, so.fullpose_from_pose(m, pose[f]), trans[f])
        assert np.abs(got64[f] - ref).max() < 1e-10
        assert np.abs(got32[f] - ref).max() < 2e-5
