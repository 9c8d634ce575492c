"""GPU: Stage-II of the SMAL animal types through the C ABI on the device, against the animal oracle (tests/animal_oracle.py):
one-workgroup and cooperative chains, the chunked sequence solve, the drop-in mosh_stageii and the full-mesh export."""
import os

import numpy as np
import pytest

from oracle import stageii_oracle as so
from tests import animal_oracle as ao
from tests import parity_envelope as pe

pytestmark = pytest.mark.gpu

ANIMALS = ('animal_horse', 'animal_dog')


def _solve(capi, dev, case, coop):
    return capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'],
                                 [dict(attach=dev['attach'], obs=case['obs'], vis=case['vis'], first=True)], coop=coop)[0]


def _oracle_with_spread(case, model_type, k=2):
    """The oracle's trajectory and its spread: the largest per-frame state difference of k runs on observations perturbed by 1e-13 m
    (tests/parity_envelope.py: where that spread exceeds WELL the reference's own algorithm sits on a knife edge)."""
    runs = []
    for i in range(k + 1):
        obs = case['obs'] + (0.0 if i == 0 else np.random.default_rng(100 + i).normal(0, 1e-13, case['obs'].shape))
        runs.append(ao.animal_chain(case['m'], case['prior'], case['closest'], case['coef'], obs, case['vis'], model_type))
    spread = np.zeros(len(runs[0]['frame_ids']))
    for r in runs[1:]:
        spread = np.maximum(spread, np.maximum(np.abs(r['pose'] - runs[0]['pose']).max(1), np.abs(r['trans'] - runs[0]['trans']).max(1)))
    runs[0]['perturbed_marker_rmse'] = max(_marker_rmse(r['markers_sim'], runs[0]['markers_sim']) for r in runs[1:])
    return runs[0], pe.dilated(spread)


def _marker_rmse(a, b):
    return float(np.sqrt(np.concatenate([((x - y) ** 2).sum(-1) for x, y in zip(a, b)]).mean()))


def _judge(dev, d):
    """parity_envelope's criterion on a per-frame deviation: -> (frames outside it, well-conditioned frames that did not part)."""
    outside, parted = pe._judge(dev, d, pe._stretch_max(d))
    return outside, (d <= pe.WELL) & ~parted


@pytest.mark.parametrize('model_type', ANIMALS)
def test_animal_chain_matches_oracle_on_device(gpu_lib, model_type):
    """200 frames with dropouts and gaps, held as tests/parity_envelope.py holds the human configs: on well-conditioned frames pose
    <= 1e-7 rad, the same dogleg iteration counts, markers <= 1e-6 m RMSE and the poseB / poseB_jangles SSE; the cooperative chain
    (4 workgroups) against one workgroup to 1e-9 there.  (The synthetic dog frees its ears, jaw and tail tip, which few markers see:
    its oracle parts from itself under 1e-13 m perturbations on long stretches; the horse is well conditioned throughout.)"""
    from moshpp_amd import capi
    case = ao.animal_case(model_type, F=200, M=40, seed=11)
    dev = ao.animal_device_case(case)
    out = _solve(capi, dev, case, coop=1)
    coop = _solve(capi, dev, case, coop=4)
    assert capi.last_launch_info()[0].endswith(',coop4>'), capi.last_launch_info()
    ref, d = _oracle_with_spread(case, model_type)
    solved = np.flatnonzero(out['status'] == 0)
    assert list(solved) == list(ref['frame_ids'])
    dev_ = np.maximum(np.abs(out['pose'][solved] - ref['pose']).max(1), np.abs(out['trans'][solved] - ref['trans']).max(1))
    outside, well = _judge(dev_, d)
    assert not outside.any(), np.flatnonzero(outside)[:10]
    if model_type == 'animal_horse':
        assert well.all()
    assert not well.any() or dev_[well].max() < 1e-7
    # the north star over every frame, parted ones included -- or, where the oracle's own perturbed runs land on other local solutions
    # further apart than that (the dog), no further from the oracle than twice their distance
    rmse = _marker_rmse([out['markers_sim'][f][case['vis'][f]] for f in solved], ref['markers_sim'])
    assert rmse <= max(pe.MARKER_TOL, 2.0 * ref['perturbed_marker_rmse']), (rmse, ref['perturbed_marker_rmse'])
    np.testing.assert_array_equal(out['iters'][solved, 0][well], ref['iters'][well])
    for i, f in enumerate(solved):
        if well[i]:
            v = case['vis'][f]
            assert np.sqrt(np.mean((out['markers_sim'][f][v] - ref['markers_sim'][i]) ** 2)) < 1e-6
    np.testing.assert_allclose(out['errs'][solved, 1][well], ref['errs']['poseB'][well], rtol=1e-6)
    if model_type == 'animal_horse':
        np.testing.assert_allclose(out['errs'][solved, 7], ref['errs']['poseB_jangles'], rtol=1e-6)
    dc = np.maximum(np.abs(coop['pose'][solved] - out['pose'][solved]).max(1), np.abs(coop['trans'][solved] - out['trans'][solved]).max(1))
    outside, well_c = _judge(dc, d)
    assert not outside.any()
    assert not well_c.any() or dc[well_c].max() < 1e-9
    np.testing.assert_array_equal(coop['iters'][solved][well_c], out['iters'][solved][well_c])


@pytest.mark.parametrize('model_type', ANIMALS)
def test_animal_chunked_equals_sequential_on_device(gpu_lib, model_type):
    from moshpp_amd import capi
    case = ao.animal_case(model_type, F=400, M=40, seed=12)
    dev = ao.animal_device_case(case)
    seq = _solve(capi, dev, case, coop=1)
    outs, report = capi.sequence_solve_host(dev['model'], dev['prior'], dev['opts'],
                                            [dict(attach=dev['attach'], obs=case['obs'], vis=case['vis'])], verify_tol=1e-9)
    assert report['n_chunks'] > 1
    np.testing.assert_array_equal(outs[0]['status'], seq['status'])
    if model_type == 'animal_horse':
        assert np.abs(outs[0]['fullpose'] - seq['fullpose']).max() < pe.TIGHT   # (hand-offs verified to 1e-9, as the human chunked tests hold them)
    else:   # the chunks' repair sweeps are cooperative chains: round-off apart from the one-workgroup chain, judged on the oracle's spread
        _, d = _oracle_with_spread(case, model_type)
        ok = np.flatnonzero(seq['status'] == 0)
        dev = np.maximum(np.abs(outs[0]['pose'][ok] - seq['pose'][ok]).max(1), np.abs(outs[0]['trans'][ok] - seq['trans'][ok]).max(1))
        outside, well = _judge(dev, d)
        assert not outside.any() and (not well.any() or dev[well].max() < pe.TIGHT)


@pytest.mark.parametrize('model_type', ANIMALS)
def test_animal_full_mesh_export_on_device(gpu_lib, model_type):
    case = ao.animal_case(model_type, F=2, M=40, seed=6)
    rng = np.random.default_rng(3)
    F = 37
    pose = rng.normal(0, 0.3, (F, case['m']['NP']))
    trans = rng.normal(0, 1, (F, 3))
    dev = ao.animal_device_case(case)
    got64 = dev['model'].lbs_forward(pose, trans)
    got32 = dev['model'].lbs_forward(pose, trans, dtype=np.float32)
    m = case['m']
    for f in range(F):
        ref = so.verts_forward(m, so.fullpose_from_pose(m, pose[f]), trans[f])
        assert np.abs(got64[f] - ref).max() < 1e-9
        assert np.abs(got32[f] - ref).max() < 2e-5


def test_mosh_stageii_horse_end_to_end(gpu_lib, tmp_path):
    """cfg surface_model.type = animal_horse on files: the output layout and the reference's stageii_errs keys, poseB_jangles included."""
    import pickle
    from moshpp_amd.cfg import make_cfg
    from moshpp_amd.chmosh import mosh_stageii
    from moshpp_amd.mocap_interface import MocapSession, write_mocap_c3d
    case = ao.animal_case('animal_horse', F=12, M=40, seed=13)
    s = case['s']
    raw = {k: v for k, v in s['model'].items() if not k.startswith('_') and k != 'model_type'}
    with open(tmp_path / 'horse.pkl', 'wb') as f:
        pickle.dump(raw, f)
    with open(tmp_path / 'horse_prior.pkl', 'wb') as f:
        pickle.dump(s['animal_prior'], f)
    c3d = str(tmp_path / 'ds' / 'horse' / 'walk01.c3d')
    os.makedirs(os.path.dirname(c3d))
    write_mocap_c3d(s['markers'], list(s['labels']), c3d, frame_rate=120)
    cfg = make_cfg(**{'mocap.fname': c3d, 'surface_model.type': 'animal_horse', 'surface_model.fname': str(tmp_path / 'horse.pkl'),
                      'moshpp.pose_body_prior_fname': str(tmp_path / 'horse_prior.pkl'),
                      'opt_settings.weights_type': 'smplh'})   # (the reference yaml has no weights table of its own for the animals)
    out = mosh_stageii(c3d, cfg, s['markers_latent'], s['latent_labels'], s['betas'], s['marker_meta'])
    dd = out['stageii_debug_details']
    assert list(dd['stageii_errs']) == ['data', 'poseB', 'poseB_jangles', 'velo']
    assert out['fullpose'].shape == (12, 108)
    ms = MocapSession(c3d, 'mm')
    obs, vis = ms.markers_aslabeled_arrays(s['latent_labels'])
    ref = ao.animal_chain(case['m'], case['prior'], case['closest'], case['coef'], obs, vis, 'animal_horse')
    assert np.abs(out['fullpose'] - ref['fullpose']).max() < 1e-7
    np.testing.assert_allclose(dd['stageii_errs']['poseB_jangles'], ref['errs']['poseB_jangles'], rtol=1e-6)


@pytest.mark.parametrize('model_type', ANIMALS)
def test_short_animal_chain_matches_oracle_tightly_on_device(gpu_lib, model_type):
    """A few frames, before the synthetic dog's long ill-conditioned stretches begin: no envelope -- every frame <= 1e-7 rad, the same
    iteration counts, the prior SSE per frame (the long test above can only hold the dog to the envelope)."""
    from moshpp_amd import capi
    case = ao.animal_case(model_type, F=4, M=40, seed=1)
    dev = ao.animal_device_case(case)
    ref = ao.animal_chain(case['m'], case['prior'], case['closest'], case['coef'], case['obs'], case['vis'], model_type)
    for coop in (1, 4):
        out = _solve(capi, dev, case, coop=coop)
        solved = np.flatnonzero(out['status'] == 0)
        assert list(solved) == list(ref['frame_ids'])
        assert np.abs(out['pose'][solved] - ref['pose']).max() < 1e-7 and np.abs(out['trans'][solved] - ref['trans']).max() < 1e-7
        np.testing.assert_array_equal(out['iters'][solved, 0], ref['iters'])
        np.testing.assert_allclose(out['errs'][solved, 1], ref['errs']['poseB'], rtol=1e-6)


@pytest.mark.parametrize('name', ['horse', 'horse_toes', 'horse_dropouts', 'dog'])
def test_animal_chain_matches_executed_reference_on_device(gpu_lib, name):
    """The device against the reference's own mosh_stageii executed on the same inputs (tests/golden/ref_stageii_animal.npz)."""
    from moshpp_amd import capi
    from tests import test_animal_ref_golden as rg
    g = rg._load()
    case, toes = rg._case(g, name)
    dev = ao.animal_device_case(case, optimize_toes=toes)
    out = _solve(capi, dev, case, coop=1)
    solved = np.flatnonzero(out['status'] == 0)
    fp = g[f'{name}_fullpose']
    assert np.abs(out['fullpose'][solved] - fp).max() <= rg.BAR[rg.CASES[name]]
    np.testing.assert_array_equal(out['iters'][solved, 0], rg._iters_per_frame(g[f'{name}_minimize_calls'], len(fp)))
    if rg.CASES[name] == 'animal_horse':
        np.testing.assert_allclose(out['errs'][solved, 7], g[f'{name}_err_poseB_jangles'], rtol=1e-6)
