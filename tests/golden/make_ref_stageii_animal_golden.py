"""Generates tests/golden/ref_stageii_animal.npz by EXECUTING the reference's own `mosh_stageii` (chmosh.py:458-741, function source
taken from the file, unmodified) on seeded synthetic SMAL-sized quadrupeds, with the reference code it drives for the animal types:
load_moshpp_models (bodymodel_loader.py:121-131), smal_horse_prior / smal_horse_joint_angle_prior (prior/horse_body_prior.py) and
MaxMixtureDog (prior/dog_body_prior.py) over MaxMixtureComplete (prior/gmm_prior_ch.py).

It reuses the lazy chumpy stand-in, the stand-ins for the other absent modules and the loader of make_ref_stageii_golden.py (imported,
not edited), adding the two chumpy functions the animal priors use: ch.exp and ch.power.  As there, ch.minimize is the oracle's dogleg
on the residual vector the REFERENCE built, with a central-difference Jacobian.

The dog: `MaxMixtureDog.get_gmm_prior` asserts `np.any(sqrdets == 0.0)` (dog_body_prior.py:73-74) -- inverted: with any
positive-definite covariance it fails as shipped.  Its module is therefore compiled with assertions off (optimize=1, as `python -O`
would), that module only; nothing else of it changes.  The product refuses a zero determinant instead (moshpp_amd/prior.py).
The dog's prior constants, as get_gmm_prior computes them, are recorded as well (`dog_prior_*`).

Cases: horse (optimize_toes off), horse with optimize_toes, horse with heavy dropouts and an empty frame (annealing), dog.
Run where the reference sources are present; the npz is committed and tests/test_animal_ref_golden.py holds the animal oracle to it.
"""
import ast
import importlib.util
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import make_ref_stageii_golden as g  # noqa: E402  (installs the stand-in modules)
from tests import animal_oracle as ao  # noqa: E402
from oracle import stageii_oracle as so  # noqa: E402

g.ch.exp = lambda a: g.Op(np.exp, a)
g.ch.power = lambda a, b: g.Op(np.power, a, b)

CASES = {   # name: (model_type, frames, markers, seed, vertices, empty frames, dropout, optimize_toes)
    'horse': ('animal_horse', 4, 40, 21, 1200, (), 0.02, False),
    'horse_toes': ('animal_horse', 3, 40, 22, 1200, (), 0.02, True),
    'horse_dropouts': ('animal_horse', 4, 40, 23, 1200, (2,), 0.15, False),
    'dog': ('animal_dog', 3, 40, 24, 1200, (), 0.02, False),
}


def load_ref_no_asserts(name, rel):
    """load_ref with the module compiled at optimize=1 (assert statements dropped): the dog prior's inverted assert."""
    path = os.path.join(g.REF, rel)
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    exec(compile(open(path).read(), path, 'exec', optimize=1), mod.__dict__)
    return mod


def run_reference_animal(model_type, F, M, seed, V, empty, dropout, toes):
    tmp = tempfile.mkdtemp(prefix='ref_stageii_animal_')
    case = ao.animal_ref_case(model_type, F, M, seed, V, empty_frames=empty, dropout=dropout, outdir=tmp)
    for n in ('moshpp', 'moshpp.models', 'moshpp.prior', 'moshpp.tools', 'moshpp.marker_layout'):
        g._module(n)
    g.load_ref('moshpp.models.smpl_fast_derivatives', 'models/smpl_fast_derivatives.py')
    g.load_ref('moshpp.prior.gmm_prior_ch', 'prior/gmm_prior_ch.py')
    g.load_ref('moshpp.prior.horse_body_prior', 'prior/horse_body_prior.py')
    dogp = load_ref_no_asserts('moshpp.prior.dog_body_prior', 'prior/dog_body_prior.py')
    bml = g.load_ref('moshpp.models.bodymodel_loader', 'models/bodymodel_loader.py')
    tlm = g.load_ref('moshpp.transformed_lm', 'transformed_lm.py')
    rig = g.load_ref('moshpp.rigid_transformations', 'rigid_transformations.py')
    mi = g.load_ref('moshpp.tools.mocap_interface', 'tools/mocap_interface.py')
    lm = g.load_ref('moshpp.marker_layout.labels_map', 'marker_layout/labels_map.py')
    src = open(os.path.join(g.REF, 'chmosh.py')).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == 'mosh_stageii'][0]
    ns = {'np': np, 'ch': g.ch, 'pickle': pickle, 'DictConfig': dict, 'logger': g._quiet, 'MocapSession': mi.MocapSession,
          'general_labels_map': lm.general_labels_map, 'load_moshpp_models': bml.load_moshpp_models,
          'TransformedCoeffs': tlm.TransformedCoeffs, 'TransformedLms': tlm.TransformedLms,
          'perform_rigid_adjustment': rig.perform_rigid_adjustment, 'visualize_pose_estimate': None}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), 'chmosh.py', 'exec'), ns)
    cfg = g.Cfg.of(dict(
        mocap=dict(unit='m', rotate=None, subject_name=None, multi_subject=False, start_fidx=0, end_fidx=-1, ds_rate=1),
        moshpp=dict(optimize_fingers=False, optimize_face=False, optimize_toes=toes, optimize_dynamics=False,
                    pose_hand_prior_fname=None, pose_body_prior_fname=case['prior_fname'], verbosity=0,
                    visualization=dict(marker_radius=dict(body=0.009))),
        surface_model=dict(fname=case['model_fname'], type=model_type, use_hands_mean=False, dof_per_hand=12, num_betas=16,
                           num_dmpls=0, num_expressions=0, betas_expr_start_id=16, dmpl_fname=None),
        opt_settings=dict(maxiter=100, weights=dict(so.stageii_weights_default()))))
    del g.N_MINIMIZE[:]
    out = ns['mosh_stageii'](case['mocap_fname'], cfg, case['s']['markers_latent'], case['s']['latent_labels'], case['s']['betas'],
                             case['s']['marker_meta'])
    extra = {}
    if model_type == 'animal_dog':
        w = dogp.MaxMixtureDog(case['prior_fname']).get_gmm_prior()
        extra = dict(means=np.asarray(w.means), chols=np.asarray(w.precs.r), weights=np.asarray(w.weights.r))
    return out, extra


def main():
    out = {}
    for name, (mt, F, M, seed, V, empty, dropout, toes) in CASES.items():
        res, extra = run_reference_animal(mt, F, M, seed, V, empty, dropout, toes)
        dbg = res['stageii_debug_details']
        out[f'{name}_args'] = np.array([F, M, seed, V, int(toes), int(round(dropout * 100))] + list(empty), dtype=np.int64)
        out[f'{name}_fullpose'] = np.asarray(res['fullpose'])
        out[f'{name}_trans'] = np.asarray(res['trans'])
        out[f'{name}_keys'] = np.array(sorted(res.keys()))
        out[f'{name}_err_keys'] = np.array(list(dbg['stageii_errs'].keys()))
        for k, v in dbg['stageii_errs'].items():
            out[f'{name}_err_{k}'] = np.asarray(v)
        out[f'{name}_n_obs'] = np.array([len(l) for l in dbg['labels_obs']])
        out[f'{name}_minimize_calls'] = np.array(g.N_MINIMIZE, dtype=np.int64)
        for k, v in extra.items():
            out[f'dog_prior_{k}'] = v
        print(name, 'frames solved', len(res['fullpose']), 'minimize calls', len(g.N_MINIMIZE), 'err keys', list(dbg['stageii_errs'].keys()))
    np.savez_compressed(os.path.join(HERE, 'ref_stageii_animal.npz'), **out)
    print('wrote', os.path.join(HERE, 'ref_stageii_animal.npz'))


if __name__ == '__main__':
    main()
