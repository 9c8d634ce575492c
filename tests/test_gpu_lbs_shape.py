"""GPU: the full-mesh export with per-frame coefficients of a free shape block (moshii_lbs_forward_shape_f32 / _f64), against the
ORACLE's verts_forward(..., shp=) after set_free_shape -- every vertex of every frame, 2e-5 m for the f32 export (the shape columns
ride in front of the pose features as hi + lo f16 pairs) -- and end to end: the mesh of a Stage-II result with
free expression / DMPL coefficients carries the markers the solver simulated."""
import os

import numpy as np
import pytest

from oracle import stageii_oracle as so
from tests.lbs_shape_common import F32_TOL, F64_TOL, block_case, block_device, export_inputs, oracle_verts

pytestmark = pytest.mark.gpu


def _export(dev, pose, trans, shape, env=None):
    """The f32 export, twice: the repeat has the same bits."""
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        got = dev['model'].lbs_forward(pose, trans, dtype=np.float32, shape=shape)
        again = dev['model'].lbs_forward(pose, trans, dtype=np.float32, shape=shape)
    finally:
        for k in (env or {}):
            del os.environ[k]
    np.testing.assert_array_equal(got, again)
    return got


@pytest.fixture(scope='module')
def smplx80(gpu_lib):
    """SMPL-X with 80 free columns, a 260-frame input with still hands, jaw and eyes, and the oracle's vertices for it: made once."""
    case = block_case('smplx', 80, seed=67)
    dev = block_device(case)
    pose, trans, shape = export_inputs(case, 260, seed=12, still=case['m']['body_dof'] - 9)
    return dict(case=case, dev=dev, pose=pose, trans=trans, shape=shape, ref=oracle_verts(case['m'], pose, trans, shape))


def test_smplx_80_expressions_130_frames(smplx80):
    c = smplx80
    pose, trans, shape = export_inputs(c['case'], 130, seed=11)
    ref = oracle_verts(c['case']['m'], pose, trans, shape)
    got = _export(c['dev'], pose, trans, shape)
    e64 = np.abs(c['dev']['model'].lbs_forward(pose[:3], trans[:3], shape=shape[:3]) - ref[:3]).max()
    print(f'smplx E=80 F=130: f32 export vs oracle {np.abs(got - ref).max():.2e} m; f64 kernel vs oracle {e64:.2e} m')
    assert np.abs(got - ref).max() < F32_TOL and e64 < F64_TOL
    assert np.abs(got[:2] - oracle_verts(c['case']['m'], pose[:2], trans[:2])).max() > 1e-3      # the block matters


def test_smplx_80_expressions_still_hands_jaw_eyes(smplx80):
    c = smplx80
    got = _export(c['dev'], c['pose'], c['trans'], c['shape'])
    full = _export(c['dev'], c['pose'], c['trans'], c['shape'], env={'MOSHII_LBS_STOP': '8'})      # no still-joint shortcut
    e1, e2 = np.abs(got - c['ref']).max(), np.abs(full - c['ref']).max()
    print(f'smplx E=80 F=260 still hands / jaw / eyes: vs oracle {e1:.2e} m with the shortcut, {e2:.2e} m without')
    assert e1 < F32_TOL and e2 < F32_TOL


def test_plain_kernel_with_shape_rows(smplx80):
    c = smplx80
    n = 40
    plain = _export(c['dev'], c['pose'][:n], c['trans'][:n], c['shape'][:n], env={'MOSHII_LBS_PLAIN': '1'})
    print(f'plain f32 kernel with shape rows vs oracle {np.abs(plain - c["ref"][:n]).max():.2e} m')
    assert np.abs(plain - c['ref'][:n]).max() < 5e-6


def test_plain_call_keeps_its_bits_next_to_shape_calls(smplx80):
    """No `shape`: the launches, instantiations and k-step count of a handle without a block -- same bits before and after a shape call
    that re-laid the shared scratch."""
    c = smplx80
    n = 130
    before = c['dev']['model'].lbs_forward(c['pose'][:n], c['trans'][:n], dtype=np.float32)
    _export(c['dev'], c['pose'][:n], c['trans'][:n], c['shape'][:n])
    np.testing.assert_array_equal(c['dev']['model'].lbs_forward(c['pose'][:n], c['trans'][:n], dtype=np.float32), before)
    assert np.abs(before[:4] - oracle_verts(c['case']['m'], c['pose'][:4], c['trans'][:4])).max() < F32_TOL


def test_smplh_8_dmpls_shuffled(gpu_lib):
    case = block_case('smplh', 8, seed=67, order='shuffled')
    dev = block_device(case)
    pose, trans, shape = export_inputs(case, 130, seed=11)
    ref = oracle_verts(case['m'], pose, trans, shape)
    got = _export(dev, pose, trans, shape)
    print(f'smplh E=8 F=130 shuffled: vs oracle {np.abs(got - ref).max():.2e} m')
    assert np.abs(got - ref).max() < F32_TOL


@pytest.mark.parametrize('E', [1, 125])
def test_smallest_and_largest_block(gpu_lib, E):
    case = block_case('smpl', E, seed=61)
    dev = block_device(case)
    pose, trans, shape = export_inputs(case, 33, seed=3)
    ref = oracle_verts(case['m'], pose, trans, shape)
    got = _export(dev, pose, trans, shape)
    e64 = np.abs(dev['model'].lbs_forward(pose, trans, shape=shape) - ref).max()
    print(f'smpl E={E} F=33: f32 vs oracle {np.abs(got - ref).max():.2e} m, f64 vs oracle {e64:.2e} m')
    assert np.abs(got - ref).max() < F32_TOL and e64 < F64_TOL


def test_cut_export_has_the_bits_of_the_one_call_export(gpu_lib):
    case = block_case('smplh', 8, seed=77)
    dev = block_device(case)
    pose, trans, shape = export_inputs(case, 700, seed=3)
    whole = _export(dev, pose, trans, shape)
    cut = _export(dev, pose, trans, shape, env={'MOSHII_LBS_FMAX': '256'})      # three sub-calls: the shape rows advance with the frames
    np.testing.assert_array_equal(cut, whole)
    ids = [0, 255, 256, 699]
    assert np.abs(whole[ids] - oracle_verts(case['m'], pose[ids], trans[ids], shape[ids])).max() < F32_TOL


# ---- end to end: a Stage-II solve with a free block, its mesh, its markers ----------------------------------------------------
def _surface_model(case):
    from moshpp_amd.models import SurfaceModel
    md = case['model']
    return SurfaceModel(case['model_type'], md['v_template'], md['shapedirs'], md['posedirs'], md['weights'], md['J_regressor'],
                        np.asarray(md['parents'], dtype=np.int32), md['body_dof'], md['hand_dof'], md['hands_mean'], md['selected_components'])


@pytest.fixture(scope='module', params=['expr', 'dmpl'])
def solved(request, gpu_lib):
    from moshpp_amd.chmosh import StageIISolver
    from moshpp_amd.prior import create_gmm_body_prior
    from tests.helpers import shape_case
    kind = request.param
    case = shape_case('smplx', F=6, kind='expr') if kind == 'expr' else shape_case('smplh', kind='dmpl')
    sm = _surface_model(case)
    E, start = case['E'], case['start']
    kw = dict(optimize_face=True, betas_expr_start_id=start, num_expressions=E) if kind == 'expr' else \
        dict(optimize_dynamics=True, num_dmpls=E, dmpl_pcs=case['model']['shapedirs'][:, :, start:start + E])
    solver = StageIISolver(sm, case['s']['betas'], case['s']['markers_latent'], create_gmm_body_prior(case['s']['gmm'], exclude_hands=True),
                           so.stageii_weights_default(), surface_model_type=case['model_type'], num_betas=start, **kw)
    # the solver attaches the markers where the case did: its markers_sim can be rebuilt from vertices with the case's closest / coef
    assert np.array_equal(solver.tc.closest, case['closest']) and np.abs(solver.tc.coef - case['coef']).max() < 1e-9
    out = solver.solve(case['obs'], case['vis'], chain_mode='sequential')
    assert (out['status'] == 0).all() and np.abs(out['shape']).max() > 0.2
    return dict(kind=kind, case=case, sm=sm, solver=solver, out=out)


def _markers(case, verts):
    cl = case['closest']
    return np.stack([so.markers_from_verts(case['coef'], v[cl[:, 0]], v[cl[:, 1]], v[cl[:, 2]]) for v in verts])


def test_vertices_of_a_solve_carry_its_simulated_markers(solved):
    s = solved
    verts = s['solver'].vertices(s['out'])
    assert verts.dtype == np.float32 and verts.shape == (s['out']['pose'].shape[0], s['sm'].V, 3)
    err = np.abs(_markers(s['case'], verts.astype(np.float64)) - s['out']['markers_sim']).max(axis=(1, 2))
    frozen = s['solver'].dev.lbs_forward(s['out']['pose'], s['out']['trans'], dtype=np.float32)
    miss = np.abs(_markers(s['case'], frozen.astype(np.float64)) - s['out']['markers_sim']).max()
    print(f"{s['kind']}: markers re-attached to the exported mesh vs markers_sim, per frame {err}; without the block {miss:.2e} m")
    assert err.max() < 2e-5
    assert miss > 1e-3            # the frozen mesh does not carry them: the check above cannot pass vacuously


def test_stageii_vertices_of_a_stageii_dict(solved):
    from moshpp_amd import mosh_head
    s = solved
    case, out, solver = s['case'], s['out'], s['solver']
    E, start = case['E'], case['start']
    betas_t = np.tile(solver.betas, (out['pose'].shape[0], 1))
    betas_t[:, start:start + E] += out['shape']
    cfg = {'surface_model': {'type': case['model_type'], 'num_betas': start, 'betas_expr_start_id': start, 'num_expressions': E,
                             'num_dmpls': E, 'fname': None},
           'moshpp': {'optimize_face': s['kind'] == 'expr', 'optimize_dynamics': s['kind'] == 'dmpl'}}
    data = {'fullpose': out['fullpose'], 'trans': out['trans'], 'betas': case['s']['betas'], 'stageii_debug_details': {'cfg': cfg}}
    data['expression' if s['kind'] == 'expr' else 'dmpls'] = betas_t[:, start:]
    ref = np.stack([so.verts_forward(case['m'], out['fullpose'][f], out['trans'][f], shp=out['shape'][f]) for f in range(len(out['trans']))])
    got = mosh_head.stageii_vertices(data, surface_model=s['sm'])
    e = np.abs(got - ref).max()
    print(f"{s['kind']}: stageii_vertices vs oracle {e:.2e} m")
    assert got.dtype == np.float32 and e < 2e-5
    rows = mosh_head.stageii_vertices(data, surface_model=s['sm'], frame_ids=[4, 1])
    assert rows.shape == (2,) + got.shape[1:] and np.abs(rows - ref[[4, 1]]).max() < 2e-5      # frame_ids selects rows, in the order given
    assert np.abs(mosh_head.stageii_vertices(data, surface_model=s['sm'], dtype=np.float64) - ref).max() < 1e-9
    # without free coefficients: the plain export of the frozen body
    plain = {k: v for k, v in data.items() if k not in ('expression', 'dmpls')}
    plain['stageii_debug_details'] = {'cfg': dict(cfg, moshpp={'optimize_face': False, 'optimize_dynamics': False})}
    frozen = np.stack([so.verts_forward(case['m'], out['fullpose'][f], out['trans'][f]) for f in range(len(out['trans']))])
    assert np.abs(mosh_head.stageii_vertices(plain, surface_model=s['sm']) - frozen).max() < 2e-5
