"""CPU: posed joints and world joint rotations (moshii_joints_*) in the emulation build -- lbs_forward.hip and moshii_api.hip compiled
unchanged for the host, the kernel's wavefronts run as fibers, its cross-lane fetches as rendezvous.  Reference: the oracle's
fullpose_from_pose -> _shaped -> joint_transforms in NumPy f64 on the device's own inputs; bodies, inputs, checker and bounds:
tests/joints_common.py."""
import numpy as np
import pytest

from oracle import stageii_oracle as so
from tests import joints_common as jc
from tests import normals_common as nc
from tests.emu.emu_moshii import emulated_libmoshii


@pytest.mark.parametrize('name,F', [('mano', 1), ('mano', 5), ('smpl', 3), ('smplh', 5), ('smplx', 5), ('one', 3), ('chain', 3), ('star', 3)])
def test_posed_joints_against_the_oracle_in_emulation(name, F):
    b = jc.body(name)
    with emulated_libmoshii():
        dev = jc.device(b)
        res = jc.run_body(dev, b, F)
        if b['E']:      # without the row: the frozen joints, through the instantiation without one
            pose, trans, _, with_row, _ = res[np.float64]
            plain = dev.posed_joints(pose, trans)
            jc.check(plain, None, b['m'], pose, trans, None, np.float64)
            assert np.abs(plain - with_row).max() > 1e-4
        dev.close()


def test_pinned_body_export_vertices_are_the_joints_in_emulation():
    b = jc.body('pinned')
    with emulated_libmoshii():
        dev = jc.device(b)
        jc.run_body(dev, b, 3)
        for with_shape in (False, True):
            jc.check_pinned(dev, b, 3, with_shape)
        dev.close()


def test_all_four_launch_names_are_reported_in_emulation():
    from moshpp_amd import capi
    b = jc.body('pinned')
    seen = set()
    with emulated_libmoshii():
        dev = jc.device(b)
        for dtype in (np.float32, np.float64):
            pose, trans, shape = jc.inputs(b, 2, dtype)
            for s in (None, shape):
                dev.posed_joints(pose, trans, shape=s, dtype=dtype)
                name, lds, threads = capi.last_launch_info()
                assert name == jc.NAMES[(dtype, s is not None)] and lds == 0 and threads % 64 == 0
                seen.add(name)
        dev.close()
    assert seen == {'k_joints<float>', 'k_joints<double>', 'k_joints_shape<float>', 'k_joints_shape<double>'}


def test_library_refusals_in_emulation():
    """The C ABI's own checks: null joints, negative F, a shape row without a block -> MOSHII_ERR_ARG with a message that names the
    fault; F == 0 -> MOSHII_OK and nothing launched; rot may be null.  (A handle always has betas -- moshii_model_create sets zeros --
    so the refusal before moshii_model_set_betas cannot be reached through the public calls.)"""
    from moshpp_amd import capi
    b = jc.body('mano')
    pose, trans, _ = jc.inputs(b, 2, np.float32)
    K = b['m']['K']
    with emulated_libmoshii():
        lib = capi.load()
        assert lib.moshii_version() >= 106
        dev = jc.device(b)
        want = dev.posed_joints(pose, trans, dtype=np.float32)
        assert capi.last_launch_info()[0] == 'k_joints<float>'
        j = np.zeros((2, K, 3), np.float32)
        args = [dev.handle, 2, pose.ctypes.data, trans.ctypes.data, None, j.ctypes.data, None, capi.BUFFERS_HOST, None]
        assert lib.moshii_joints_f32(*args) == 0
        np.testing.assert_array_equal(j, want)
        bad = list(args); bad[5] = None
        assert lib.moshii_joints_f32(*bad) == -1 and b'joints is null' in lib.moshii_last_error()
        bad = list(args); bad[1] = -1
        assert lib.moshii_joints_f32(*bad) == -1 and b'negative F' in lib.moshii_last_error()
        bad = list(args); bad[4] = pose.ctypes.data
        assert lib.moshii_joints_f32(*bad) == -1 and b'moshii_model_set_free_shape' in lib.moshii_last_error()
        bad = list(args); bad[0] = None
        assert lib.moshii_joints_f64(*bad) == -1 and b'null model' in lib.moshii_last_error()
        bad = list(args); bad[2] = None
        assert lib.moshii_joints_f32(*bad) == -1 and b'pose or trans' in lib.moshii_last_error()
        dev.posed_joints(pose.astype(np.float64), trans.astype(np.float64))
        zero = list(args); zero[1] = 0; zero[2] = zero[3] = None
        j[:] = 7.0
        assert lib.moshii_joints_f32(*zero) == 0 and (j == 7.0).all()
        assert capi.last_launch_info()[0] == 'k_joints<double>'          # nothing was launched: the call before it still stands
        assert dev.posed_joints(np.zeros((0, b['m']['NP'])), np.zeros((0, 3))).shape == (0, K, 3)
        with pytest.raises(ValueError, match='no free shape block'):
            dev.posed_joints(pose, trans, shape=np.zeros((2, 3)))
        with pytest.raises(ValueError, match='pose / trans'):
            dev.posed_joints(pose[:, :-1], trans)
        with pytest.raises(ValueError, match='dtype'):
            dev.posed_joints(pose, trans, dtype=np.float16)
        dev.close()


def test_mosh_head_stageii_joints_in_emulation(tmp_path):
    from moshpp_amd import mosh_head
    from tests.test_normals_emulation import _stageii_result
    case = nc.mesh_case('mano', 778)
    sm, data, _ = _stageii_result(case, 5)
    m = case['m']
    fullpose, trans = data['fullpose'], data['trans']
    full_m = dict(m, body_dof=3 * m['K'], hand_dof=0, NP=3 * m['K'])        # the stored pose is the FULL pose
    oj, orot = jc.oracle(full_m, fullpose, trans)
    fname = tmp_path / 'sub' / 'joints.npz'
    with emulated_libmoshii():
        res = mosh_head.stageii_joints(data, surface_model=sm, return_rotations=True, out_fname=str(fname))
        sub = mosh_head.stageii_joints(data, surface_model=sm, frame_ids=[4, 0, 4], dtype=np.float32)
        with pytest.raises(FileExistsError, match='joints.npz'):
            mosh_head.stageii_joints(data, surface_model=sm, out_fname=str(fname))
    assert set(res) == {'joints', 'rotations', 'parents', 'frame_ids', 'mocap_frame_rate', 'surface_model_type'}
    assert res['joints'].dtype == np.float64 and np.abs(res['joints'] - oj).max() <= jc.F64_TOL
    assert np.abs(res['rotations'] - orot).max() <= jc.F64_TOL
    np.testing.assert_array_equal(res['parents'], np.asarray(case['model']['parents']))
    assert list(res['frame_ids']) == list(range(5)) and res['mocap_frame_rate'] == 100.0 and res['surface_model_type'] == 'mano'
    assert 'rotations' not in sub and sub['joints'].dtype == np.float32 and list(sub['frame_ids']) == [4, 0, 4]
    np.testing.assert_array_equal(sub['joints'][0], sub['joints'][2])
    rows = [4, 0, 4]                                                          # (float32: the stored pose and translation rounded first)
    jc.check(sub['joints'], None, full_m, fullpose[rows].astype(np.float32), trans[rows].astype(np.float32), None, np.float32)
    with np.load(fname) as z:
        assert set(z.files) == set(res)
        for k in ('joints', 'rotations', 'parents', 'frame_ids'):
            np.testing.assert_array_equal(z[k], res[k])
        assert float(z['mocap_frame_rate']) == 100.0 and str(z['surface_model_type']) == 'mano'


def test_expression_result_moves_the_face_joints_in_emulation():
    """A Stage-II result with per-frame expression coefficients on the SMPL-X block case: stageii_joints passes them on, the joints
    follow (the oracle with the coefficients as an offset on the frozen betas), and differ from the frozen body's."""
    from moshpp_amd import mosh_head
    from moshpp_amd.models import SurfaceModel
    b = jc.body('smplx')
    md, m, E, start = b['model'], b['m'], b['E'], b['start']
    sm = SurfaceModel('smplx', md['v_template'], md['shapedirs'], md['posedirs'], md['weights'], md['J_regressor'],
                      np.asarray(md['parents'], dtype=np.int32), md['body_dof'], md['hand_dof'], md['hands_mean'], md['selected_components'])
    pose, trans, shape = jc.inputs(b, 4, np.float64, seed=9)
    fullpose = np.stack([so.fullpose_from_pose(m, p) for p in pose])
    nb = start                                                                 # the Stage-I betas: everything in front of the block
    betas = np.asarray(b['betas'], dtype=np.float64)
    block = betas[start:start + E]                                             # a result stores the block's frozen betas + the solved offsets
    cfg = {'surface_model': {'type': 'smplx', 'num_betas': nb, 'fname': None, 'betas_expr_start_id': start, 'num_expressions': E},
           'moshpp': {'optimize_face': True}}
    data = {'fullpose': fullpose, 'trans': trans, 'betas': betas[:nb], 'expression': block + shape,
            'stageii_debug_details': {'cfg': cfg, 'mocap_frame_rate': 120.0}}
    still = dict(data, expression=np.tile(block, (len(shape), 1)))
    with emulated_libmoshii():
        moved = mosh_head.stageii_joints(data, surface_model=sm)
        frozen = mosh_head.stageii_joints(still, surface_model=sm)
    oj, _ = jc.oracle(m, pose, trans, shape)
    assert np.abs(moved['joints'] - oj).max() <= jc.F64_TOL
    diff = np.abs(moved['joints'] - frozen['joints']).max()
    print(f'expression coefficients move the joints by up to {diff:.3e} m')
    assert diff > 1e-4


def test_solver_joints_needs_trans():
    from moshpp_amd import chmosh
    s = chmosh.StageIISolver.__new__(chmosh.StageIISolver)
    s.n_shape, s.dev = 0, None
    with pytest.raises(KeyError, match=r"StageIISolver.joints: the result has no 'trans'"):
        s.joints(dict(pose=np.zeros((3, 72))))
    s.n_shape = 4
    with pytest.raises(KeyError, match="'shape'"):
        s.joints(dict(pose=np.zeros((3, 72)), trans=np.zeros((3, 3))))
