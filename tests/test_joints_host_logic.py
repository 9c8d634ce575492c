"""CPU, no kernel: the posed-joint calls are declared where they must be, and capi.Model.posed_joints, StageIISolver.joints and
mosh_head.stageii_joints refuse bad input with a clear error BEFORE any model file or device is touched (the models here have no
handle and the stored model file does not exist: anything that got further would raise something else)."""
import os
import re

import numpy as np
import pytest

from moshpp_amd import capi, chmosh, mosh_head
from tests.test_normals_host_logic import _data, _handleless_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('moshii_joints_f32', 'moshii_joints_f64')


def test_header_declares_the_two_entries_and_names_the_kernels():
    hdr = open(os.path.join(ROOT, 'include', 'moshii.h')).read()
    for name in ENTRIES:
        assert re.search(r'\bint\s+' + name + r'\s*\(moshii_model_t m, int32_t F,', hdr), name
    for kernel in ('k_joints<float>', 'k_joints<double>', 'k_joints_shape<float>', 'k_joints_shape<double>'):
        assert kernel in hdr


def test_exports_hold_the_two_entries_and_version_106():
    for name in ENTRIES:
        res, args = capi.EXPORTS[name]
        assert len(args) == 9                                   # m, F, pose, trans, shape, joints, rot, flags, stream
    from moshpp_amd import build
    build.build(force=False, verbose=False)
    lib = capi.load()
    assert lib.moshii_version() >= 106
    for name in ENTRIES:
        assert hasattr(lib, name)


def test_posed_joints_checks_its_arguments():
    m = _handleless_model()
    with pytest.raises(ValueError, match='dtype'):
        m.posed_joints(np.zeros((1, 72)), np.zeros((1, 3)), dtype=np.float16)
    with pytest.raises(ValueError, match=r'pose / trans must be \[F, 72\] / \[F, 3\]'):
        m.posed_joints(np.zeros((2, 71)), np.zeros((2, 3)))
    with pytest.raises(ValueError, match='pose / trans'):
        m.posed_joints(np.zeros((2, 72)), np.zeros((3, 3)))
    with pytest.raises(ValueError, match='no free shape block'):
        m.posed_joints(np.zeros((2, 72)), np.zeros((2, 3)), shape=np.zeros((2, 4)))
    with pytest.raises(ValueError, match=r'\[2, 4\]'):
        _handleless_model(nshape=4).posed_joints(np.zeros((2, 72)), np.zeros((2, 3)), shape=np.zeros((2, 3)))
    with pytest.raises(ValueError, match='non-finite'):
        _handleless_model(nshape=4).posed_joints(np.zeros((2, 72)), np.zeros((2, 3)), shape=np.full((2, 4), np.nan))
    with pytest.raises(ValueError, match='no free shape block'):
        m.posed_joints_device(1, 1, 2, 3, shape_ptr=5)


def test_solver_joints_key_checks():
    s = chmosh.StageIISolver.__new__(chmosh.StageIISolver)
    s.n_shape, s.dev = 0, None
    with pytest.raises(KeyError, match=r"StageIISolver.joints: the result has no 'pose'"):
        s.joints(dict(trans=np.zeros((3, 3))))
    with pytest.raises(KeyError, match=r"StageIISolver.joints: the result has no 'trans'"):
        s.joints(dict(pose=np.zeros((3, 72))))
    s.n_shape = 8
    with pytest.raises(KeyError, match=r"StageIISolver.joints: the result has no 'shape'"):
        s.joints(dict(pose=np.zeros((3, 72)), trans=np.zeros((3, 3))))


def test_stageii_joints_refusals_come_before_any_model_or_device(tmp_path):
    d = _data()
    for k in ('fullpose', 'trans', 'betas', 'stageii_debug_details'):
        with pytest.raises(KeyError, match=k):
            mosh_head.stageii_joints({a: v for a, v in d.items() if a != k})
    with pytest.raises(KeyError, match='cfg'):
        mosh_head.stageii_joints(dict(d, stageii_debug_details={}))
    with pytest.raises(ValueError, match=r'not \[T, 3K\] / \[T, 3\]'):
        mosh_head.stageii_joints(dict(d, trans=np.zeros((4, 3))))
    with pytest.raises(IndexError, match='frame_ids'):
        mosh_head.stageii_joints(d, frame_ids=[5])
    with pytest.raises(IndexError, match='frame_ids'):
        mosh_head.stageii_joints(d, frame_ids=[-1])
    with pytest.raises(ValueError, match='integers'):
        mosh_head.stageii_joints(d, frame_ids=[0.5])
    with pytest.raises(ValueError, match=r'must end in \.npz'):
        mosh_head.stageii_joints(d, out_fname=str(tmp_path / 'joints.bvh'))
    taken = tmp_path / 'taken.npz'
    taken.write_bytes(b'kept')
    with pytest.raises(FileExistsError, match='taken.npz'):
        mosh_head.stageii_joints(d, out_fname=str(taken))
    assert taken.read_bytes() == b'kept'
    e = _data()
    del e['stageii_debug_details']['mocap_frame_rate']
    with pytest.raises(KeyError, match='frame rate'):
        mosh_head.stageii_joints(e, out_fname=str(tmp_path / 'new.npz'))
    assert not (tmp_path / 'new.npz').exists()
    # an expression result on a model type that has none
    with pytest.raises(ValueError, match='smplx'):
        mosh_head.stageii_joints(dict(d, expression=np.zeros((5, 80))))


def test_plan_of_a_good_call(tmp_path):
    d = _data()
    plan, rate = mosh_head._stageii_joints_plan(d, [2, 0, 2], str(tmp_path / 'sub' / 'j.npz'))
    assert list(plan[5]) == [2, 0, 2] and rate == 100.0 and plan[2] is None
    assert not (tmp_path / 'sub').exists()                      # planning creates nothing
    del d['stageii_debug_details']['mocap_frame_rate']
    plan, rate = mosh_head._stageii_joints_plan(d, None, None)
    assert list(plan[5]) == list(range(5)) and rate is None
