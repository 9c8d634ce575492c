"""CPU: argument handling of the marker-to-skin distance calls -- capi.Model.surface_distance / marker_surface_distance,
StageIISolver.marker_skin_distance and mosh_head.stageii_marker_skin_distance refuse bad input with a clear error BEFORE any device
call (the models here have no handle and no device exists: anything that reached the library would raise MoshiiError instead) --, the
packing of the ragged observations and the summary statistics."""
import types

import numpy as np
import pytest

from moshpp_amd import capi, chmosh, mosh_head
from tests.test_normals_host_logic import _data, _handleless_model


def test_declares_the_four_entries_and_version_105():
    for name in ('moshii_surface_distance_f32', 'moshii_surface_distance_f64', 'moshii_marker_surface_distance_f32',
                 'moshii_marker_surface_distance_f64'):
        assert name in capi.EXPORTS
    from moshpp_amd import build
    build.build(force=False, verbose=False)
    assert capi.load().moshii_version() >= 105


def test_calls_without_faces_are_refused():
    m = _handleless_model(faces=0)
    with pytest.raises(ValueError, match='no faces'):
        m.surface_distance(np.zeros((1, 100, 3)), np.zeros((1, 2, 3)))
    with pytest.raises(ValueError, match='no faces'):
        m.marker_surface_distance(np.zeros((1, 72)), np.zeros((1, 3)), np.zeros((1, 2, 3)))
    with pytest.raises(ValueError, match='no faces'):
        m.surface_distance_device(1, 1, 2, 3, 4)
    with pytest.raises(ValueError, match='no faces'):
        m.marker_surface_distance_device(1, 1, 2, 2, 3, 4)


@pytest.mark.parametrize('verts,points,msg', [(np.zeros((3, 99, 3)), np.zeros((3, 2, 3)), r'verts must be \[F, 100, 3\]'),
                                              (np.zeros(300), np.zeros((1, 2, 3)), r'verts must be'),
                                              (np.zeros((3, 100, 3)), np.zeros((2, 2, 3)), r'points must be \[F, N, 3\] = \[3, N, 3\]'),
                                              (np.zeros((3, 100, 3)), np.zeros((3, 2, 2)), 'points must be'),
                                              (np.zeros((3, 100, 3)), np.zeros((2, 3)), 'points must be'),
                                              (np.zeros((1, 100, 3)), np.zeros((2, 3), dtype=complex), 'real numbers'),
                                              (np.zeros((1, 100, 3)), np.array([[['a', 'b', 'c']]]), 'real numbers')])
def test_surface_distance_checks_shapes(verts, points, msg):
    with pytest.raises(ValueError, match=msg):
        _handleless_model().surface_distance(verts, points)


def test_dtype_and_pose_checks():
    m = _handleless_model()
    with pytest.raises(ValueError, match='dtype'):
        m.surface_distance(np.zeros((1, 100, 3)), np.zeros((1, 2, 3)), dtype=np.float16)
    with pytest.raises(ValueError, match='dtype'):
        m.marker_surface_distance(np.zeros((1, 72)), np.zeros((1, 3)), np.zeros((1, 2, 3)), dtype=int)
    with pytest.raises(ValueError, match='pose / trans'):
        m.marker_surface_distance(np.zeros((2, 71)), np.zeros((2, 3)), np.zeros((2, 2, 3)))
    with pytest.raises(ValueError, match='no free shape block'):
        m.marker_surface_distance(np.zeros((2, 72)), np.zeros((2, 3)), np.zeros((2, 2, 3)), shape=np.zeros((2, 4)))
    with pytest.raises(ValueError, match=r'\[2, 4\]'):
        _handleless_model(nshape=4).marker_surface_distance(np.zeros((2, 72)), np.zeros((2, 3)), np.zeros((2, 2, 3)), shape=np.zeros((2, 3)))
    with pytest.raises(ValueError, match='points must be'):
        m.marker_surface_distance(np.zeros((2, 72)), np.zeros((2, 3)), np.zeros((3, 2, 3)))
    with pytest.raises(ValueError, match='no free shape block'):
        m.marker_surface_distance_device(1, 1, 2, 2, 3, 4, shape_ptr=5)


def _ragged():
    """Four frames over the labels A B C: B missing on frame 1, nothing on frame 2, the observed order differs from the label order."""
    mk = [np.array([[1., 0, 0], [2., 0, 0], [3., 0, 0]]), np.array([[13., 0, 0], [11., 0, 0]]), np.zeros((0, 3)),
          np.array([[32., 0, 0], [33., 0, 0], [31., 0, 0]])]
    lb = [['A', 'B', 'C'], ['C', 'A'], [], ['B', 'C', 'A']]
    return mk, lb


def test_packing_of_ragged_observations():
    mk, lb = _ragged()
    p = chmosh.pack_observed_markers(mk, lb, ['A', 'B', 'C'])
    assert p.shape == (4, 3, 3)
    np.testing.assert_array_equal(p[:, :, 0], [[1, 2, 3], [11, np.nan, 13], [np.nan] * 3, [31, 32, 33]])
    assert np.isnan(p[1, 1]).all() and (p[0, :, 1:] == 0).all()
    # frames in frame_ids order, repeats allowed; another label order
    q = chmosh.pack_observed_markers(mk, lb, ['C', 'A', 'B'], frame_ids=[3, 1, 3])
    np.testing.assert_array_equal(q[:, :, 0], [[33, 31, 32], [13, 11, np.nan], [33, 31, 32]])
    assert chmosh.pack_observed_markers(mk, lb, ['A', 'B', 'C'], frame_ids=[]).shape == (0, 3, 3)


def test_packing_refusals():
    mk, lb = _ragged()
    with pytest.raises(ValueError, match='4 frames, labels_obs 3'):
        chmosh.pack_observed_markers(mk, lb[:3], ['A', 'B', 'C'])
    with pytest.raises(ValueError, match=r"frame 1: markers_obs is \(2, 3\), labels_obs names 3"):
        chmosh.pack_observed_markers(mk, [lb[0], ['C', 'A', 'B']] + lb[2:], ['A', 'B', 'C'])
    with pytest.raises(ValueError, match="'Z'"):
        chmosh.pack_observed_markers(mk, [['A', 'B', 'Z']] + lb[1:], ['A', 'B', 'C'])
    with pytest.raises(ValueError, match='twice'):
        chmosh.pack_observed_markers(mk, lb, ['A', 'B', 'A'])
    with pytest.raises(IndexError, match='frame_ids'):
        chmosh.pack_observed_markers(mk, lb, ['A', 'B', 'C'], frame_ids=[4])
    with pytest.raises(ValueError, match='integers'):
        chmosh.pack_observed_markers(mk, lb, ['A', 'B', 'C'], frame_ids=[0.5])


def test_summary_statistics_are_nan_aware():
    d = np.array([[0.010, np.nan, np.nan], [0.012, -0.002, np.nan], [np.nan, 0.004, np.nan], [-0.001, 0.006, np.nan], [0.009, -0.008, np.nan]])
    s = chmosh.skin_distance_summary(d, ['A', 'B', 'C'])
    assert s['A']['count'] == 4 and s['B']['count'] == 4 and s['C']['count'] == 0
    assert s['A']['median'] == pytest.approx(0.0095) and s['A']['negative_share'] == 0.25
    assert s['B']['median'] == pytest.approx(0.001) and s['B']['negative_share'] == 0.5
    assert s['A']['p5'] == pytest.approx(np.percentile([0.010, 0.012, -0.001, 0.009], 5))
    assert s['B']['p95'] == pytest.approx(np.percentile([-0.002, 0.004, 0.006, -0.008], 95))
    assert all(np.isnan(s['C'][k]) for k in ('median', 'p5', 'p95', 'negative_share'))
    with pytest.raises(ValueError, match='expected'):
        chmosh.skin_distance_summary(d, ['A', 'B'])


def _data_with_markers(T=5):
    d = _data(T)
    d['stageii_debug_details']['markers_obs'] = [np.zeros((2, 3))] * T
    d['stageii_debug_details']['labels_obs'] = [['A', 'B']] * T
    return d


def test_mosh_head_refusals_come_before_any_model_or_device():
    # (the stored model file does not exist: reaching load_surface_model would raise something else than these)
    d = _data_with_markers()
    with pytest.raises(KeyError, match='trans'):
        mosh_head.stageii_marker_skin_distance({k: v for k, v in d.items() if k != 'trans'})
    for k in ('markers_obs', 'labels_obs'):
        e = _data_with_markers()
        del e['stageii_debug_details'][k]
        with pytest.raises(KeyError, match=k):
            mosh_head.stageii_marker_skin_distance(e)
    with pytest.raises(ValueError, match='no faces'):
        mosh_head.stageii_marker_skin_distance(d, surface_model=types.SimpleNamespace(f=None, V=6890, K=52))
    with pytest.raises(IndexError, match='frame_ids'):
        mosh_head.stageii_marker_skin_distance(d, frame_ids=[5])
    e = _data_with_markers()
    e['stageii_debug_details']['labels_obs'] = [['A', 'B']] * 4 + [['A']]
    with pytest.raises(ValueError, match='frame 4'):
        mosh_head.stageii_marker_skin_distance(e)
    e = _data_with_markers()
    e['stageii_debug_details']['markers_obs'] = e['stageii_debug_details']['markers_obs'][:4]
    with pytest.raises(ValueError, match='hold 4 / 5 frames'):
        mosh_head.stageii_marker_skin_distance(e)
    e = _data_with_markers()
    e['latent_labels'] = ['A', 'C']
    with pytest.raises(ValueError, match="'B'"):
        mosh_head.stageii_marker_skin_distance(e)


def test_plan_of_a_good_call():
    d = _data_with_markers()
    plan, labels, points = mosh_head._stageii_marker_skin_distance_plan(d, None, [2, 0])
    assert labels == ['A', 'B'] and points.shape == (2, 2, 3) and list(plan[5]) == [2, 0]
    d['latent_labels'] = ['B', 'X', 'A']
    plan, labels, points = mosh_head._stageii_marker_skin_distance_plan(d, None, None)
    assert labels == ['B', 'X', 'A'] and points.shape == (5, 3, 3) and np.isnan(points[:, 1]).all() and np.isfinite(points[:, [0, 2]]).all()


def test_solver_method_refusals():
    s = chmosh.StageIISolver.__new__(chmosh.StageIISolver)
    s.n_shape, s.sm, s.dev = 0, types.SimpleNamespace(f=None), None
    out = dict(pose=np.zeros((3, 72)), trans=np.zeros((3, 3)))
    with pytest.raises(KeyError, match='trans'):
        s.marker_skin_distance(dict(pose=out['pose']), obs=np.zeros((3, 2, 3)))
    with pytest.raises(ValueError, match='no faces'):
        s.marker_skin_distance(out, obs=np.zeros((3, 2, 3)))
    s.sm = types.SimpleNamespace(f=np.zeros((1, 3), int))
    with pytest.raises(KeyError, match='markers_obs'):
        s.marker_skin_distance(out)
    mk, lb = _ragged()
    with pytest.raises(ValueError, match='label order'):
        s.marker_skin_distance(dict(out, markers_obs=mk[:3], labels_obs=lb[:3]))
    with pytest.raises(ValueError, match='the result has 3 frames'):
        s.marker_skin_distance(dict(out, markers_obs=mk, labels_obs=lb), labels=['A', 'B', 'C'])
    with pytest.raises(ValueError, match='the result has 3 frames'):
        s.marker_skin_distance(out, obs=np.zeros((2, 2, 3)))
