"""CPU: argument handling of the mesh-export calls that take free shape coefficients -- mosh_head.stageii_vertices and
capi.Model.lbs_forward(shape=) refuse bad input with a clear error BEFORE any device call (this host has no device: reaching the
library would raise MoshiiError instead)."""
import numpy as np
import pytest

from moshpp_amd import capi, mosh_head


def _data(T=5, K=55, model_type='smplx', face=True, dyn=False, E=10):
    cfg = {'surface_model': {'type': model_type, 'num_betas': 16, 'betas_expr_start_id': 300, 'num_expressions': E, 'num_dmpls': E,
                             'fname': '/nonexistent/model.npz'},
           'moshpp': {'optimize_face': face, 'optimize_dynamics': dyn}}
    d = {'fullpose': np.zeros((T, 3 * K)), 'trans': np.zeros((T, 3)), 'betas': np.zeros(16), 'stageii_debug_details': {'cfg': cfg}}
    if face:
        d['expression'] = np.zeros((T, E))
    if dyn:
        d['dmpls'] = np.zeros((T, E))
    return d


@pytest.mark.parametrize('key', ['fullpose', 'trans', 'betas', 'stageii_debug_details', 'expression'])
def test_stageii_vertices_names_the_missing_key(key):
    d = _data()
    del d[key]
    with pytest.raises(KeyError, match=key):
        mosh_head.stageii_vertices(d)


def test_stageii_vertices_needs_the_stored_cfg():
    d = _data()
    d['stageii_debug_details'] = {}
    with pytest.raises(KeyError, match='cfg'):
        mosh_head.stageii_vertices(d)


@pytest.mark.parametrize('ids', [[5], [-1], [0, 7]])
def test_stageii_vertices_frame_ids_out_of_range(ids):
    with pytest.raises(IndexError, match='frame_ids'):
        mosh_head.stageii_vertices(_data(), frame_ids=ids)


def test_stageii_vertices_frame_ids_must_be_integers():
    with pytest.raises(ValueError, match='frame_ids'):
        mosh_head.stageii_vertices(_data(), frame_ids=[0.5])


def test_stageii_vertices_expression_on_a_model_without_that_block():
    d = _data(model_type='smplh', K=52, face=False)
    d['expression'] = np.zeros((5, 10))
    with pytest.raises(ValueError, match='expression'):
        mosh_head.stageii_vertices(d)
    with pytest.raises(ValueError, match='expression'):
        mosh_head.stageii_vertices(_data(model_type='smplh', K=52, face=True))
    with pytest.raises(ValueError, match='DMPL'):
        mosh_head.stageii_vertices(_data(model_type='smplx', face=False, dyn=True))
    with pytest.raises(ValueError, match='DMPL'):
        mosh_head.stageii_vertices(_data(model_type='animal_horse', K=36, face=False, dyn=True))


def test_stageii_vertices_coefficient_array_must_match_the_frames():
    d = _data()
    d['expression'] = np.zeros((4, 10))
    with pytest.raises(ValueError, match='expression'):
        mosh_head.stageii_vertices(d)
    d['expression'] = np.zeros((5, 9))      # fewer columns than cfg.surface_model.num_expressions
    with pytest.raises(ValueError, match='expression'):
        mosh_head.stageii_vertices(d)


def test_stageii_vertices_plan_of_a_good_dict():
    sm, mp, kind, start, count, ids = mosh_head._stageii_vertices_plan(_data(), [3, 0])
    assert (kind, start, count, list(ids)) == ('expr', 300, 10, [3, 0])
    assert mosh_head._stageii_vertices_plan(_data(model_type='smplh', K=52, face=False, dyn=True), None)[2:5] == ('dmpl', 16, 10)
    kind, start, count, ids = mosh_head._stageii_vertices_plan(_data(model_type='animal_dog', K=36, face=False), None)[2:]
    assert kind is None and count == 0 and list(ids) == [0, 1, 2, 3, 4]


def _handleless_model(NP=72, V=100, nshape=8):
    m = capi.Model.__new__(capi.Model)      # no device, no handle: anything that reached the library would fail on the null handle
    m.NP, m.V, m.handle = NP, V, None
    if nshape is not None:
        m.n_free_shape = nshape
    return m


@pytest.mark.parametrize('shape,msg', [(np.zeros((3, 7)), r'\[3, 8\]'), (np.zeros((2, 8)), r'\[3, 8\]'), (np.zeros(8), r'\[3, 8\]'),
                                       (np.zeros((3, 8, 1)), r'\[3, 8\]'), (np.full((3, 8), np.nan), 'non-finite'),
                                       (np.zeros((3, 8), dtype=complex), 'real'), (np.array([['a'] * 8] * 3), 'real')])
def test_lbs_forward_checks_the_shape_array(shape, msg):
    m = _handleless_model()
    for dtype in (np.float64, np.float32):
        with pytest.raises(ValueError, match=msg):
            m.lbs_forward(np.zeros((3, 72)), np.zeros((3, 3)), dtype=dtype, shape=shape)


def test_lbs_forward_shape_without_a_block():
    for m in (_handleless_model(nshape=None), _handleless_model(nshape=0)):
        with pytest.raises(ValueError, match='no free shape block'):
            m.lbs_forward(np.zeros((3, 72)), np.zeros((3, 3)), shape=np.zeros((3, 8)))
        with pytest.raises(ValueError, match='no free shape block'):
            m.lbs_forward_device(3, 1, 2, 3, shape_ptr=4)


def test_lbs_forward_refuses_other_dtypes():
    with pytest.raises(ValueError, match='dtype'):
        _handleless_model().lbs_forward(np.zeros((3, 72)), np.zeros((3, 3)), dtype=np.float16)
