"""The argument path every export of capi.Model shares, without a device: the six host methods that take pose / trans / shape refuse the
same faults with the same words and their own name in front, before any library call; the *_device methods refuse a shape buffer on a
model without a free block; every f32 / f64 pair of entries declares one argument list."""
import numpy as np
import pytest

from moshpp_amd import capi

NP, V, NSHAPE, F = 72, 100, 8, 3


def _handleless_model(nshape=NSHAPE):
    m = capi.Model.__new__(capi.Model)      # no device, no handle: anything that reached the library would fail on the null handle
    m.NP, m.V, m.K, m.handle, m.n_faces = NP, V, 24, None, 12
    if nshape is not None:
        m.n_free_shape = nshape
    return m


# method -> the call with (pose, trans, shape, dtype) filled in; everything else is valid and the same for every row
POSED = {
    'lbs_forward': lambda m, p, t, s, d: m.lbs_forward(p, t, dtype=d, shape=s),
    'virtual_markers': lambda m, p, t, s, d: m.virtual_markers(p, t, [1, 2], 0.01, dtype=d, shape=s),
    'marker_surface_distance': lambda m, p, t, s, d: m.marker_surface_distance(p, t, np.zeros((F, 2, 3)), shape=s, dtype=d),
    'posed_joints': lambda m, p, t, s, d: m.posed_joints(p, t, shape=s, dtype=d),
    'render_posed': lambda m, p, t, s, d: m.render_posed(p, t, capi.Camera.make(np.eye(3), [0, 0, 2], 64, 64, 4, 4, 0.1), (8, 8), shape=s, dtype=d),
    'lbs_forward_with_normals': lambda m, p, t, s, d: m.lbs_forward_with_normals(p, t, dtype=d, shape=s),
}
POSE, TRANS, SHAPE = np.zeros((F, NP)), np.zeros((F, 3)), np.zeros((F, NSHAPE))
# fault -> (nshape of the model, pose, trans, shape, dtype, the message behind the method's name; None: the shape rows say lbs_forward)
FAULTS = {
    'float16': (NSHAPE, POSE, TRANS, None, np.float16, 'dtype must be numpy float64 or float32, not '),
    'pose one column short': (NSHAPE, POSE[:, :-1], TRANS, None, np.float64, rf'pose / trans must be \[F, {NP}\] / \[F, 3\], got \({F}, {NP - 1}\) / \({F}, 3\)'),
    'trans rows': (NSHAPE, POSE, TRANS[:-1], None, np.float32, rf'pose / trans must be \[F, {NP}\] / \[F, 3\], got \({F}, {NP}\) / \({F - 1}, 3\)'),
    'shape without a block': (None, POSE, TRANS, SHAPE, np.float64, None),
    'shape width': (NSHAPE, POSE, TRANS, SHAPE[:, :-1], np.float32, None),
    'shape not finite': (NSHAPE, POSE, TRANS, np.full((F, NSHAPE), np.inf), np.float64, None),
}
SHAPE_ROWS = {      # _check_shape_rows names lbs_forward whichever method asks
    'shape without a block': r'lbs_forward: shape coefficients given, but the model has no free shape block \(set_free_shape\)',
    'shape width': rf'lbs_forward: shape must be \[F, nshape\] = \[{F}, {NSHAPE}\], got \({F}, {NSHAPE - 1}\)',
    'shape not finite': 'lbs_forward: shape holds non-finite coefficients',
}


@pytest.mark.parametrize('fault', sorted(FAULTS))
@pytest.mark.parametrize('method', sorted(POSED))
def test_posed_methods_refuse_alike_before_the_library(method, fault):
    nshape, pose, trans, shape, dtype, msg = FAULTS[fault]
    want = f'^{method}: {msg}' if msg is not None else '^' + SHAPE_ROWS[fault]
    with pytest.raises(ValueError, match=want):
        POSED[method](_handleless_model(nshape), pose, trans, shape, dtype)


def test_posed_methods_take_a_lone_frame():
    m = _handleless_model()
    pose, trans, shape, n = m._posed_inputs('x', np.zeros(NP), np.zeros(3), np.zeros(NSHAPE), np.float32)
    assert (pose.shape, trans.shape, shape.shape, n) == ((1, NP), (1, 3), (1, NSHAPE), 1)
    assert pose.dtype == trans.dtype == shape.dtype == np.float32 and pose.flags.c_contiguous


# the *_device methods that check the block in Python (virtual_markers_device leaves a shape buffer to the library's own refusal)
DEVICE = {
    'lbs_forward_device': lambda m: m.lbs_forward_device(F, 1, 2, 3, shape_ptr=4),
    'marker_surface_distance_device': lambda m: m.marker_surface_distance_device(F, 1, 2, 2, 3, 4, shape_ptr=5),
    'posed_joints_device': lambda m: m.posed_joints_device(F, 1, 2, 3, shape_ptr=4),
    'render_posed_device': lambda m: m.render_posed_device(F, 1, 2, None, (8, 8), rgb_ptr=3, shape_ptr=4),
}


@pytest.mark.parametrize('method', sorted(DEVICE))
def test_device_methods_refuse_a_shape_buffer_without_a_block(method):
    with pytest.raises(ValueError, match=rf'^{method}: shape_ptr given, but the model has no free shape block \(set_free_shape\)$'):
        DEVICE[method](_handleless_model(nshape=None))


def test_every_f32_f64_pair_declares_one_argument_list():
    pairs = [n[:-4] for n in capi.EXPORTS if n.endswith('_f32')]
    assert len(pairs) == 9 and all(p + '_f64' in capi.EXPORTS for p in pairs)
    assert sorted(n for n in capi.EXPORTS if n.endswith('_f64')) == sorted(p + '_f64' for p in pairs)
    for p in pairs:
        (r32, a32), (r64, a64) = capi.EXPORTS[p + '_f32'], capi.EXPORTS[p + '_f64']
        assert r32 is r64 and a32 == a64, p


def test_owners_close_once_and_quietly():
    class Lib:
        freed = []

        def moshii_model_destroy(self, h):
            self.freed.append(h.value)

    saved, capi._lib = capi._lib, Lib()
    try:
        m = _handleless_model()
        m.close()                                   # never held a handle: nothing to give back
        m.handle = capi.C.c_void_p(7)
        m.close(); m.close()
        assert Lib.freed == [7] and not m.handle
    finally:
        capi._lib = saved
