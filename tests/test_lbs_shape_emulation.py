"""CPU: the full-mesh export with per-frame coefficients of a free shape block (moshii_lbs_forward_shape_f32 / _f64) in the emulation
build -- lbs_forward.hip and moshii_api.hip compiled unchanged for the host.  Reference: the oracle's verts_forward(..., shp=) after
set_free_shape.  The f32 export's shape columns are hi + lo f16 pairs in front of the pose features; its bound
stays 2e-5 m against the f64 kernel, the f64 kernel's 1e-12 m against the oracle."""
import numpy as np
import pytest

from tests.emu.emu_moshii import emulated_libmoshii
from tests.lbs_shape_common import F32_TOL, F64_TOL, block_case, block_device, export_inputs, oracle_verts


def _check(dev, case, pose, trans, shape):
    ref = dev['model'].lbs_forward(pose, trans, shape=shape)
    got = dev['model'].lbs_forward(pose, trans, dtype=np.float32, shape=shape)
    again = dev['model'].lbs_forward(pose, trans, dtype=np.float32, shape=shape)
    orc = oracle_verts(case['m'], pose, trans, shape)
    e64, e32 = np.abs(ref - orc).max(), np.abs(got - ref).max()
    print(f'f64 kernel vs oracle {e64:.2e} m, f32 export vs f64 kernel {e32:.2e} m')
    assert e64 < F64_TOL
    assert e32 < F32_TOL
    np.testing.assert_array_equal(got, again)
    return got


# (model, E, F, vertex order, still from, coefficients)
CASES = [('mano', 5, 140, 'mesh', None, 'random'),        # two frame tiles
         ('smpl', 8, 17, 'shuffled', None, 'random'),
         ('smpl', 33, 18, 'shuffled', None, 'random'),    # 99 shape columns: three whole k-steps and 3 columns of a fourth
         ('smpl', 8, 19, 'shuffled', 30, 'random'),       # still joints, moving coefficients
         ('smpl', 8, 17, 'mesh', None, 'constant'),       # the same coefficients in every frame
         ('mano', 5, 16, 'shuffled', None, 'zero')]       # a block that does nothing


@pytest.mark.parametrize('model_type,E,F,order,still,coef', CASES)
def test_shape_export_matches_oracle_and_f64_in_emulation(model_type, E, F, order, still, coef):
    case = block_case(model_type, E, order=order)
    pose, trans, shape = export_inputs(case, F, still=still)
    if coef == 'constant':
        shape[:] = shape[0]
    elif coef == 'zero':
        shape[:] = 0.0
    with emulated_libmoshii():
        dev = block_device(case)
        got = _check(dev, case, pose, trans, shape)
        if coef == 'zero':      # ... equals the frozen body to the export's own precision
            assert np.abs(got - dev['model'].lbs_forward(pose, trans)).max() < F32_TOL
        else:                   # the block matters: without it the mesh is millimetres away
            assert np.abs(got - oracle_verts(case['m'], pose, trans)).max() > 1e-3


def test_plain_export_keeps_its_bits_after_a_shape_export_in_emulation():
    """A call without `shape` on a handle with a declared block runs the code it always ran: same bits before and after a shape call
    (which leaves the shared per-call scratch in the extended layout)."""
    case = block_case('smpl', 8)
    pose, trans, shape = export_inputs(case, 17)
    with emulated_libmoshii():
        dev = block_device(case)
        before = dev['model'].lbs_forward(pose, trans, dtype=np.float32)
        with_shape = dev['model'].lbs_forward(pose, trans, dtype=np.float32, shape=shape)
        after = dev['model'].lbs_forward(pose, trans, dtype=np.float32)
        ref = dev['model'].lbs_forward(pose, trans)
    np.testing.assert_array_equal(before, after)
    assert np.abs(before - ref).max() < F32_TOL and np.abs(with_shape - before).max() > 1e-3


def test_another_block_size_on_a_handle_that_has_exported_in_emulation():
    """set_free_shape invalidates the f32 export's prepared state: fragments, scales and scratch follow the new block."""
    from oracle import stageii_oracle as so
    case = block_case('smpl', 33)
    pose, trans, shape = export_inputs(case, 17)
    with emulated_libmoshii():
        dev = block_device(case)
        _check(dev, case, pose, trans, shape)
        for start, E in ((20, 4), (16, 33)):
            so.set_free_shape(case['m'], start, E)
            dev['model'].set_free_shape(start, E)
            _check(dev, case, pose, trans, shape[:, :E])
        dev['model'].set_free_shape(0, 0)
        with pytest.raises(ValueError):
            dev['model'].lbs_forward(pose, trans, dtype=np.float32, shape=shape)
        from moshpp_amd import capi
        p32, t32, s32 = (np.ascontiguousarray(a, dtype=np.float32) for a in (pose, trans, shape))
        out = np.zeros((17, dev['model'].V, 3), dtype=np.float32)
        rc = capi.load().moshii_lbs_forward_shape_f32(dev['model'].handle, 17, p32.ctypes.data, t32.ctypes.data, s32.ctypes.data,
                                                      out.ctypes.data, capi.BUFFERS_HOST, None)
        assert rc == -1      # a row without a block: MOSHII_ERR_ARG
        plain = dev['model'].lbs_forward(pose, trans, dtype=np.float32)
        assert np.abs(plain - dev['model'].lbs_forward(pose, trans)).max() < F32_TOL
