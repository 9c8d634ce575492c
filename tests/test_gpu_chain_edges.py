"""tests/chain_edges.py's table on the device: the hipcc build of k_chain_solve (DPP row broadcasts, v_readlane pivots, matrices passed
as register vectors, the f64 matrix instruction of ldl_big) at the edges of every size class, held to the oracle at TIGHT = 1e-7 with
equal iteration counts; every solve twice, bit for bit."""
import pytest

from tests import chain_edges as ce

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', [n for n in ce.names() if n not in ce.TM_NAMES])
def test_chain_edge_matches_oracle(gpu_lib, name):
    from moshpp_amd import capi
    ce.check_case(capi, name, 'gpu')


def test_marker_tile_height_switch(gpu_lib):
    from moshpp_amd import capi
    ce.check_tile_switch(capi, 'gpu')


def test_every_instantiation_was_asserted(gpu_lib):
    """Runs last in the file: the kernel names the cases above asserted from last_launch_info() cover all 17 instantiations of
    chain_solve.hip (a cooperative case also runs, and names, its plain chain)."""
    from moshpp_amd import capi
    if len(ce.ASSERTED_KERNELS) < 10:                       # (selected on its own: run the table first)
        for name in ce.names():
            ce.check_case(capi, name, 'gpu')
    seen = sorted({ce.instantiation(k) for k in ce.ASSERTED_KERNELS})
    print('kernel names asserted:', sorted(ce.ASSERTED_KERNELS))
    print('instantiations:', seen)
    print('worst deviation from the oracle per family:', {f: f'{d:.2e}' for f, d in ce.worst_per_family('gpu').items()})
    assert set(seen) == set(ce.INSTANTIATIONS), sorted(set(ce.INSTANTIATIONS) - set(seen))
