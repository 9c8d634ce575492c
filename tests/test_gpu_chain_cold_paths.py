"""tests/chain_cold_paths.py's cases on the device: the hipcc build of the chain kernel's out-of-line cold paths (first-frame rigid
init with the cooperative marker gather, column tables and fixed-joint correctives rebuilt twice a frame, the chunk protocol at the
frame head), held to the oracle at 1e-7 with equal iteration counts; every sequential solve twice, bit for bit."""
import pytest

from tests import chain_cold_paths as cp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('fingers,G', cp.CHAIN_PARAMS)
def test_cold_start_chain_matches_oracle(gpu_lib, fingers, G):
    from moshpp_amd import capi
    kernel = cp.check_chain(capi, fingers, G, 12, 'gpu')
    assert kernel == 'k_chain_solve<%d,1%s>' % (8 if fingers else 4, f',coop{G}' if G else ''), kernel


@pytest.mark.parametrize('coop', [1, 3, 0])
def test_chunked_solve_with_a_short_warmup(gpu_lib, coop):
    from moshpp_amd import capi
    cp.check_chunked(capi, coop, 48, 6, 'gpu')
