"""tests/chain_edges.py's table on the CPU: the Stage-II kernels compiled unchanged by g++ (tests/emu), every case held to the oracle
with equal iteration counts; and what the library refuses at the ends of the size classes."""
import pytest

from moshpp_amd.capi import MoshiiError
from tests import chain_edges as ce
from tests.emu.emu_moshii import emulated_libmoshii
from tests.helpers import device_case


@pytest.mark.parametrize('name', [n for n in ce.names() if n not in ce.TM_NAMES])
def test_chain_edge_matches_oracle_in_emulation(monkeypatch, name):
    if ce.CASES[name]['G']:
        monkeypatch.setenv('HIPEMU_CONCURRENT', '1')      # a cooperative group's workgroups on OS threads of their own
    with emulated_libmoshii() as capi:
        ce.check_case(capi, name, 'emulation')


def test_marker_tile_height_switch_in_emulation():
    with emulated_libmoshii() as capi:
        ce.check_tile_switch(capi, 'emulation')


def _solve(capi, c, ids, **kw):
    case, vis = ce.inputs(c)
    dev = device_case(case, id_sets=ids, **kw)
    return capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], [dict(attach=dev['attach'], obs=case['obs'], vis=vis, first=True)], coop=1)[0]


@pytest.mark.parametrize('name,forced', [('A-n16', 3), ('A-n63', 6), ('A-n63', 9)])
def test_forced_block_count_without_an_instantiation_is_an_error_before_any_launch(monkeypatch, name, forced):
    """MOSHII_FORCE_NBLK names a block count no k_chain_solve was built for: the call returns an error code (the launcher finds no
    kernel: MOSHII_ERR_HIP, invalid argument) and nothing is launched -- last_launch_info() still names the solve before it."""
    c = ce.CASES[name]
    with emulated_libmoshii() as capi:
        ce.check_case(capi, 'A-n127', 'emulation')        # leaves a launch of another instantiation on record
        before = capi.last_launch_info()
        assert before[0] == 'k_chain_solve<8,1>'
        monkeypatch.setenv('MOSHII_FORCE_NBLK', str(forced))
        with pytest.raises(MoshiiError, match=r'libmoshii error -2: moshii_launch_chain_solve'):
            _solve(capi, c, ce.id_sets_of(c), optimize_fingers=True)
        assert capi.last_launch_info() == before


def test_more_unknowns_than_the_largest_instantiation_holds_are_refused():
    """125 free pose variables (128 unknowns) in the plain variant, 208 unknowns in the extended one: MOSHII_ERR_UNSUPPORTED, no launch;
    one fewer is solved (A-n127 and C-n207 of the table)."""
    c = ce.CASES['A-n127']
    with emulated_libmoshii() as capi:
        ce.check_case(capi, 'A-n16', 'emulation')
        before = capi.last_launch_info()
        finger = list(range(66, 125))
        ids = (ce.BODY, finger, list(range(66)), list(range(125)))
        with pytest.raises(MoshiiError) as e:
            _solve(capi, c, ids, optimize_fingers=True)
        assert str(e.value) == 'libmoshii error -3: more than 124 free pose variables per step'
        assert capi.last_launch_info() == before
        x = dict(ce.CASES['C-n207'], E=94)
        case, vis = ce.inputs(x)
        assert ce.n_unknowns(x) == (63, 208)
        dev = device_case(case, optimize_fingers=True, optimize_face=True, shape_kind='expr')
        with pytest.raises(MoshiiError) as e:
            capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], [dict(attach=dev['attach'], obs=case['obs'], vis=vis, first=True)], coop=1)
        assert str(e.value) == 'libmoshii error -3: more than 207 unknowns per step'
        assert capi.last_launch_info() == before


def test_the_table_names_every_case_the_edges_ask_for():
    """The table itself: every n2 of the sweep with the instantiation written out for it, n1 / n2 as the id lists really give them."""
    for n2, nblk in ce.A_KERNEL.items():
        c = ce.CASES[f'A-n{n2}']
        assert ce.n_unknowns(c)[1] == n2 and c['kernel'] == f'k_chain_solve<{nblk},1>'
        assert nblk == next(b for top, b in ce.NBLK_PLAIN if n2 <= top)
    for n1, n2 in ((64, 97), (48, 81), (16, 33), (80, 113)):
        assert ce.n_unknowns(ce.CASES[f'A-n{n1}-n{n2}']) == (n1, n2)
    for n in (79, 80, 127, 128, 159, 160, 207):
        c = ce.CASES[f'C-n{n}']
        assert ce.n_unknowns(c)[1] == n and c['kernel'] == 'k_chain_solve<%d,1,xt>' % next(b for top, b in ce.NBLK_XT if n <= top)
    assert len(set(ce.INSTANTIATIONS)) == 17                 # ... and all 17 instantiations among the kernels the cases expect
    assert {ce.instantiation(c['kernel']) for c in ce.CASES.values()} == set(ce.INSTANTIATIONS)
