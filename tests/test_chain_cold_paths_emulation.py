"""CPU: the chain kernel's out-of-line cold paths (tests/chain_cold_paths.py has the cases and the checker) in the emulation -- the
kernels compiled unchanged by g++, one fiber per GPU thread, the ranks of a cooperative chain on OS threads."""
import pytest

from tests import chain_cold_paths as cp
from tests.emu.emu_moshii import emulated_libmoshii


@pytest.mark.parametrize('fingers,G', cp.CHAIN_PARAMS)
def test_cold_start_chain_matches_oracle_in_emulation(monkeypatch, fingers, G):
    monkeypatch.setenv('HIPEMU_CONCURRENT', '1')
    with emulated_libmoshii() as capi:
        kernel = cp.check_chain(capi, fingers, G, 6, 'emulation')
    assert kernel == 'k_chain_solve<%d,1%s>' % (8 if fingers else 4, f',coop{G}' if G else ''), kernel


@pytest.mark.parametrize('coop', [1, 3, 0])
def test_chunked_solve_with_a_short_warmup_in_emulation(monkeypatch, coop):
    monkeypatch.setenv('HIPEMU_CONCURRENT', '1')
    with emulated_libmoshii() as capi:
        cp.check_chunked(capi, coop, 24, 4, 'emulation')


def test_prepare_launch_refuses_a_layout_without_the_control_block_distances(monkeypatch):
    """The guard where it sits: MOSHII_TEST_BREAK_LAYOUT (emulated build only) moves dgn and what follows it by two doubles between
    make_layout and the check in prepare_launch -- the solve is refused with the internal error, and goes through again without."""
    from moshpp_amd.capi import MoshiiError
    c = cp.chain_case(False, 0, 2)
    with emulated_libmoshii() as capi:
        case, vis, dev = cp.device(c)
        ch = [dict(attach=dev['attach'], obs=case['obs'], vis=vis, first=True)]
        monkeypatch.setenv('MOSHII_TEST_BREAK_LAYOUT', '1')
        with pytest.raises(MoshiiError, match=r'error -3: internal error: chain layout: the control vectors g, dsd, dgn, ddl, y are not LDJ doubles apart'):
            capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], ch)
        monkeypatch.delenv('MOSHII_TEST_BREAK_LAYOUT')
        out = capi.chain_solve_host(dev['model'], dev['prior'], dev['opts'], ch)[0]
    assert out['status'].tolist() == [0, 0]


def test_a_layout_without_the_control_block_distances_is_refused(tmp_path):
    """chain_layout_fault (moshii_dev.h), what prepare_launch asks before every launch: the kernel body reaches g, dsd, dgn, ddl, y, red,
    scal and colpid / colprior from one base each with compile-time distances.  A small g++ program builds the layout make_layout
    produces for those fields and moves one field at a time."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / 'layout_check.cpp'
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime.h>
#include "moshii_dev.h"
namespace hipemu { void register_dynamic_lds(double*, size_t) {} }   // (the stand-in header's LDS registration: nothing launches here)
static ChainLayout good(int nblk) {
    ChainLayout ly; memset(&ly, 0, sizeof(ly));
    const int L = 16 * nblk; ly.LDJ = L;
    ly.o_g = 1000; ly.o_dsd = ly.o_g + L; ly.o_dgn = ly.o_dsd + L; ly.o_ddl = ly.o_dgn + L; ly.o_y = ly.o_ddl + L;
    ly.o_red = ly.o_y + L; ly.o_scal = ly.o_red + 16; ly.i_colpid = 53; ly.i_colprior = 53 + L;
    return ly;
}
int main() {
    for (int nblk : {2, 4, 13}) {
        ChainLayout ly = good(nblk);
        printf("%d", chain_layout_fault(ly, nblk) == nullptr);
        printf(" %d", chain_layout_fault(ly, nblk + 1) != nullptr);          // another instantiation's stride
        int* moved[] = {&ly.o_dsd, &ly.o_dgn, &ly.o_ddl, &ly.o_y, &ly.o_red, &ly.o_scal, &ly.i_colprior, &ly.LDJ};
        for (int* f : moved) { *f += 2; printf(" %d", chain_layout_fault(ly, nblk) != nullptr); *f -= 2; }
        printf(" %d\n", chain_layout_fault(ly, nblk) == nullptr);
    }
    return 0;
}
''')
    exe = tmp_path / 'layout_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wno-psabi', '-I', os.path.join(root, 'tests', 'emu', 'fakehip'),
                           '-I', os.path.join(root, 'moshpp_amd', 'csrc'), '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)])
    rows = subprocess.check_output([str(exe)]).decode().split('\n')[:3]
    assert rows == ['1 1 1 1 1 1 1 1 1 1 1'] * 3, rows
