"""CPU: moshpp_amd/csrc/dev_mem.h on its own -- the owner of device allocations (DevArena), the host-buffer / device-buffer staging
helper (Staging) and the handles' grow-only Scratch -- through the stand-alone program tests/emu/dev_mem_check.cpp, compiled by g++
against the stand-in HIP runtime header (its hipMalloc counts calls and live allocations and fails the n-th on request).  The program
prints numbers; the expected ones follow from what each case does and are worked out beside it here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    exe = tmp_path_factory.mktemp('dev_mem') / 'dev_mem_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-Wno-psabi', '-I', os.path.join(ROOT, 'tests', 'emu', 'fakehip'),
                           '-I', os.path.join(ROOT, 'moshpp_amd', 'csrc'), '-I', os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'emu', 'dev_mem_check.cpp'), '-o', str(exe)])
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        key, *rest = line.split()
        out[key] = [float(v) for v in rest]
    return out


def test_arena_owns_what_it_hands_out(rows):
    # ok, 3 pointers owned (upload, zeros, the one-element alloc(0); upload of nothing allocates nothing), 3 live, 7 + 8 + 9 uploaded,
    # zeros are zero, alloc(0) is not null, upload(.., 0) is null; all gone with the arena
    assert rows['arena'] == [1, 3, 3, 24, 1, 1, 1]
    assert rows['arena_gone'] == [0]


def test_arena_moves_and_clears(rows):
    # live 3 (a: 2, b: 1); after c(move(a)): live 3, a owns 0, c owns 2; after b = move(c): b's one freed -> live 2, b owns 2, c owns 0;
    # after b.clear(): live 0; the cleared arena allocates again: owns 1
    assert rows['moves'] == [3, 3, 0, 2, 2, 2, 0, 0, 1]


def test_a_failed_allocation_is_sticky_and_nothing_leaks(rows):
    # not ok, both later pointers null, the one good pointer still owned and live, no hipMalloc tried after the failure
    assert rows['sticky'] == [0, 1, 1, 1, 1, 0]
    assert rows['sticky_cleared'] == [1, 0]


def test_staging_in_host_and_device_mode(rows):
    # host: rc 0, 4 allocations (two inputs, two outputs; the null optional arrays none), 4 live inside, 0 after; 2 * 1, 2 * 4, 30 + 1
    # copied back, the neighbour of the output untouched
    assert rows['staged_host'] == [0, 4, 4, 0, 2, 8, 31, -1]
    # device: rc 0 (every pointer passed through untouched, the null ones null), no allocation, results written in place
    assert rows['staged_device'] == [0, 0, 0, 8, 11]


@pytest.mark.parametrize('nth', [1, 2, 3, 4])
def test_staging_frees_everything_when_the_nth_allocation_fails(rows, nth):
    # the call reports it, nth - 1 temporaries lived inside, none after, and the host outputs were not written
    assert rows[f'staged_fail_{nth}'] == [1, nth - 1, 0, -5, -5]


def test_finish_copies_back_what_was_recorded_once(rows):
    assert rows['finish'] == [1.5, 2.5, 0]


def test_scratch_grows_keeps_and_frees(rows):
    # 64 KiB at first, kept for the second request (one allocation live), grown for the third; a failed growth reports MOSHII_ERR_HIP
    # through moshii_internal_fail and leaves an empty buffer, no allocation
    assert rows['scratch'] == [0, 65536, 0, 1, 0, 100000, -2, -2, 0, 0]
    assert rows['scratch_gone'] == [0]
    assert rows['end'] == [0]
