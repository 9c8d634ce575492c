"""CPU: the batch planning of the entries that export meshes into the handle's scratch (moshpp_amd/csrc/export_plan.h, used by
moshii_virtual_markers_* and moshii_marker_surface_distance_*) compiled on its own by g++ -- no HIP, no device -- and held to numbers
worked out by hand from its rules:

  batch    = 268435456 / frame_bytes (at least 1), cut to whole 128-frame tiles once it reaches 128; the override replaces it;
             then no more than F, no more than 2147483647 / items, and in f64 no more than 65535;
  off_vids = off_win = batch * frame_bytes rounded up to 16;  off_dist = (off_vids + 4 items) rounded up to 16;
  vm_bytes = off_dist + 8 items;  sd_bytes_face = off_win;  sd_bytes = off_win + 4 batch items.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "export_plan.h"
#include <cstdio>
static void row(const char* name, size_t frame_bytes, long long F, long long items, bool f64, int ov) {
    const export_plan::Batch b = export_plan::plan_batch(frame_bytes, F, items, f64, ov);
    printf("%s %lld %zu %zu %zu %zu %zu %zu\n", name, b.batch, b.off_vids, b.off_dist, b.vm_bytes, b.off_win, b.sd_bytes_face, b.sd_bytes);
}
int main() {
    row("smplh_f32", 6890 * 3 * 4, 4000, 53, false, 0);
    row("smplh_f64", 6890 * 3 * 8, 4000, 53, true, 0);
    row("short", 6890 * 3 * 4, 100, 53, false, 0);
    row("no_tiles", 250000 * 3 * 4, 1000, 10, false, 0);
    row("huge_frame", 300000000, 7, 5, false, 0);
    row("override", 6890 * 3 * 4, 5, 53, false, 2);
    row("override_beyond_F", 6890 * 3 * 4, 5, 53, false, 8);
    row("items_clamp", 12, 10, 1000000000, false, 0);
    row("grid_cap_f64", 24, 100000, 3, true, 0);
    row("grid_cap_f32", 12, 100000, 3, false, 0);
    row("odd_sizes", 778 * 3 * 4, 3, 3, false, 0);
    return 0;
}
'''


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    """The program's output rows by name: compiled by g++ alone against the product header."""
    d = tmp_path_factory.mktemp('export_plan')
    src, exe = d / 'plan.cpp', d / 'plan'
    src.write_text(PROGRAM)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'moshpp_amd', 'csrc'), str(src), '-o', str(exe)])
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        key, *rest = line.split()
        out[key] = dict(zip(('batch', 'off_vids', 'off_dist', 'vm_bytes', 'off_win', 'sd_bytes_face', 'sd_bytes'), (int(v) for v in rest)))
    return out


# name -> (batch, off_vids, off_dist, vm_bytes, sd_bytes); off_win and sd_bytes_face equal off_vids in every row
EXPECTED = {
    # 82 680 bytes a frame: 268435456 / 82680 = 3246.7 -> 3246 -> 25 tiles = 3200 frames; 3200 * 82680 = 264 576 000 = 16 * 16 536 000;
    # + 53 * 4 = 264 576 212 -> 264 576 224; + 53 * 8 = 264 576 648.  Winners: 3200 * 53 * 4 = 678 400.
    'smplh_f32': (3200, 264576000, 264576224, 264576648, 265254400),
    # 165 360 bytes: 1623.3 -> 1623 -> 12 tiles = 1536 (< 65535); 1536 * 165360 = 253 992 960 = 16 * 15 874 560; + 212 = 253 993 172
    # -> 253 993 184; + 424 = 253 993 608.  Winners: 1536 * 53 * 4 = 325 632.
    'smplh_f64': (1536, 253992960, 253993184, 253993608, 254318592),
    # F = 100 below the 3200: 100 * 82680 = 8 268 000 = 16 * 516 750; + 212 -> 8 268 224; + 424; winners 100 * 53 * 4 = 21 200
    'short': (100, 8268000, 8268224, 8268648, 8289200),
    # 3 000 000 bytes a frame (> 268435456 / 128 = 2 097 152): 89.5 -> 89 frames, below a tile, so no rounding; 267 000 000 =
    # 16 * 16 687 500; + 40 -> 267 000 048; + 80; winners 89 * 10 * 4 = 3560
    'no_tiles': (89, 267000000, 267000048, 267000128, 267003560),
    # a frame beyond the whole budget: one frame a batch; 300 000 000 = 16 * 18 750 000; + 20 -> 300 000 032; + 40; winners 1 * 5 * 4
    'huge_frame': (1, 300000000, 300000032, 300000072, 300000020),
    # MOSHII_VM_BATCH = 2: 2 * 82680 = 165 360 = 16 * 10 335; + 212 = 165 572 -> 165 584; + 424; winners 2 * 53 * 4 = 424
    'override': (2, 165360, 165584, 166008, 165784),
    # ... = 8 with F = 5: F wins; 5 * 82680 = 413 400 -> 413 408 (= 16 * 25 838); + 212 = 413 620 -> 413 632; + 424; winners 1060
    'override_beyond_F': (5, 413408, 413632, 414056, 414468),
    # 10^9 items: 2147483647 / 10^9 = 2 binds (the budget gives 22 369 536, F 10); 2 * 12 = 24 -> 32; + 4 * 10^9 = 4 000 000 032 =
    # 16 * 250 000 002; + 8 * 10^9; winners 2 * 10^9 * 4
    'items_clamp': (2, 32, 4000000032, 12000000032, 8000000032),
    # f64, 24 bytes a frame: budget 11 184 768 frames, F 100 000, grid.y 65 535 binds; 65535 * 24 = 1 572 840 -> 1 572 848 (16 * 98 303);
    # + 12 = 1 572 860 -> 1 572 864; + 24; winners 65535 * 3 * 4 = 786 420
    'grid_cap_f64': (65535, 1572848, 1572864, 1572888, 2359268),
    # the same body in f32 has no such cap: F binds; 100000 * 12 = 1 200 000 = 16 * 75 000; + 12 -> 1 200 016; + 24; winners 1 200 000
    'grid_cap_f32': (100000, 1200000, 1200016, 1200040, 2400000),
    # MANO, 9336 bytes a frame, 3 frames, 3 items: neither 3 * 9336 = 28 008 nor 3 * 4 = 12 is a multiple of 16:
    # 28 008 -> 28 016; + 12 = 28 028 -> 28 032; + 24; winners 3 * 3 * 4 = 36
    'odd_sizes': (3, 28016, 28032, 28056, 28052),
}


@pytest.mark.parametrize('name', sorted(EXPECTED))
def test_batch_and_scratch_layout(plan, name):
    batch, off_vids, off_dist, vm_bytes, sd_bytes = EXPECTED[name]
    got = plan[name]
    print(name, got)
    assert got == dict(batch=batch, off_vids=off_vids, off_dist=off_dist, vm_bytes=vm_bytes, off_win=off_vids, sd_bytes_face=off_vids,
                       sd_bytes=sd_bytes)
    assert got['off_vids'] % 16 == 0 and got['off_dist'] % 16 == 0


def test_every_case_was_planned(plan):
    assert sorted(plan) == sorted(EXPECTED)
