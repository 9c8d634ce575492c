"""CPU: the host-side planning of the Stage-II solve entries (moshpp_amd/csrc/solve_plan.h: chunk table, cooperative-group layout and
shares, repair scheduler) compiled on its own by g++ -- no HIP, no device -- and held to results worked out by hand from the
scheduler's rules."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "solve_plan.h"
#include <cstdio>
using namespace solve_plan;

static std::vector<Chunk> table(std::vector<int> per_seq) {   // chunks of 20 frames, s = 20 c, pred = c - 1 (-1 at a sequence's start)
    std::vector<Chunk> ch;
    for (int q = 0; q < (int)per_seq.size(); ++q)
        for (int i = 0; i < per_seq[q]; ++i) {
            const int c = (int)ch.size();
            ch.push_back(Chunk{q, 20 * c, 20 * c + 20, 20 * c, i == 0 ? -1 : c - 1});
        }
    return ch;
}
static void repairs(const char* name, std::vector<int> per_seq, bool rejoin, std::vector<std::pair<int, double>> set) {
    const std::vector<Chunk> ch = table(per_seq);
    std::vector<double> hdev(ch.size(), 0.0);
    for (auto& kv : set) hdev[kv.first] = kv.second;
    const Repairs r = pick_repairs(ch, hdev, 1e-9, rejoin, 160);
    printf("%s todo", name);
    for (int c : r.todo) printf(" %d", c);
    printf("\n%s gross", name);
    for (char g : r.gross) printf(" %d", (int)g);
    printf("\n");
}
static void split(const char* name, int M, int G, double frac) {
    int mlo[kMaxGroup + 1];
    coop_split(M, G, frac, mlo);
    printf("%s", name);
    for (int r = 0; r <= G; ++r) printf(" %d", mlo[r]);
    printf("\n");
}
static void chunks(const char* name, std::vector<int> frames, int want, int warmup, int n_cu) {
    const std::vector<Chunk> ch = chunk_table(frames, want, warmup, n_cu);
    printf("%s", name);
    for (const Chunk& c : ch) printf(" %d:%d:%d:%d:%d", c.seq, c.s, c.e, c.a, c.pred);
    printf("\n");
}
int main() {
    repairs("row1", {8}, true, {{2, 3e-8}});
    repairs("row2", {8}, true, {{2, 1e-3}, {3, 1e-2}, {5, 5e-8}});
    repairs("row3", {12}, true, {{1, 1e-3}, {10, 5e-8}});
    repairs("row4", {12}, true, {{1, 1e-3}, {9, 5e-8}, {10, 5e-8}});
    repairs("row5", {8}, true, {{3, MOSHII_HANDOFF_GIVEN_UP}, {4, MOSHII_HANDOFF_PRED_GIVEN_UP}, {5, 1e-3}});
    repairs("row6", {8}, true, {{2, MOSHII_HANDOFF_MISMATCH}, {3, 1e-3}});
    repairs("row7", {8}, false, {{2, 1e-3}, {3, 1e-3}, {5, 5e-8}});
    repairs("row8", {4, 4}, true, {{1, 1e-3}, {2, 5e-8}, {5, 5e-8}});
    printf("verdicts %d %d %d %d %d\n", (int)handoff_given_up(MOSHII_HANDOFF_GIVEN_UP), (int)handoff_given_up(MOSHII_HANDOFF_PRED_GIVEN_UP),
           (int)handoff_given_up(MOSHII_HANDOFF_MISMATCH), (int)handoff_given_up(MOSHII_HANDOFF_NAN), (int)handoff_given_up(1e-3));
    const CoopLayout a(4, 53, 6), b(4, 3000, 2);
    printf("layout_a %d %zu %zu %zu\n", a.slot_doubles, a.flags_offset, a.abort_offset, a.bytes_per_chain);
    printf("layout_b %d %zu %zu %zu\n", b.slot_doubles, b.flags_offset, b.abort_offset, b.bytes_per_chain);
    split("split_a", 53, 6, 0.0);
    split("split_b", 53, 2, 0.4);
    for (int M : {1, 2, 7, 33, 53, 128}) for (int G = 1; G <= kMaxGroup; ++G) for (double f : {0.0, 0.4, 0.5, 1.0}) {
        char name[64];
        snprintf(name, sizeof(name), "shares_%d_%d_%.1f", M, G, f);
        split(name, M, G, f);
    }
    chunks("auto_one", {4000}, 0, 32, 256);
    chunks("auto_two", {4000, 400}, 0, 32, 256);
    const int plans[][3] = {{4000, 256, 16}, {4000, 512, 16}, {10, 4, 16}, {3, 8, 2}, {1, 1, 0}, {0, 4, 16}, {97, 5, 0}};
    for (auto& p : plans) {
        char name[64];
        snprintf(name, sizeof(name), "plan_%d_%d_%d", p[0], p[1], p[2]);
        chunks(name, {p[0]}, p[1], p[2], 256);
    }
    std::vector<int32_t> st(10), ls(10);
    printf("capped %d\n", plan_chunks(100, 10, 4, 3, st.data(), ls.data()));
    printf("group %d %d %d %d\n", own_group_size(53, 20, true, false), own_group_size(53, 20, false, false), own_group_size(53, 20, true, true),
           own_group_size(33, 5, false, false));
    return 0;
}
'''


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    """The program's output lines, by their first word: compiled by g++ alone against the product header."""
    d = tmp_path_factory.mktemp('solve_plan')
    src, exe = d / 'plan.cpp', d / 'plan'
    src.write_text(PROGRAM)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'moshpp_amd', 'csrc'), str(src), '-o', str(exe)])
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        key, *rest = line.split()
        if rest and rest[0] in ('todo', 'gross'):
            key, rest = key + ' ' + rest[0], rest[1:]
        out[key] = rest
    return out


@pytest.mark.parametrize('row,todo,gross', [
    ('row1', [2], [0]),            # a lone slight miss
    ('row2', [2], [1]),            # a gross miss behind a gross miss is swept by the first; the slight miss inside the span waits
    ('row3', [1, 10], [1, 0]),     # a slight miss 180 frames behind the span start, clean predecessor: repaired at once
    ('row4', [1, 9], [1, 0]),      # ... chunk 10's predecessor is failing: chunk 10 waits
    ('row5', [3, 5], [1, 1]),      # the successor of a given-up chunk is skipped; a given-up predecessor does not hold back a gross miss
    ('row6', [2], [1]),            # a flag mismatch is not "given up": chunk 3 waits behind it
    ('row7', [2, 5], [0, 0]),      # without re-joining: one chunk per chain, only behind a clean predecessor
    ('row8', [1, 5], [1, 0]),      # the span ends with the sequence
])
def test_pick_repairs(plan, row, todo, gross):
    assert [int(v) for v in plan[row + ' todo']] == todo
    assert [int(v) for v in plan[row + ' gross']] == gross


def test_given_up_is_one_predicate(plan):
    assert plan['verdicts'] == ['1', '1', '0', '0', '0']


def test_coop_layout(plan):
    assert [int(v) for v in plan['layout_a']] == [6176, 592896, 592920, 593152]
    assert int(plan['layout_b'][0]) == 9034      # the marker term wins
    slot, flags, abort, per = (int(v) for v in plan['layout_b'])
    assert flags == 2 * 2 * slot * 8 and abort == flags + 2 * 4 and per % 256 == 0 and flags + (2 * 2 + 2) * 4 <= per < flags + (2 * 2 + 2) * 4 + 256


def test_coop_split(plan):
    assert [int(v) for v in plan['split_a']] == [0, 11, 21, 32, 42, 53, 53]
    assert [int(v) for v in plan['split_b']] == [0, 38, 53]
    shares = {k: [int(v) for v in vals] for k, vals in plan.items() if k.startswith('shares_')}
    assert len(shares) == 6 * 8 * 4
    for k, mlo in shares.items():
        M, G = int(k.split('_')[1]), int(k.split('_')[2])
        assert len(mlo) == G + 1 and mlo[0] == 0 and mlo[-1] == M and all(a <= b for a, b in zip(mlo, mlo[1:])), k


def _chunks(words):
    return [tuple(int(v) for v in w.split(':')) for w in words]   # (seq, s, e, a, pred)


def test_chunk_table(plan):
    """The moshii_plan_chunks properties (tests/test_capi_symbols.py) through the header's function, and the automatic count."""
    for key, words in plan.items():
        if not key.startswith('plan_'):
            continue
        F, C, W = (int(v) for v in key.split('_')[1:])
        ch = _chunks(words)
        n = len(ch)
        assert 1 <= n <= max(1, min(C, max(F, 1)))
        assert ch[0][1] == 0 and ch[0][3] == 0 and ch[-1][2] == F
        lens = [e - s for _, s, e, _, _ in ch]
        assert sum(lens) == F and min(lens) >= 0 and max(lens) - min(lens) <= 1
        assert all(ch[c][2] == ch[c + 1][1] for c in range(n - 1))
        assert all(ch[c][3] == max(0, ch[c][1] - W) for c in range(1, n))
        assert [c[4] for c in ch] == [-1] + list(range(n - 1)) and all(c[0] == 0 for c in ch)
    assert plan['capped'] == ['3']
    assert len(plan['auto_one']) == 250
    two = _chunks(plan['auto_two'])
    assert [sum(1 for c in two if c[0] == q) for q in (0, 1)] == [232, 23]
    assert [c[4] for c in two if c[1] == 0] == [-1, -1] and two[232][0] == 1 and two[233][4] == 232
    assert all(c[2] - c[1] >= 16 for c in two)   # min_len = max(4, warmup / 2)


def test_own_group_size(plan):
    """SMPL-H, 53 markers x 20 needed joints: five item ranks + the prior's; fewer than three ranks, or an unsuitable solve: plain."""
    assert plan['group'] == ['6', '5', '0', '0']
