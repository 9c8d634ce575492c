// Host-side planning of moshii_chain_solve / moshii_sequence_solve: chunk table, cooperative-group choice, exchange-buffer layout and
// the repair scheduler.  Pure arithmetic -- C++17 and standard headers only, no HIP types, no environment, no globals -- so that it is
// tested on its own (tests/test_solve_plan.py).  moshii_dev.h includes it: the hand-off verdicts below are shared with the kernels.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

// What k_verify_chunks reports in a chunk's deviation word in place of a deviation (all above any tolerance; the order matters to
// the scheduler's range tests) ...
#define MOSHII_HANDOFF_NAN 2e300             // a NaN in a hand-off state: MOSHII_ERR_NUMERIC, repairing cannot make it verify
#define MOSHII_HANDOFF_MISMATCH 1e300        // the flag words differ (first-frame schedule pending / velocity term missing on one side)
#define MOSHII_HANDOFF_GIVEN_UP 5e299        // this chunk's pass-1 chain gave the chunk up (ChainDev::tail_done): re-solve it, nothing else is wrong
#define MOSHII_HANDOFF_PRED_GIVEN_UP 4e299   // the predecessor was given up: its sweep hands over at the boundary
#define MOSHII_HANDOFF_GIVEN_UP_MIN 1e299    // [this, MISMATCH): the two "given up" verdicts
// ... and the has_prev flag words of spoiled states (finite, matching nothing): the entry state of a chunk that has to be re-solved -- its
// pass-1 chain gave it up, or a repair chain was stopped inside it -- and the end state of a chunk that was given up
#define MOSHII_MARK_ENTRY_SPOILED (-1.0)
#define MOSHII_MARK_FINAL_SPOILED (-2.0)

namespace solve_plan {

inline bool handoff_given_up(double d) { return d >= MOSHII_HANDOFF_GIVEN_UP_MIN && d < MOSHII_HANDOFF_MISMATCH; }

constexpr int kThreads = 256;   // MOSHII_TPB
constexpr int kMaxGroup = 8;    // MOSHII_COOP_MAXG

// moshii_plan_chunks (arguments checked by the caller); returns the number of chunks
inline int plan_chunks(int32_t F, int32_t num_chunks, int32_t warmup, int32_t cap, int32_t* starts, int32_t* launch_starts) {
    int C = std::min<int64_t>(num_chunks, std::max(F, 1));
    C = std::min(C, cap);
    for (int c = 0; c < C; ++c) {
        starts[c] = (int32_t)(((int64_t)F * c) / C);                 // balanced: lengths differ by at most one frame
        launch_starts[c] = (c == 0) ? 0 : std::max(0, starts[c] - warmup);
    }
    return C;
}

// chunk [s, e) of sequence `seq`, launched from frame a <= s (warm-up); pred: index of the chunk before it in the sequence, or -1
struct Chunk { int seq, s, e, a, pred; };

// The chunks of a call, sequence after sequence.  want_total > 0: that many per sequence; else as many as fill the chip once
// (one workgroup per CU), each at least min_len frames long.
inline std::vector<Chunk> chunk_table(const std::vector<int>& frames, int want_total, int warmup, int n_cu) {
    std::vector<Chunk> chunks;
    int64_t Ftot = 0;
    for (int F : frames) Ftot += F;
    const int min_len = std::max(4, warmup / 2);
    const int64_t slots = n_cu;
    std::vector<int32_t> st, ls;
    for (int q = 0; q < (int)frames.size(); ++q) {
        const int F = frames[q];
        int C = want_total;
        if (C <= 0) {   // auto: fill the chip once, but keep chunks at least min_len frames long
            const int64_t share = std::max<int64_t>(1, (slots * F) / std::max<int64_t>(Ftot, 1));
            C = (int)std::max<int64_t>(1, std::min<int64_t>(share, F / min_len));
        }
        st.assign(std::max(C, 1), 0); ls.assign(std::max(C, 1), 0);
        C = plan_chunks(F, C, warmup, 1 << 20, st.data(), ls.data());
        for (int c = 0; c < C; ++c) {
            Chunk ck; ck.seq = q; ck.s = st[c]; ck.e = (c + 1 < C) ? st[c + 1] : F; ck.a = ls[c];
            ck.pred = (c == 0) ? -1 : (int)chunks.size() - 1;
            chunks.push_back(ck);
        }
    }
    return chunks;
}

// Cooperative chains: the markers [mlo[r], mlo[r + 1]) of rank r.  The ranks 0 .. G-2 get equal shares, the last rank -- which also
// evaluates the prior for the group -- `prior_frac` of one (MOSHII_COOP_PRIOR_FRAC; 1 without a prior).
inline void coop_split(int M, int G, double prior_frac, int* mlo) {
    const double w_last = (G > 1) ? prior_frac : 1.0;
    const double total = (G - 1) + w_last;
    double acc = 0.0;
    mlo[0] = 0;
    for (int r = 0; r < G; ++r) {
        acc += (r == G - 1) ? w_last : 1.0;
        mlo[r + 1] = (r == G - 1) ? M : std::min(M, (int)std::lround(M * acc / total));
        if (mlo[r + 1] < mlo[r]) mlo[r + 1] = mlo[r];
    }
}

// The library's own choice of a group size: one rank per round of (marker, joint) Jacobian items (256 threads build 256 of them at a
// time) plus one for the prior; 0 (plain chains) when that is fewer than three ranks (few items) or the caller finds the solve
// `unsuitable` (so small -- MANO -- that the exchanges cost what the split saves: measured; or no instantiation for it).
inline int own_group_size(int Mmax, int nkfmax, bool with_prior, bool unsuitable) {
    const int item_ranks = (Mmax * nkfmax + kThreads - 1) / kThreads;
    const int g = std::min(kMaxGroup, item_ranks + (with_prior ? 1 : 0));
    return (g < 3 || unsuitable) ? 0 : g;
}

// One chain's slice of the exchange buffer of a group of g workgroups (moshii_dev.h: CoopDev), nblk register blocks, at most Mmax markers:
// [2][g] slots of slot_doubles 8-byte words, then [g] posted-exchange words, the abort word, padding to 256 bytes.
struct CoopLayout {
    int slot_doubles = 0;
    size_t flags_offset = 0, abort_offset = 0, bytes_per_chain = 0;
    CoopLayout() = default;
    CoopLayout(int nblk, int Mmax, int g) {
        const int NE = nblk * (nblk + 1) / 2, NT = (NE + 3) / 4;
        // slot: accumulators (2 NT 16-byte units per thread), prior block + gradient ((NE + 2) / 2 units), or 3 M marker coordinates; + 32 granule words
        slot_doubles = std::max((4 * NT + 2 * ((NE + 2) / 2)) * kThreads, 3 * Mmax + 2) + 32;
        flags_offset = (size_t)2 * g * slot_doubles * sizeof(unsigned long long);
        abort_offset = flags_offset + g * sizeof(unsigned);
        bytes_per_chain = (flags_offset + (size_t)(2 * g + 2) * sizeof(unsigned) + 255) & ~size_t(255);
    }
};

// Scheduling of one round's repair chains from the verified hand-off deviations hdev[] (any mistake here only costs time: whatever
// ends up inconsistent fails the next verification).  A GROSS miss (> 1e-6) is a chunk whose fresh start sat in another basin: its
// repair chain may have to run through several chunks before it re-joins, so it owns everything up to the next gross miss.  A SLIGHT
// miss is a warm-up that had not quite converged: its chain re-joins within a few frames; slight misses that lie in a gross chain's
// span wait for the next round (they may be swept anyway), the others are repaired right away.
struct Repairs { std::vector<int> todo; std::vector<char> gross; };   // chunks that get a chain this round; is it a gross miss's
inline Repairs pick_repairs(const std::vector<Chunk>& chunks, const std::vector<double>& hdev, double tol, bool rejoin, int far_frames) {
    const int NC = (int)chunks.size();
    std::vector<char> failing(NC, 0);
    for (int c = 0; c < NC; ++c) failing[c] = chunks[c].pred >= 0 && !(hdev[c] <= tol);
    Repairs r;
    std::vector<int>& todo = r.todo;
    std::vector<char>& todo_gross = r.gross;
    const double gross_dev = 1e-6;
    // ... except when the slight miss lies far (>= far_frames) behind the start of the gross chain whose span it is in:
    // gross chains re-join within ~140 frames on every sequence looked at, so such a chunk is repaired right away and
    // bounds that chain (should the chain ever get there, the next round continues it).
    int seq = -1, span_start = 0;
    bool in_span = false;
    for (int c = 0; c < NC; ++c) {
        if (chunks[c].seq != seq) { seq = chunks[c].seq; in_span = false; }
        if (!failing[c]) continue;
        const int p = chunks[c].pred;
        // Chunks a pass-1 chain gave up in the launch's tail (ChainDev::tail_done) are re-solved like gross misses -- they are the hard
        // stretches, their sweeps run 30-70 frames -- but neither they nor their successors (the entry state stands against a spoiled
        // end state; the sweep hands over at the boundary) say anything about the chunks behind them: as predecessors they do not
        // hold back a gross miss's chain (they did: a cascade of one round per territory).
        const bool aftercut = hdev[c] == MOSHII_HANDOFF_PRED_GIVEN_UP, p_given_up = failing[p] && handoff_given_up(hdev[p]);
        const bool g = rejoin && hdev[c] > gross_dev, pg = rejoin && failing[p] && hdev[p] > gross_dev && !p_given_up;
        if (rejoin && aftercut) continue;
        if (!rejoin) { if (!failing[p]) { todo.push_back(c); todo_gross.push_back(0); } continue; }
        if (g) { if (!pg) { todo.push_back(c); todo_gross.push_back(1); in_span = true; span_start = chunks[c].s; } }
        else if (!in_span || (far_frames > 0 && chunks[c].s - span_start >= far_frames && !failing[p])) { todo.push_back(c); todo_gross.push_back(0); }
    }
    return r;
}

}  // namespace solve_plan
