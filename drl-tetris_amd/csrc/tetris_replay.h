// Kernel bodies of the prioritised experience replay (include/tetris_hip.h: tetris_replay_add_dev, tetris_replay_sample_dev,
// tetris_replay_update_prios_dev, tetris_replay_gather_dev): the ring with its device-side cursor, rank-based sampling without
// replacement by exponential keys, and the pieces of the stable LSD radix sort both the ranks and the selection run on — the path
// through experience_replay.add_samples / add_indices / get_random_sample / update_prios (agents/agent_utils/
// experience_replay.py:42-74, 108-141).  The gather is tetris_batch.h's own (batch_entry with ba.steps > 0).
//
// `__host__ __device__` like tetris_batch.h: tetris_hip.hip wraps these in gfx950 kernels (k_replay_*, k_sort_*:
// tetris_dev_replay.h), tests/cpu_harness/harness_lib_agent.h in plain host loops, tile by tile.
#pragma once
#include <math.h>

#include "tetris_batch.h"

namespace te {

constexpr int SORT_THREADS = 256;                            // threads per workgroup of the sort's kernels: four waves
constexpr int SORT_ITEMS = 8;                                // entries per lane
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS;         // entries per workgroup: wave w holds entries [512 w, 512 w + 512)
constexpr int SORT_RADIX = 256;                              // 8-bit digits, four passes
constexpr int SORT_SCAN_SPAN = SORT_THREADS;                 // tiles per trip of k_sort_scan: past that many the scan carries
constexpr uint32_t SORT_PAD = 0xFFFFFFFFu;                   // the key of positions at and past n
constexpr int REPLAY_MAX_SIZE = 1 << 24;                     // a rank stays exact as a float32

// the buffer, as the kernels see it
struct ReplayRing {
    int capacity, k_step, max_size, n_slots;
    uint32_t* obs;                  // [C][S][12]
    uint8_t* action;                // [C][4]
    float *prob, *adv, *target, *reward;
    uint8_t *done, *flags;
    float* prio;                    // [max_size]
    int32_t* cursor;                // [4]: current_idx, current_size, samples added modulo 2^32, entries dropped
};

// ---- add ---------------------------------------------------------------------------------------------------------------------
struct ReplayAddArgs {
    ReplayRing rp;
    int n, rows, augment;
    const uint8_t* mask;            // [rows][N]
    const uint32_t* obs;            // the window: [T][N][S][12]
    const uint8_t* action;          // [T][N][4]
    const float *prob, *reward;     // [T][N]
    const uint8_t* done;            // [T][N]
    const float *adv, *target;      // [T][N] or NULL: zeros
    const float* prio;              // [T][N] or NULL: 2.0f
    uint32_t* offsets;              // scratch [N + 1]: entries per game, then their exclusive scan; [N]: the position of entry 0
};

// the non-zero mask bytes of game g
TE_HD uint32_t replay_add_count(const ReplayAddArgs& aa, int g) {
    uint32_t c = 0u;
    for (int t = 0; t < aa.rows; t++) c += aa.mask[(size_t)t * aa.n + g] != 0 ? 1u : 0u;
    return c;
}
// add_indices (experience_replay.py:130-138), applied once to the k entries of a call -> the position of entry 0.  Entries whose
// position would reach max_size (k > max_size only) are not written: they count as dropped.
TE_HD uint32_t replay_cursor_rule(int32_t* cur, uint32_t k, uint32_t max_size) {
    uint32_t idx = (uint32_t)cur[0], size = (uint32_t)cur[1];
    if (idx > max_size) idx = max_size;             // (a cursor the caller filled with nonsense leaves no array either)
    if (size > max_size) size = max_size;
    if ((uint64_t)idx + k > max_size) { size = idx; idx = 0u; }
    const uint32_t start = idx;
    const uint32_t written = k > max_size ? max_size : k;
    idx += written;
    if (idx > size) size = idx;
    cur[0] = (int32_t)idx; cur[1] = (int32_t)size;
    cur[2] = (int32_t)((uint32_t)cur[2] + k);
    cur[3] = (int32_t)((uint32_t)cur[3] + (k - written));
    return start;
}
// one entry of the window -> ring position pos
TE_HD void replay_add_entry(const ReplayAddArgs& aa, size_t at, uint32_t pos, uint32_t flag) {
    const ReplayRing& rp = aa.rp;
    if (pos >= (uint32_t)rp.max_size) return;
    const Quad* src = reinterpret_cast<const Quad*>(aa.obs + at * (size_t)rp.n_slots * OBS_WORDS);
    Quad* dst = reinterpret_cast<Quad*>(rp.obs + (size_t)pos * (size_t)rp.n_slots * OBS_WORDS);
    for (int q = 0; q < 3 * rp.n_slots; q++) dst[q] = src[q];
    for (int k = 0; k < 4; k++) rp.action[(size_t)pos * 4 + k] = aa.action[at * 4 + k];
    rp.prob[pos] = aa.prob[at];
    rp.reward[pos] = aa.reward[at];
    rp.adv[pos] = aa.adv ? aa.adv[at] : 0.0f;
    rp.target[pos] = aa.target ? aa.target[at] : 0.0f;
    rp.done[pos] = aa.done[at];
    rp.flags[pos] = (uint8_t)flag;
    rp.prio[pos] = aa.prio ? aa.prio[at] : 2.0f;           // the reference's "very large prio" (trajectory.py:82)
}
// game g's run, in ascending t, and with augment the same run once more with the flag set, directly behind it
TE_HD void replay_add_game(const ReplayAddArgs& aa, int g) {
    const uint32_t first = aa.offsets[aa.n] + aa.offsets[g];
    uint32_t run = 0u;
    if (aa.augment) run = replay_add_count(aa, g);
    uint32_t o = 0u;
    for (int t = 0; t < aa.rows; t++) {
        const size_t at = (size_t)t * aa.n + g;
        if (aa.mask[at] == 0) continue;
        replay_add_entry(aa, at, first + o, 0u);
        if (aa.augment) replay_add_entry(aa, at, first + run + o, 1u);
        o++;
    }
}

// ---- the sort ----------------------------------------------------------------------------------------------------------------
// a float's bits -> an unsigned key of the same order; -0.0 is +0.0
TE_HD uint32_t sort_float_key(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
TE_HD uint32_t sort_digit(uint32_t key, int pass) { return (key >> (8 * pass)) & 255u; }

// One pass: (key_in, pos_in) -> (key_out, pos_out) by digit `pass`, stable.  hist [256][ntiles] digit-major: the tiles' counts
// of a digit, then their exclusive scan along the tiles; totals [256]: the digits' counts.  An entry's place is
// (digits below it: sum of totals) + hist[digit][tile] + (entries of its digit before it in the tile).
struct SortArgs {
    uint32_t total;                 // entries (max_size)
    int ntiles, pass;
    const uint32_t *key_in, *pos_in;
    uint32_t *key_out, *pos_out;
    uint32_t *hist, *totals;
};
// serial forms (CPU harness; the kernels count with LDS atomics, scan by workgroup and rank with wave ballots)
TE_HD void sort_tile_histogram(const SortArgs& sa, int tile) {
    uint32_t cnt[SORT_RADIX];
    for (int d = 0; d < SORT_RADIX; d++) cnt[d] = 0u;
    const uint32_t first = (uint32_t)tile * SORT_TILE;
    for (uint32_t e = first; e < first + SORT_TILE && e < sa.total; e++) cnt[sort_digit(sa.key_in[e], sa.pass)]++;
    for (int d = 0; d < SORT_RADIX; d++) sa.hist[(size_t)d * sa.ntiles + tile] = cnt[d];
}
TE_HD void sort_scan_digit(const SortArgs& sa, int d) {
    uint32_t carry = 0u;
    uint32_t* row = sa.hist + (size_t)d * sa.ntiles;
    for (int t = 0; t < sa.ntiles; t++) { const uint32_t c = row[t]; row[t] = carry; carry += c; }
    sa.totals[d] = carry;
}
TE_HD void sort_tile_scatter(const SortArgs& sa, int tile) {
    uint32_t at[SORT_RADIX];
    uint32_t below = 0u;
    for (int d = 0; d < SORT_RADIX; d++) { at[d] = below + sa.hist[(size_t)d * sa.ntiles + tile]; below += sa.totals[d]; }
    const uint32_t first = (uint32_t)tile * SORT_TILE;
    for (uint32_t e = first; e < first + SORT_TILE && e < sa.total; e++) {
        const uint32_t key = sa.key_in[e], dst = at[sort_digit(key, sa.pass)]++;
        if (dst < sa.total) { sa.key_out[dst] = key; sa.pos_out[dst] = sa.pos_in[e]; }
    }
}

// ---- sample ------------------------------------------------------------------------------------------------------------------
struct ReplaySampleArgs {
    uint32_t max_size;
    int m;
    const float* prio;              // [max_size]
    const int32_t* cursor;
    float alpha, alpha_beta;        // (alpha * beta rounded once, on the host)
    uint32_t seed, draw_lo, draw_hi;
    uint32_t *key_a, *pos_a, *key_b, *pos_b;       // the sort's two pairs
    int32_t* rank;                  // scratch [max_size]
    int32_t *index, *count;         // [M], [1]
    float* weight;                  // [M]
    int32_t* rank_out;              // [max_size] or NULL
    float* key_out;                 // [max_size] or NULL
};
TE_HD uint32_t replay_size(const int32_t* cursor, uint32_t max_size) {
    const int32_t n = cursor[1];
    return n < 0 ? 0u : ((uint32_t)n > max_size ? max_size : (uint32_t)n);
}
// position i -> the first sort's input: the priority's key, or the pad at and past n
TE_HD void replay_prio_key(const ReplaySampleArgs& sa, uint32_t i) {
    const uint32_t n = replay_size(sa.cursor, sa.max_size);
    sa.key_a[i] = i < n ? sort_float_key(f2u(sa.prio[i])) : SORT_PAD;
    sa.pos_a[i] = i;
}
// slot s of the priorities' sorted order -> rank, sampling key and the second sort's input of the position it holds
TE_HD void replay_sample_key(const ReplaySampleArgs& sa, uint32_t s) {
    const uint32_t n = replay_size(sa.cursor, sa.max_size);
    uint32_t i = sa.pos_a[s];
    if (i >= sa.max_size) return;                                   // (never: the sort permutes 0 .. max_size - 1)
    if (s >= n) { sa.key_b[i] = SORT_PAD; sa.pos_b[i] = i; return; }   // (the pads keep their order: positions n .. max_size - 1)
    const uint32_t rank = n - s;                                    // 1 + n - ordinal rank, ordinal rank = s + 1
    const float w = powf((float)rank, -sa.alpha);
    uint32_t r[4];
    philox4x32_10(sa.seed, i, sa.draw_lo, sa.draw_hi, r);
    const float u = (float)((r[0] >> 8) + 1u) * 5.9604644775390625e-08f;      // (0, 1], exact
    const float key = (-logf(u)) / w;
    sa.rank[i] = (int32_t)rank;
    if (sa.rank_out) sa.rank_out[i] = (int32_t)rank;
    if (sa.key_out) sa.key_out[i] = key;
    sa.key_b[i] = sort_float_key(f2u(key));
    sa.pos_b[i] = i;
}
// output j from the sampling keys' sorted order (in pair b after the second sort)
TE_HD void replay_emit(const ReplaySampleArgs& sa, int j) {
    const uint32_t n = replay_size(sa.cursor, sa.max_size);
    const uint32_t c = (uint32_t)sa.m < n ? (uint32_t)sa.m : n;
    if (j == 0) sa.count[0] = (int32_t)c;
    uint32_t i = (uint32_t)j < c ? sa.pos_b[j] : sa.max_size;
    if (i >= sa.max_size) { sa.index[j] = -1; sa.weight[j] = 0.0f; return; }
    sa.index[j] = (int32_t)i;
    sa.weight[j] = powf((float)sa.rank[i] / (float)n, sa.alpha_beta);
}

// ---- update_prios ------------------------------------------------------------------------------------------------------------
struct ReplayUpdateArgs {
    float* prio;                    // [max_size]
    uint32_t max_size;
    const int32_t* index;           // [M]
    const float* value;             // [M]
    int m;
};
TE_HD void replay_update(const ReplayUpdateArgs& ua, int j) {
    const uint32_t i = (uint32_t)ua.index[j];
    if (i < ua.max_size) ua.prio[i] = ua.value[j];
}

}  // namespace te
