// Kernel bodies of a trajectory window's states and sample sets (include/tetris_hip.h: tetris_traj_observe_dev,
// tetris_traj_select_dev, tetris_traj_batch_dev): the packed observation record of a row, the ordered list of a mask's entries,
// and the expansion of a minibatch of entries, mirrored or not, into the arrays a trainer consumes — the path through
// sventon_trajectory.process_trajectory(augment=...) and augment_data (agents/datatypes/trajectory.py:56-109), state_dict's
// `aug` (environment/env_utils/state_processors.py:44-53) and unpacker(mirrored=True) (agents/agent_utils/state_unpack.py:88-105).
//
// `__host__ __device__` like tetris_traj.h: tetris_hip.hip wraps these in gfx950 kernels (k_traj_observe, k_select_count,
// k_select_scan, k_select_scatter, k_traj_batch: tetris_dev_traj.h), tests/cpu_harness/harness_lib_agent.h in plain host loops.
#pragma once
#include "tetris_kernels.h"

namespace te {

constexpr int OBS_WORDS = 12;                    // words of one slot's record: ten columns, two words of scalars
constexpr int BATCH_BLOCK = 64;                  // samples per workgroup of k_traj_batch: one lane each
constexpr int SELECT_THREADS = 256;              // threads per workgroup of the selection kernels, 16 mask bytes each
constexpr int SELECT_ELEMS = SELECT_THREADS * 16;   // mask bytes per workgroup
constexpr uint32_t BATCH_MIRROR = 0x80000000u;   // bit 31 of an index: the mirrored sample

struct alignas(16) Quad { uint32_t x, y, z, w; };   // one 16-byte load or store

// ---- the record --------------------------------------------------------------------------------------------------------------
// words 10 and 11 of a record from the scalars of the observation, and back
TE_HD uint32_t obs_record_word10(const ObsScalars& s) { return s.x | (s.y << 8) | (s.inc << 16) | (s.time << 24); }
TE_HD uint32_t obs_record_word11(const ObsScalars& s) { return s.combo | (s.next << 8) | (s.kind << 16); }
TE_HD ObsScalars obs_record_scalars(uint32_t w10, uint32_t w11) {
    ObsScalars s;
    s.x = w10 & 255u; s.y = (w10 >> 8) & 255u; s.inc = (w10 >> 16) & 255u; s.time = w10 >> 24;
    s.combo = w11 & 255u; s.next = (w11 >> 8) & 255u; s.kind = (w11 >> 16) & 255u;
    return s;
}

struct TrajObserveArgs {
    Geo geo;
    int n, n_players;
    const uint8_t* player;          // [N] or NULL (player 0; clamped)
    uint32_t* obs;                  // row `row` of the window: [N][S][12]
};

// slot sl of game i: the board of player[i] (slot 0) or of the opponent (slot 1), as three 16-byte stores
TE_HD void traj_observe_slot(const TrajObserveArgs& oa, int i, int sl) {
    const int me = safe_player(oa.player, i, oa.n_players);
    const Ref br = board_ref(oa.geo, sl == 0 ? me : oa.n_players - 1 - me, (size_t)i);
    const ObsScalars s = obs_scalars(word_at(br, W_PIECE), word_at(br, W_MISC), word_at(br, W_DROPCOMBO));
    Quad* rec = reinterpret_cast<Quad*>(oa.obs + ((size_t)i * oa.n_players + sl) * OBS_WORDS);
    const Quad a = {word_at(br, W_COL0 + 0), word_at(br, W_COL0 + 1), word_at(br, W_COL0 + 2), word_at(br, W_COL0 + 3)};
    const Quad b = {word_at(br, W_COL0 + 4), word_at(br, W_COL0 + 5), word_at(br, W_COL0 + 6), word_at(br, W_COL0 + 7)};
    const Quad c = {word_at(br, W_COL0 + 8), word_at(br, W_COL0 + 9), obs_record_word10(s), obs_record_word11(s)};
    rec[0] = a; rec[1] = b; rec[2] = c;
}

// ---- the selection -----------------------------------------------------------------------------------------------------------
struct TrajSelectArgs {
    const uint8_t* mask;            // [total]
    uint32_t total;                 // rows * N
    int augment;
    int32_t* index;                 // [cap]
    long long cap;
    int32_t* count;                 // [1]
    int32_t* blocks;                // scratch [nblocks + 1]: counts per workgroup, then their exclusive scan and the total
    int nblocks;
};

TE_HD uint32_t select_word_bits(uint32_t w) {
    return ((w & 0xFFu) ? 1u : 0u) | ((w & 0xFF00u) ? 2u : 0u) | ((w & 0xFF0000u) ? 4u : 0u) | ((w & 0xFF000000u) ? 8u : 0u);
}
// bit k set: mask[base + k] is non-zero (k = 0..15; bytes at and past `total` count as zero).  One 16-byte load where the 16
// bytes lie inside the mask and the mask is 16-byte aligned (base is a multiple of 16), else byte loads.
TE_HD uint32_t select_bits(const TrajSelectArgs& sa, uint32_t base) {
    if (base >= sa.total) return 0u;
    if (sa.total - base >= 16u && (((uintptr_t)sa.mask) & 15u) == 0) {
        const Quad q = *reinterpret_cast<const Quad*>(sa.mask + base);
        return select_word_bits(q.x) | (select_word_bits(q.y) << 4) | (select_word_bits(q.z) << 8) | (select_word_bits(q.w) << 12);
    }
    uint32_t bits = 0u;
    for (uint32_t k = 0; k < 16u; k++)
        if (base + k < sa.total && sa.mask[base + k] != 0) bits |= 1u << k;
    return bits;
}
// the entries of `bits` go to index[pos ...] and, with augment, again with bit 31 set to index[k + pos ...]; k = entries in all
TE_HD void select_emit(const TrajSelectArgs& sa, uint32_t base, uint32_t bits, long long pos, long long k) {
    while (bits) {
        const uint32_t e = base + (uint32_t)ctz32(bits);
        bits &= bits - 1u;
        if (pos < sa.cap) sa.index[pos] = (int32_t)e;
        if (sa.augment && k + pos < sa.cap) sa.index[k + pos] = (int32_t)(e | BATCH_MIRROR);
        pos++;
    }
}

// ---- the minibatch -----------------------------------------------------------------------------------------------------------
struct TrajBatchArgs {
    int m, n_slots, H;
    uint32_t total;                 // T * N entries of the window
    const int32_t* index;           // [M]
    const uint32_t* obs;            // [T][N][S][12]
    const uint8_t* action;          // [T][N][4]
    const float* prob;              // [T][N]
    const float* reward;            // [T][N]
    const uint8_t* done;            // [T][N]
    const float* adv;               // [T][N] or NULL
    const float* target;            // [T][N] or NULL
    uint8_t* visual;                // [S][M][H][10]   (every output: or NULL)
    uint8_t* vector;                // [S][M][12]
    uint8_t* piece;                 // [S][M]
    uint8_t* action_out;            // [M][3]
    float* prob_out;                // [M]
    float* adv_out;
    float* target_out;
    float* reward_out;
    uint8_t* done_out;              // [M]
    uint8_t* valid;                 // [M]
    // tetris_replay_gather_dev (tetris_replay.h): steps > 0 makes sample j the ring position index[j / steps] + j % steps, valid
    // for an index in [0, limit), mirrored by bit 0 of flags[position]; 0: the window's own index list, as above
    int steps;
    uint32_t limit;                 // max_size
    const uint8_t* flags;           // [C]
    // tetris_replay_gather_steps_dev: a non-zero step_mask (popcount = steps) makes it index[j / steps] + the (j % steps)-th set
    // bit of the mask instead; 0: the first `steps` rows, as above
    uint64_t step_mask;
};

struct BatchEntry { uint32_t at; bool valid, mirror; };
// an element v of a window's index list: entry v & 0x7FFFFFFF of `total`, mirrored with bit 31; outside [0, total): no sample
TE_HD BatchEntry batch_index_entry(uint32_t v, uint32_t total) {
    BatchEntry en;
    en.at = v & ~BATCH_MIRROR;
    en.mirror = (v & BATCH_MIRROR) != 0;
    en.valid = en.at < total;               // (-1: 0x7FFFFFFF, never below T * N < 2^31)
    if (!en.valid) { en.at = 0; en.mirror = false; }
    return en;
}
// the position of the i-th set bit of a step mask (i < popcount(mask)), ascending
TE_HD uint32_t batch_step_row(uint64_t mask, uint32_t i) {
    for (uint32_t n = 0; n < i; n++) mask &= mask - 1u;
    const uint32_t lo = (uint32_t)mask;
    return lo ? (uint32_t)ctz32(lo) : 32u + (uint32_t)ctz32((uint32_t)(mask >> 32));
}
TE_HD BatchEntry batch_entry(const TrajBatchArgs& ba, int j) {
    BatchEntry en;
    if (ba.steps > 0) {
        const uint32_t base = (uint32_t)ba.index[j / ba.steps];
        const uint32_t i = (uint32_t)(j % ba.steps);
        en.valid = base < ba.limit;         // (limit + k_step = C = total: base + a row <= k_step stays inside the ring)
        en.at = en.valid ? base + (ba.step_mask ? batch_step_row(ba.step_mask, i) : i) : 0u;
        en.mirror = en.valid && (ba.flags[en.at] & 1u) != 0;
        return en;
    }
    return batch_index_entry((uint32_t)ba.index[j], ba.total);
}
// augment_data's piece_swap = (1, 0, 3, 2, 4, 5, 6) (trajectory.py:89); index 7 (no piece) stays
TE_HD uint32_t batch_piece_swap(uint32_t k) { return k < 4u ? (k ^ 1u) : k; }

// the 12 vector bytes (as words) and the piece byte of a record's scalar words; all zero for an entry that is not valid
TE_HD void batch_scalars(const BatchEntry& en, uint32_t w10, uint32_t w11, uint32_t& v0, uint32_t& v1, uint32_t& v2, uint32_t& piece) {
    if (!en.valid) { v0 = v1 = v2 = piece = 0u; return; }
    const ObsScalars s = obs_record_scalars(w10, w11);
    obs_vector_words(s, en.mirror, v0, v1, v2);
    piece = en.mirror ? batch_piece_swap(s.kind) : s.kind;
}
TE_HD void batch_store_vector(const TrajBatchArgs& ba, int sl, int j, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t piece) {
    if (ba.vector) {
        uint8_t* v = ba.vector + ((size_t)sl * ba.m + j) * 12;
        if ((((uintptr_t)v) & 3u) == 0) {
            uint32_t* vw = reinterpret_cast<uint32_t*>(v);
            vw[0] = v0; vw[1] = v1; vw[2] = v2;
        } else {
            for (int k = 0; k < 4; k++) { v[k] = (uint8_t)(v0 >> (8 * k)); v[4 + k] = (uint8_t)(v1 >> (8 * k)); v[8 + k] = (uint8_t)(v2 >> (8 * k)); }
        }
    }
    if (ba.piece) ba.piece[(size_t)sl * ba.m + j] = (uint8_t)piece;
}
// the row entry of sample j: action (r, 9 - t and the swapped piece when mirrored), the floats bit for bit, done, valid
TE_HD void batch_store_entry(const TrajBatchArgs& ba, int j, const BatchEntry& en) {
    const bool ok = en.valid;
    const size_t at = en.at;
    if (ba.action_out) {
        const uint8_t* a = ba.action + at * 4;
        uint32_t r = ok ? a[0] : 0u, t = ok ? a[1] : 0u, p = ok ? a[2] : 0u;
        if (en.mirror) { t = (9u - t) & 0xFFu; p = batch_piece_swap(p); }
        uint8_t* o = ba.action_out + (size_t)j * 3;
        o[0] = (uint8_t)r; o[1] = (uint8_t)t; o[2] = (uint8_t)p;
    }
    const uint32_t* prob = reinterpret_cast<const uint32_t*>(ba.prob);
    const uint32_t* reward = reinterpret_cast<const uint32_t*>(ba.reward);
    const uint32_t* adv = reinterpret_cast<const uint32_t*>(ba.adv);
    const uint32_t* target = reinterpret_cast<const uint32_t*>(ba.target);
    if (ba.prob_out) reinterpret_cast<uint32_t*>(ba.prob_out)[j] = ok ? prob[at] : 0u;
    if (ba.adv_out) reinterpret_cast<uint32_t*>(ba.adv_out)[j] = (ok && adv) ? adv[at] : 0u;
    if (ba.target_out) reinterpret_cast<uint32_t*>(ba.target_out)[j] = (ok && target) ? target[at] : 0u;
    if (ba.reward_out) reinterpret_cast<uint32_t*>(ba.reward_out)[j] = ok ? reward[at] : 0u;
    if (ba.done_out) ba.done_out[j] = ok ? ba.done[at] : (uint8_t)0;
    if (ba.valid) ba.valid[j] = ok ? (uint8_t)1 : (uint8_t)0;
}

// Serial form of sample j, slot sl (CPU harness; the kernel builds the planes in an LDS tile instead)
TE_HD void batch_sample_slot(const TrajBatchArgs& ba, int j, int sl) {
    const BatchEntry en = batch_entry(ba, j);
    const uint32_t* rec = ba.obs + ((size_t)en.at * ba.n_slots + sl) * OBS_WORDS;
    if (ba.visual) {
        uint8_t* cells = ba.visual + ((size_t)sl * ba.m + j) * (size_t)(ba.H * NCOL);
        for (int y = 0; y < ba.H; y++)
            for (int c = 0; c < NCOL; c++)
                cells[y * NCOL + c] = en.valid ? (uint8_t)((rec[en.mirror ? NCOL - 1 - c : c] >> y) & 1u) : (uint8_t)0;
    }
    uint32_t v0, v1, v2, piece;
    batch_scalars(en, rec[10], rec[11], v0, v1, v2, piece);
    batch_store_vector(ba, sl, j, v0, v1, v2, piece);
    if (sl == 0) batch_store_entry(ba, j, en);
}

}  // namespace te
