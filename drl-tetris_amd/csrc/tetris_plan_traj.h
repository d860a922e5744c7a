// Kernel bodies of the planning agent's trajectory windows (include/tetris_hip.h: tetris_traj_record_plan_dev,
// tetris_traj_plan_batch_dev): what sherlock_agent.get_action stores per step (agents/sherlock_agent/sherlock_agent.py:137-146)
// — a_idx, piece, pi(a), v_piece, v_mean, delta(s, a), delta_sum(s) — kept as one packed record per entry, and the expansion of a
// permuted slice of records into the delta / delta_sum planes sherlock_agent_ppo_trainer.do_training consumes
// (sherlock_agent_ppo_trainer.py:36-63).
//
// `__host__ __device__` like tetris_traj.h and tetris_choose.h: tetris_hip.hip wraps these in gfx950 kernels (k_traj_record_plan,
// k_traj_plan_batch: tetris_dev_traj.h), tests/cpu_harness/harness_lib_agent.h in plain host loops.  The values of the
// planes are plan_delta_value / plan_sums_value (tetris_plan.h) on integers read out of the record, so the expansion gives the
// bits tetris_plan_deltas_dev and tetris_select_lists_dev write for the same small_fill.
#pragma once
#include "tetris_batch.h"
#include "tetris_choose.h"
#include "tetris_traj.h"

namespace te {

// ---- the record ----------------------------------------------------------------------------------------------------------------
constexpr int PLAN_REC_WORDS = 112;              // words of one entry's record (= TETRIS_PLAN_REC_WORDS)
constexpr int PLAN_REC_QUADS = PLAN_REC_WORDS / 4;
constexpr int PLAN_REC_BEFORE = 0;               // words 0..9: the acting player's columns before the step
constexpr int PLAN_REC_AFTER = 10;               // words 10..19: the columns of the chosen list (zero unless it is NORMAL)
constexpr int PLAN_REC_KIND = 20;                // the chosen list's kind (PLAN_LIST_PAST = 2: no list)
constexpr int PLAN_REC_COUNTS = 21;              // n_small | n_normal << 16
constexpr int PLAN_REC_PLANES = 22;              // word 22 + 9 c + j: bit-plane j of the per-cell counts of column c
static_assert(PLAN_REC_PLANES + NCOL * CHOOSE_COUNT_PLANES == PLAN_REC_WORDS, "ten columns of nine planes end the record");
static_assert(PLAN_REC_WORDS % 4 == 0 && PLAN_REC_WORDS == TETRIS_PLAN_REC_WORDS, "a record is whole 16-byte units");

constexpr int PLAN_RECORD_GAMES = 32;            // games per workgroup of k_traj_record_plan
constexpr int PLAN_RECORD_THREADS = 256;
constexpr int PLAN_RECORD_MAX_LISTS = CHOOSE_MAX_LISTS;
constexpr int PLAN_BATCH_SAMPLES = 32;           // samples per workgroup of k_traj_plan_batch: a multiple of 8
constexpr int PLAN_BATCH_THREADS = 256;
static_assert(PLAN_BATCH_SAMPLES % 8 == 0, "a workgroup's run of either output starts on 16 bytes for every H and both types");

struct PlanRecordArgs {
    int n, n_players, H, max_lists;
    const uint8_t* player;          // [N] or NULL (player 0; clamped): e->d_player
    const int32_t* count;           // [N] (with rec)
    const uint32_t* cols;           // [L][P][10][N] (with rec)
    const int32_t* choice;          // [N]
    const uint8_t* piece;           // [N]
    const float* prob_in;           // [N]
    const float* value;             // [2][N] or NULL (zeros)
    const uint8_t* done;            // [N] the step's outputs
    const uint8_t* dead;            // [P][N]
    const uint32_t* obs;            // row `row` of the observation records: [N][S][12] (with rec)
    uint32_t* rec;                  // row `row` of the plan records: [N][112], or NULL (the row arrays only)
    uint8_t* action;                // row `row` of the window: [N][4]
    float* prob;                    // [N]
    float* value0;                  // [N] of value[0]
    float* value1;                  // [N] of value[1]
    float* reward;                  // [N]
    uint8_t* done_out;              // [N]
};

// the chosen list of game i: e->d_choice[i] clamped into [0, max(count, 1) - 1]
TE_HD int plan_record_choice(int choice, int count) { return imax(0, imin(choice, imax(count, 1) - 1)); }

// row `row` of game i: what tetris_traj_record_dev writes, with the list's index in place of (r, t)
TE_HD void plan_record_row(const PlanRecordArgs& ra, int i, int p, int choice) {
    uint8_t* a = ra.action + (size_t)i * 4;
    a[0] = (uint8_t)(choice & 255); a[1] = 0; a[2] = ra.piece[i]; a[3] = (uint8_t)p;
    ra.prob[i] = ra.prob_in[i];
    ra.value0[i] = ra.value ? ra.value[i] : 0.0f;
    ra.value1[i] = ra.value ? ra.value[(size_t)ra.n + i] : 0.0f;
    const uint8_t d = ra.done[i];
    ra.done_out[i] = d;
    ra.reward[i] = traj_reward(ra.dead, i, ra.n, ra.n_players, p, d != 0);
}

// one more column word into the nine bit-sliced counters of a column (a ripple-carry add of 1 per set bit)
TE_HD void plan_count_add(uint32_t* plane, uint32_t word) {
    uint32_t carry = word;
    TE_UNROLL
    for (int j = 0; j < CHOOSE_COUNT_PLANES; j++) {
        const uint32_t both = plane[j] & carry;
        plane[j] ^= carry;
        carry = both;
    }
}
// the count of row y out of the nine planes at w[0..8]
TE_HD uint32_t plan_count_read(const uint32_t* w, int y) {
    uint32_t cnt = 0;
    TE_UNROLL
    for (int j = 0; j < CHOOSE_COUNT_PLANES; j++) cnt |= ((w[j] >> y) & 1u) << j;
    return cnt;
}

// Serial form of game i (CPU harness; k_traj_record_plan spreads the same steps over a workgroup).
TE_HD void plan_record_game(const PlanRecordArgs& ra, int i) {
    const int P = ra.n_players, L = ra.max_lists;
    const size_t n = (size_t)ra.n;
    const int p = safe_player(ra.player, i, P);
    if (!ra.rec) {                                         // no plan records: no count to clamp the choice with
        plan_record_row(ra, i, p, ra.choice[i]);
        return;
    }
    const int count = plan_clamp_count(ra.count[i], L);
    const int choice = plan_record_choice(ra.choice[i], count);
    const uint32_t mask = plan_row_mask(ra.H);
    uint32_t* rec = ra.rec + (size_t)i * PLAN_REC_WORDS;
    uint32_t before[NCOL], after[NCOL];
    for (int c = 0; c < NCOL; c++) before[c] = ra.obs[(size_t)i * P * OBS_WORDS + c] & mask;
    for (int w = 0; w < PLAN_REC_WORDS; w++) rec[w] = 0u;
    int n_small = 0, n_normal = 0, chosen_kind = PLAN_LIST_PAST;
    for (int k = 0; k < count; k++) {
        for (int c = 0; c < NCOL; c++) after[c] = ra.cols[(((size_t)k * P + p) * NCOL + c) * n + i] & mask;
        const int kind = plan_list_kind(k, count, plan_list_sum(after, before));
        n_small += kind == PLAN_LIST_SMALL;
        n_normal += kind == PLAN_LIST_NORMAL;
        if (kind == PLAN_LIST_NORMAL)
            for (int c = 0; c < NCOL; c++) plan_count_add(rec + PLAN_REC_PLANES + CHOOSE_COUNT_PLANES * c, after[c]);
        if (k == choice) {
            chosen_kind = kind;
            if (kind == PLAN_LIST_NORMAL)
                for (int c = 0; c < NCOL; c++) rec[PLAN_REC_AFTER + c] = after[c];
        }
    }
    for (int c = 0; c < NCOL; c++) rec[PLAN_REC_BEFORE + c] = before[c];
    rec[PLAN_REC_KIND] = (uint32_t)chosen_kind;
    rec[PLAN_REC_COUNTS] = (uint32_t)n_small | ((uint32_t)n_normal << 16);
    plan_record_row(ra, i, p, choice);
}

// ---- the minibatch -------------------------------------------------------------------------------------------------------------
struct PlanBatchArgs {
    int m, H;
    uint32_t total;                 // T * N entries of the window
    const int32_t* index;           // [M]
    const uint32_t* rec;            // [T][N][112]
    float small_fill;
    int f16;
    void* delta;                    // [M][H][10] float32 or binary16, or NULL
    void* sums;                     // [M][H][10], or NULL
};

// sample j: its entry (0 when it names none), whether it names one, whether it is the mirrored sample
TE_HD BatchEntry plan_batch_entry(const PlanBatchArgs& ba, int j) { return batch_index_entry((uint32_t)ba.index[j], ba.total); }

// cell (y, c) of delta and of sums from the record at r (global memory, LDS or a host array); mirror: column 9 - c of the record.
// A record of zeros — an entry that names no sample — gives +0 in both.
TE_HD float plan_rec_delta(const uint32_t* r, bool mirror, int y, int c, float small_fill) {
    const int src = mirror ? NCOL - 1 - c : c;
    return plan_delta_value((int)r[PLAN_REC_KIND], plan_cell_delta(r[PLAN_REC_AFTER + src], r[PLAN_REC_BEFORE + src], y), small_fill);
}
TE_HD float plan_rec_sums(const uint32_t* r, bool mirror, int y, int c, float small_fill) {
    const int src = mirror ? NCOL - 1 - c : c;
    const uint32_t counts = r[PLAN_REC_COUNTS];
    const int n_small = (int)(counts & 0xFFFFu), n_normal = (int)(counts >> 16);
    const int cnt = (int)plan_count_read(r + PLAN_REC_PLANES + CHOOSE_COUNT_PLANES * src, y);
    return plan_sums_value(cnt - n_normal * (int)((r[PLAN_REC_BEFORE + src] >> y) & 1u), n_small, small_fill);
}

// Serial form of sample j (CPU harness; k_traj_plan_batch builds 16 bytes of consecutive elements per thread from LDS)
TE_HD void plan_batch_sample(const PlanBatchArgs& ba, int j) {
    const BatchEntry en = plan_batch_entry(ba, j);
    uint32_t r[PLAN_REC_WORDS];
    for (int w = 0; w < PLAN_REC_WORDS; w++) r[w] = en.valid ? ba.rec[(size_t)en.at * PLAN_REC_WORDS + w] : 0u;
    const int HW = ba.H * NCOL;
    for (int t = 0; t < HW; t++) {
        const int y = t / NCOL, c = t - y * NCOL;
        const size_t at = (size_t)j * HW + t;
        if (ba.delta) choose_store(ba.delta, at, plan_rec_delta(r, en.mirror, y, c, ba.small_fill), ba.f16);
        if (ba.sums) choose_store(ba.sums, at, plan_rec_sums(r, en.mirror, y, c, ba.small_fill), ba.f16);
    }
}

}  // namespace te
