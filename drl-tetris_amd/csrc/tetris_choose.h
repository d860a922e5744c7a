// Kernel bodies of choosing a planning agent's action list from phi (include/tetris_hip.h: tetris_select_lists_dev, which
// tetris_step_lists_eval_dev begins with): the part of sherlock_agent.get_action between the network and perform_action
// (agents/sherlock_agent/sherlock_agent.py:91-156, sherlock_utils.py:34-63) — the plane of the held piece cut out of phi_eval
// [N][H][10][K], one score per list from the simulated columns, the normalisation, the choice and the trajectory's side outputs.
// The [N][H][10][L] deltas tensor is never formed: a list's score is a walk over the set bits of after ^ before.
//
// `__host__ __device__` like tetris_plan.h and tetris_act.h: tetris_hip.hip wraps these in a gfx950 kernel (k_plan_choose, tetris_dev_agent_plan.h),
// tests/cpu_harness/harness_lib_agent.h in a plain host loop.
//
// The bodies work on one game's phi plane as a strided float32 array — w[cell * sw], cell = 10 y + x — and on its scores
// x[k * sx]: on the GPU both are columns of a workgroup's LDS image (the lane's game fixed), on the host small arrays.  Every sum
// is a float32 sum in the order the header states and the builds use -ffp-contract=off, so host and device give the same bits;
// the one library call is logf in the entropy, which is compared with a tolerance.
#pragma once
#include <math.h>

#include "tetris_act.h"
#include "tetris_plan.h"

namespace te {

constexpr int CHOOSE_MAX_LISTS = 256;
constexpr int CHOOSE_THREADS = 256;              // threads of a workgroup of k_plan_choose
constexpr int CHOOSE_COUNT_PLANES = 9;           // bits of a per-cell count over at most 256 lists

struct PlanChooseArgs {
    KArgs a;                    // state, H, N (a.n = N), players, game offset
    const uint8_t* player;      // [N] acting player (NULL: player 0; clamped)
    const int32_t* count;       // [N] lists per game (clamped into [0, L])
    const uint32_t* cols;       // [L][P][10][N] (as plan_sim_lane wrote them)
    int max_lists;              // L
    float small_fill;
    const void* phi;            // [N][H][10][K] float32, or binary16 with phi_f16
    const void* state_eval;     // [N][V] float32, or binary16 with value_f16 (NULL: no value output)
    int K, V;
    int phi_f16, value_f16, out_f16;
    int mode;                   // ACT_ARGMAX or ACT_PI
    uint32_t seed, draw_lo, draw_hi;
    int32_t* choice;            // [N]
    uint8_t* piece;             // [N] (may be NULL, as everything below)
    float* prob;                // [N]
    float* probs;               // [N][L]
    float* value;               // [2][N]
    float* entropy;             // [N] (PI)
    void* delta;                // [N][H][10] float32 or binary16 (out_f16)
    void* sums;                 // [N][H][10]
};

// C_c: the sum of column c of the plane, rows in turn
TE_HD float choose_column_sum(const float* w, int sw, int H, int c) {
    float s = 0.0f;
    for (int y = 0; y < H; y++) s += w[(y * NCOL + c) * sw];
    return s;
}
// W = ((C_0 + C_1) + C_2) + ... + C_9
TE_HD float choose_plane_sum(const float* colsum, int sc) {
    float s = colsum[0];
    for (int c = 1; c < NCOL; c++) s += colsum[c * sc];
    return s;
}
// the score of a normal list: columns in turn, within a column the rows whose cell changed in turn; + w arrived, - w left
TE_HD float choose_normal_score(const uint32_t* after, const uint32_t* before, const float* w, int sw) {
    float s = 0.0f;
    TE_UNROLL
    for (int c = 0; c < NCOL; c++) {
        uint32_t x = after[c] ^ before[c];
        while (x) {
            const int y = ctz32(x);
            x &= x - 1u;
            const float v = w[(y * NCOL + c) * sw];
            s = ((after[c] >> y) & 1u) ? s + v : s - v;
        }
    }
    return s;
}
TE_HD float choose_score(int kind, const uint32_t* after, const uint32_t* before, const float* w, int sw, float small_fill, float plane_sum) {
    return kind == PLAN_LIST_NORMAL ? choose_normal_score(after, before, w, sw) : kind == PLAN_LIST_SMALL ? small_fill * plane_sum : 0.0f;
}

// From the scores x[k * sx], k < count, to the choice; x is left holding q_k.  prob = q_choice; entropy: PI with ca.entropy.
TE_HD int choose_decide(const PlanChooseArgs& ca, int i, int count, float* x, int sx, float& prob, float& entropy) {
    prob = 0.0f;
    entropy = 0.0f;
    if (count <= 0) return 0;
    float total = 0.0f;
    for (int k = 0; k < count; k++) total += x[k * sx];
    bool nan = false;
    int best = 0;
    float bq = 0.0f;
    for (int k = 0; k < count; k++) {
        const float q = x[k * sx] / total;
        x[k * sx] = q;
        nan |= q != q;
        if (k == 0 || q > bq) { bq = q; best = k; }
    }
    int choice = 0;
    if (!nan) {
        choice = best;
        if (ca.mode == ACT_PI) {
            uint32_t w[4];
            philox4x32_10(ca.seed, ca.a.game_offset + (uint32_t)i, ca.draw_lo, ca.draw_hi, w);
            const int pick = act_draw(x, sx, act_unit(w[0]), count, true);       // the weights are q > 0 ? q : 0
            if (pick >= 0) choice = pick;
            if (ca.entropy) {
                float s = 0.0f;
                for (int k = 0; k < count; k++) {
                    const float q = x[k * sx];
                    s += q * logf(q + 1e-8f);
                }
                entropy = -s;
            }
        }
    }
    prob = x[choice * sx];
    return choice;
}

// the per-game outputs that are one element each
TE_HD void choose_write(const PlanChooseArgs& ca, int i, int piece, int choice, float prob, float entropy) {
    const size_t n = (size_t)ca.a.n;
    ca.choice[i] = choice;
    if (ca.piece) ca.piece[i] = (uint8_t)piece;
    if (ca.prob) ca.prob[i] = prob;
    if (ca.entropy) ca.entropy[i] = entropy;
    if (ca.value) {                                        // as act_write
        const size_t row = (size_t)i * ca.V;
        float s = 0.0f;
        for (int k = 0; k < ca.V; k++) s += act_element(ca.state_eval, row + k, ca.value_f16);
        ca.value[i] = act_element(ca.state_eval, row + (ca.V > 1 ? imin(piece, ca.V - 1) : 0), ca.value_f16);
        ca.value[n + i] = s / (float)ca.V;
    }
}

// an element of d_delta / d_sums from its float32 value
TE_HD void choose_store(void* out, size_t at, float v, int f16) {
    if (f16) ((uint16_t*)out)[at] = plan_encode<uint16_t>(v);
    else ((float*)out)[at] = v;
}

// Serial form of game i (CPU harness; k_plan_choose spreads the same steps over a workgroup).
TE_HD void plan_choose_game(const PlanChooseArgs& ca, int i) {
    const int H = ca.a.H, L = ca.max_lists, P = ca.a.n_players, HW = H * NCOL;
    const size_t n = (size_t)ca.a.n;
    const Geo geo = geo_of(ca.a);
    const int p = safe_player(ca.player, i, P);
    const int piece = act_piece_of(geo, (size_t)i, p, ca.K);
    const int count = plan_clamp_count(ca.count[i], L);
    const uint32_t mask = plan_row_mask(H);
    const Ref br = board_ref(geo, p, (size_t)i);
    uint32_t before[NCOL], after[NCOL], chosen[NCOL];
    for (int c = 0; c < NCOL; c++) { before[c] = word_at(br, W_COL0 + c) & mask; chosen[c] = 0; }
    float w[MAX_H * NCOL], colsum[NCOL], x[CHOOSE_MAX_LISTS];
    uint8_t kinds[CHOOSE_MAX_LISTS];
    int acc[MAX_H * NCOL];
    for (int t = 0; t < HW; t++) {
        w[t] = act_element(ca.phi, ((size_t)i * HW + t) * ca.K + piece, ca.phi_f16);
        acc[t] = 0;
    }
    for (int c = 0; c < NCOL; c++) colsum[c] = choose_column_sum(w, 1, H, c);
    const float plane_sum = choose_plane_sum(colsum, 1);
    int n_small = 0;
    for (int k = 0; k < count; k++) {
        for (int c = 0; c < NCOL; c++) after[c] = ca.cols[(((size_t)k * P + p) * NCOL + c) * n + i] & mask;
        const int kind = plan_list_kind(k, count, plan_list_sum(after, before));
        kinds[k] = (uint8_t)kind;
        n_small += kind == PLAN_LIST_SMALL;
        x[k] = choose_score(kind, after, before, w, 1, ca.small_fill, plane_sum);
        if (kind == PLAN_LIST_NORMAL)
            for (int t = 0; t < HW; t++) acc[t] += plan_cell_delta(after[t % NCOL], before[t % NCOL], t / NCOL);
    }
    float prob, entropy;
    const int choice = choose_decide(ca, i, count, x, 1, prob, entropy);
    choose_write(ca, i, piece, choice, prob, entropy);
    if (ca.probs)
        for (int k = 0; k < L; k++) ca.probs[(size_t)i * L + k] = k < count ? x[k] : 0.0f;
    if (ca.sums)
        for (int t = 0; t < HW; t++) choose_store(ca.sums, (size_t)i * HW + t, plan_sums_value(acc[t], n_small, ca.small_fill), ca.out_f16);
    if (ca.delta) {
        const int kind = count > 0 ? kinds[choice] : PLAN_LIST_PAST;
        if (kind == PLAN_LIST_NORMAL)
            for (int c = 0; c < NCOL; c++) chosen[c] = ca.cols[(((size_t)choice * P + p) * NCOL + c) * n + i] & mask;
        for (int t = 0; t < HW; t++) {
            const int d = kind == PLAN_LIST_NORMAL ? plan_cell_delta(chosen[t % NCOL], before[t % NCOL], t / NCOL) : 0;
            choose_store(ca.delta, (size_t)i * HW + t, plan_delta_value(kind, d, ca.small_fill), ca.out_f16);
        }
    }
}

// ---------------------------------------------------------------- the workgroup's LDS image (k_plan_choose)
// G games per workgroup: the phi planes [H * 10][G + 1] (later the staging of d_sums and d_delta), the scores [L][G + 1], the
// column sums [10][G + 1], six words per game (player, piece, count, choice, small lists, normal lists), the list kinds [L][G]
// bytes.  Rows of G + 1 words: a lane-per-game access and a walk along one game's cells are both free of bank conflicts.
constexpr int CHOOSE_META = 6;
TE_HD size_t choose_lds_bytes(int G, int H, int L) {
    return ((size_t)(H * NCOL + L + NCOL) * (G + 1) + (size_t)CHOOSE_META * G) * 4 + (size_t)L * G;
}
// 32 games where that fits 64 KB (20 rows and 64 lists: 37 KB, four workgroups per CU), else 16 (31 rows and 256 lists: 43 KB)
TE_HD int choose_games_per_block(int H, int L) { return choose_lds_bytes(32, H, L) <= 65536 ? 32 : 16; }

}  // namespace te
