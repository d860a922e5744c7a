// Kernel bodies of acting on a network's (r, t, piece) evaluation (include/tetris_hip.h: tetris_select_eval_dev, which
// tetris_step_eval_dev and tetris_step_eval_observe_dev begin with): the part of sventon_agent.get_action between the network and
// perform_action (agents/sventon_agent/sventon_agent.py:56-98, sventon_utils.py:15-76) — the [4][10] map of the piece a game
// holds cut out of action_eval [N][4][10][K], a choice drawn from it (argmax, the map as a distribution, a rank table, epsilon
// greedy) and the trajectory's side outputs.
//
// `__host__ __device__` like tetris_plan.h and tetris_policy.h: tetris_hip.hip wraps these in a gfx950 kernel (k_act_select,
// tetris_dev_act.h), tests/cpu_harness/harness_lib_agent.h in a plain host loop.
//
// The bodies work on one game's 40 candidate values as a strided float32 array — x[c * sx] — and, for the two sampling modes, on
// 40 weights m[c * sm] of the same shape: on the GPU both are columns of a workgroup's LDS image (stride ACT_LDS_STRIDE, the
// lane's game fixed), on the host two small arrays.  No arrays indexed at run time live in registers, nothing needs scratch.
// Every sum is a float32 sum in index order and the builds use -ffp-contract=off, so host and device give the same bits; the
// one library call is logf in the entropy, which is compared with a tolerance.
#pragma once
#include <math.h>

#include "tetris_kernels.h"

namespace te {

constexpr int ACT_CANDIDATES = 40;               // c = 10 r + t
constexpr int ACT_BLOCK = 64;                    // games per workgroup
constexpr int ACT_LDS_STRIDE = ACT_BLOCK + 1;    // floats between two candidates of one game in LDS: the scatter of one game's
                                                 // candidates and the lane-per-game reads are both conflict-free
constexpr int ACT_ARGMAX = TETRIS_ACT_ARGMAX, ACT_PI = TETRIS_ACT_PI, ACT_RANK = TETRIS_ACT_RANK, ACT_EPSILON = TETRIS_ACT_EPSILON;

struct ActArgs {
    KArgs a;                    // state, tables, status words, H, N (a.n = N), ms, done / lines / dead outputs, game offset
    const uint8_t* player;      // [N] acting player (NULL: player 0; clamped)
    const void* action_eval;    // [N][4][10][K] float32, or binary16 with eval_f16
    const void* state_eval;     // [N][V] float32, or binary16 with value_f16 (NULL: no value output)
    int K, V;
    int eval_f16, value_f16;
    int mode;                   // ACT_*
    uint32_t seed, draw_lo, draw_hi;
    float epsilon;
    float table[ACT_CANDIDATES];   // RANK: weight of rank k + 1 (by value: it travels in the kernel arguments)
    uint8_t* rot;               // [N]
    uint8_t* trans;             // [N]
    uint8_t* piece;             // [N] (may be NULL, as everything below)
    float* eval;                // [N]
    float* value;               // [2][N]
    float* entropy;             // [N] (PI)
};

// IEEE binary16 bits -> float32, exact, in integer arithmetic (the opposite direction of plan_f32_to_f16; the host compiler of
// the CPU harness has no half type, and the kernel uses the same function)
TE_HD float act_f16_to_f32(uint16_t h) {
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = ((uint32_t)h >> 10) & 31u, m = (uint32_t)h & 0x3FFu;
    if (e == 31u) return u2f(sign | 0x7F800000u | (m << 13));                 // infinity, NaN (payload kept)
    if (e != 0u) return u2f(sign | ((e + 112u) << 23) | (m << 13));           // normal: rebias 15 -> 127
    if (m == 0u) return u2f(sign);
    const uint32_t p = 31u - (uint32_t)clz32(m);                              // subnormal: m * 2^-24 = 1.f * 2^(p - 24)
    return u2f(sign | ((p + 103u) << 23) | ((m << (23u - p)) & 0x7FFFFFu));
}

TE_HD float act_element(const void* base, size_t index, int f16) {
    return f16 ? act_f16_to_f32(((const uint16_t*)base)[index]) : ((const float*)base)[index];
}

// the piece index of game `slot`'s acting player as observe() gives it, limited to K - 1
TE_HD int act_piece_of(const Geo& geo, size_t slot, int player, int K) {
    return imin((int)(word_at(board_ref(geo, player, slot), W_PIECE) & 7u), K - 1);
}

// ARGMAX: the highest value among the candidates that are not NaN, the lowest c among equals; all NaN: 0
TE_HD int act_argmax(const float* x, int sx) {
    int bc = 0;
    float best = 0.0f;
    bool have = false;
    for (int c = 0; c < ACT_CANDIDATES; c++) {
        const float v = x[c * sx];
        if (have ? v > best : v == v) { best = v; bc = c; have = true; }
    }
    return bc;
}

// RANK: 1 + the number of candidates ahead of c: a higher value, or the same value and a lower index (1..40)
TE_HD int act_rank(const float* x, int sx, int c) {
    const float v = x[c * sx];
    int r = 1;
    for (int o = 0; o < ACT_CANDIDATES; o++) {
        const float w = x[o * sx];
        r += (w > v || (w == v && o < c)) ? 1 : 0;
    }
    return r;
}

TE_HD float act_pi_weight(float v) { return v > 0.0f ? v : 0.0f; }

TE_HD float act_unit(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }       // (w >> 8) * 2^-24, exact

// The inverse-CDF draw over the weights m: the first c whose running sum exceeds u * total; none: the last c with a positive
// weight; -1: the total is not a positive finite number (the caller takes ARGMAX's choice).  `count` weights (the 40 candidates;
// tetris_choose.h: a game's lists); with `clamp` the array holds values v and the weights are act_pi_weight(v).
TE_HD int act_draw(const float* m, int sm, float u, int count = ACT_CANDIDATES, bool clamp = false) {
    float total = 0.0f;
    for (int c = 0; c < count; c++) total += clamp ? act_pi_weight(m[c * sm]) : m[c * sm];
    if (!(total > 0.0f && total < INFINITY)) return -1;
    const float target = u * total;
    float run = 0.0f;
    int last = 0;
    for (int c = 0; c < count; c++) {
        const float w = clamp ? act_pi_weight(m[c * sm]) : m[c * sm];
        run += w;
        if (run > target) return c;
        if (w > 0.0f) last = c;
    }
    return last;
}

// PI's entropy: -sum q log(q + 1e-8), q = x + 1e-6 (sventon_utils.action_distribution, tools/utils.entropy)
TE_HD float act_entropy(const float* x, int sx) {
    float s = 0.0f;
    for (int c = 0; c < ACT_CANDIDATES; c++) {
        const float q = x[c * sx] + 1e-6f;
        s += q * logf(q + 1e-8f);
    }
    return -s;
}

// the weights of game i's 40 candidates (PI; RANK in the serial form)
TE_HD void act_weights(const ActArgs& aa, const float* table, const float* x, int sx, float* m, int sm) {
    for (int c = 0; c < ACT_CANDIDATES; c++)
        m[c * sm] = aa.mode == ACT_RANK ? table[act_rank(x, sx, c) - 1] : act_pi_weight(x[c * sx]);
}

// The choice of game i, 0..39.  `m` holds the weights already when weights_ready (RANK spread over a workgroup's lanes).
TE_HD int act_choose(const ActArgs& aa, int i, const float* table, const float* x, int sx, float* m, int sm, bool weights_ready) {
    if (aa.mode == ACT_ARGMAX) return act_argmax(x, sx);
    uint32_t w[4];
    philox4x32_10(aa.seed, aa.a.game_offset + (uint32_t)i, aa.draw_lo, aa.draw_hi, w);
    int c;
    if (aa.mode == ACT_EPSILON) {
        c = act_unit(w[1]) < aa.epsilon ? (int)(10u * (w[2] & 3u) + w[3] % 10u) : -1;
    } else {
        if (!weights_ready) act_weights(aa, table, x, sx, m, sm);
        c = act_draw(m, sm, act_unit(w[0]));
    }
    return c >= 0 ? c : act_argmax(x, sx);
}

// the outputs of game i for choice c and piece index `piece`
TE_HD void act_write(const ActArgs& aa, int i, int piece, int c, const float* x, int sx) {
    const size_t n = (size_t)aa.a.n;
    aa.rot[i] = (uint8_t)(c / 10);
    aa.trans[i] = (uint8_t)(c % 10);
    if (aa.piece) aa.piece[i] = (uint8_t)piece;
    if (aa.eval) aa.eval[i] = x[c * sx];
    if (aa.entropy) aa.entropy[i] = act_entropy(x, sx);
    if (aa.value) {
        const size_t row = (size_t)i * aa.V;
        float s = 0.0f;
        for (int k = 0; k < aa.V; k++) s += act_element(aa.state_eval, row + k, aa.value_f16);
        aa.value[i] = act_element(aa.state_eval, row + (aa.V > 1 ? imin(piece, aa.V - 1) : 0), aa.value_f16);     // value_piece
        aa.value[n + i] = s / (float)aa.V;                                                                        // value_mean
    }
}

// Serial form of the selection of game i (CPU harness; the kernels spread the same steps over a workgroup) -> c
TE_HD int act_select_game(const ActArgs& aa, int i) {
    const int piece = act_piece_of(geo_of(aa.a), (size_t)i, safe_player(aa.player, i, aa.a.n_players), aa.K);
    float x[ACT_CANDIDATES], m[ACT_CANDIDATES];
    for (int c = 0; c < ACT_CANDIDATES; c++)
        x[c] = act_element(aa.action_eval, ((size_t)i * ACT_CANDIDATES + c) * aa.K + piece, aa.eval_f16);
    const int c = act_choose(aa, i, aa.table, x, 1, m, 1, false);
    act_write(aa, i, piece, c, x, 1);
    return c;
}

}  // namespace te
