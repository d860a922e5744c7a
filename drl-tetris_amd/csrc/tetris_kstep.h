// Kernel bodies of the DQN trainer's k-step target estimator (include/tetris_hip.h: tetris_kstep_target_dev): what
// model.compute_targets (agents/sventon_agent/sventon_agent_dqn_trainer.py:49-59) computes from the reference net's outputs for the
// k-step views — value_estimator._create_estimator and _aggregate (agents/networks/value_estimator.py:51-88) with q_to_v
// (agents/networks/network_utils.py:95-98) for the value of a step.
//
// `__host__ __device__` like tetris_loss.h: tetris_hip.hip wraps these in gfx950 kernels (k_kstep_values, k_kstep_estimate:
// tetris_dev_kstep.h), the CPU harness (tests/cpu_harness) runs them through kstep_run_serial (tetris_host.h) in plain host loops.
// float32 throughout, -ffp-contract=off (no fused multiply-adds), the division correctly rounded, no library call on the device;
// every expression below is evaluated in the order it is written, so host and device give the same bits.
//
// DEFINITION.  k = k_step (1..63); S = the set bits of step_mask, all within [1, k], in ascending order s_0 < s_1 < ..; n = |S|.
// max(a, b) is written `a < b ? b : a` with a the running value: a NaN input gives an unspecified result (no access leaves the
// arrays whatever the bits).
//   ROWS.  Ring mode (d_index given): row t of sample j is element d_index[j] + t of d_reward / d_done, the ring's arrays; a
//     d_index[j] outside [0, max_size) makes the sample invalid: target 0, done_time 0, values 0.  Array mode (d_index NULL):
//     row t is element j (k + 1) + t, what the gather of k + 1 steps wrote as reward / done [M][k + 1].
//   dt = the smallest t in 0..k with a non-zero done byte in row t, k + 1 if there is none: the reference's
//     reduce_sum(1 - minimum(1, cumsum(dones))) (value_estimator.py:52-53).
//   VALUE of step s_i: from row j n + i of the net's output (the layout of the step-list gather, [M][n][...]).
//     Q mode, input Q [M][n][4][10][K]: m_p = x_0, then for c = 1..39 in ascending order m_p = max(m_p, x_c), x_c = Q[..][c][p];
//       K = 7: V = (sum of m_p over the pieces p of used_pieces, from +0, ascending p) / (float)n_used; K = 1: V = m_0.
//     V mode, input v [M][n][W], W = n_values: W = 1: V = v[..][0]; W = K = 7: the same masked mean of v[..][p].
//   DISCOUNTS.  g_t = (float)pow((double)gamma, t), t = 0..k, and l_s = (float)pow((double)lambda, s), computed on the host and
//     carried in the kernel's argument struct (the reference bakes gamma**t into its graph as a float32 constant in the same way).
//   ESTIMATES.  P_0 = +0; P_(t+1) = dt >= t ? P_t + r_t g_t : P_t; E_s = dt >= s ? P_s + V_s g_s : P_s — the order in which
//     k_step_estimate accumulates (value_estimator.py:69-76).
//   AGGREGATE.  w_s = l_s, and with TRUNCATE w_s = 0 where dt < s - 1; num = sum over S of E_s w_s, den = sum over S of w_s, both
//     from +0 in ascending s; target = num / den, and 0 where den == 0.
//   Two deviations, both under TRUNCATE only.  den == 0 — a step set whose smallest member exceeds dt + 1 — is 0 / 0 = NaN in the
//   reference.  And the reference forms (lambda f)^s, f the 0 / 1 filter, through TensorFlow's float32 pow, which may differ from
//   l_s in the last place; without TRUNCATE lambda^s is a Python float rounded once, as l_s is.
// OUTPUTS.  target [M]; optional values [M][n] (the V_s) and done_time uint8 [M] (dt).  Every element of an output that is given is
// written, nothing past M.
#pragma once
#include <math.h>

#include "tetris_act.h"

namespace te {

constexpr int KSTEP_Q = TETRIS_KSTEP_Q, KSTEP_V = TETRIS_KSTEP_V;
constexpr int KSTEP_MAX = 63;                    // the largest k_step: a step is a bit of a 64-bit mask
constexpr int KSTEP_ROWS = 32;                   // (sample, step) rows of Q per workgroup of k_kstep_values
constexpr int KSTEP_VALUE_THREADS = 256;         // its threads: at K = 7 a thread per (row, piece) for 224 of them
constexpr int KSTEP_THREADS = 256;               // k_kstep_estimate: a lane per sample
constexpr int KSTEP_PIECES = 8;                  // floats of a row's per-piece maxima in LDS

struct KstepArgs {
    int M, n, k, K, W;           // samples, steps of S, k_step, n_pieces, width of a row of v (V mode)
    int mode, f16, truncate;
    uint32_t used;               // used_pieces
    uint32_t limit;              // max_size (ring mode)
    float n_used;
    uint64_t step_mask;
    const void* x;               // Q [M][n][4][10][K] or v [M][n][W]
    const float* reward;
    const uint8_t* done;
    const int32_t* index;        // [M] (ring mode) or NULL
    float* target;               // [M]
    float* values;               // [M][n] or NULL
    uint8_t* done_time;          // [M] or NULL
    float* vals;                 // Q mode: where k_kstep_values leaves the V_s [M][n] — `values`, or the batch's scratch
    float g[KSTEP_MAX + 1], l[KSTEP_MAX + 1];
};

TE_HD int kstep_value_blocks(const KstepArgs& a) { return (int)(((long long)a.M * a.n + KSTEP_ROWS - 1) / KSTEP_ROWS); }
TE_HD bool kstep_valid(const KstepArgs& a, size_t j) { return a.index ? (uint32_t)a.index[j] < a.limit : true; }

// the masked mean of a row's `w` per-piece numbers m[p * sm]
TE_HD float kstep_mean(const KstepArgs& a, int w, const float* m, int sm) {
    if (w == 1) return m[0];
    float s = 0.0f;
    for (int p = 0; p < w; p++)
        if ((a.used >> p) & 1u) s += m[p * sm];
    return s / a.n_used;
}

// V mode: the value of row `row` of v
TE_HD float kstep_value_v(const KstepArgs& a, size_t row) {
    if (a.W == 1) return act_element(a.x, row, a.f16);
    float s = 0.0f;                                           // kstep_mean, without an array a lane would index at run time
    for (int p = 0; p < a.W; p++)
        if ((a.used >> p) & 1u) s += act_element(a.x, row * (size_t)a.W + (size_t)p, a.f16);
    return s / a.n_used;
}

// Serial form of a row of Q (CPU harness; the kernel takes the elements from the workgroup's LDS image): its value into vals
TE_HD void kstep_value_row(const KstepArgs& a, size_t row) {
    float m[7];
    for (int p = 0; p < a.K; p++) {
        const size_t at = row * ACT_CANDIDATES * (size_t)a.K + (size_t)p;
        float best = act_element(a.x, at, a.f16);
        for (int c = 1; c < ACT_CANDIDATES; c++) {
            const float x = act_element(a.x, at + (size_t)c * a.K, a.f16);
            best = best < x ? x : best;
        }
        m[p] = best;
    }
    a.vals[row] = kstep_valid(a, row / (size_t)a.n) ? kstep_mean(a, a.K, m, 1) : 0.0f;
}

// sample j from its rows of reward / done and its n values: target, done_time and, in V mode, values
TE_HD void kstep_sample(const KstepArgs& a, size_t j) {
    const bool ok = kstep_valid(a, j);
    const size_t r0 = !ok ? 0 : a.index ? (size_t)(uint32_t)a.index[j] : j * (size_t)(a.k + 1);
    int dt = a.k + 1;
    if (ok)
        for (int t = a.k; t >= 0; t--) dt = a.done[r0 + t] != 0 ? t : dt;
    float P = 0.0f, num = 0.0f, den = 0.0f;
    size_t at = j * (size_t)a.n;
    for (int s = 1; s <= a.k; s++) {
        const int t = s - 1;
        if (ok && dt >= t) P = P + a.reward[r0 + t] * a.g[t];
        if (!((a.step_mask >> s) & 1u)) continue;
        float V = 0.0f;
        if (ok) V = a.vals ? a.vals[at] : kstep_value_v(a, at);
        if (a.values && !a.vals) a.values[at] = V;
        at++;
        const float E = dt >= s ? P + V * a.g[s] : P;
        const float w = (a.truncate && dt < s - 1) ? 0.0f : a.l[s];
        num = num + E * w;
        den = den + w;
    }
    a.target[j] = (ok && den != 0.0f) ? num / den : 0.0f;
    if (a.done_time) a.done_time[j] = ok ? (uint8_t)dt : (uint8_t)0;
}

}  // namespace te
