// Kernel bodies of the trainer's loss heads (include/tetris_hip.h: tetris_ppo_loss_dev, tetris_dqn_loss_dev): the arithmetic
// between a network's outputs for a minibatch and the optimiser — the loss, its statistics and the gradient with respect to
// the outputs — of the PPO trainer (agents/networks/ppo_nets.py:141-196, create_training_ops, with N.action_entropy,
// network_utils.py:114-118) and of the DQN trainer (agents/networks/prio_qnet.py:102-117).
//
// `__host__ __device__` like tetris_act.h: tetris_hip.hip wraps these in gfx950 kernels (k_loss_head, tetris_dev_loss.h),
// the CPU harness (tests/cpu_harness) through loss_run_serial (tetris_host.h) in plain host loops.  A body works on one sample's 40 values x[j * sx] of its piece's
// plane — a column of the workgroup's LDS image on the GPU — and leaves the 40 gradient values in g[j * sg].  float32
// throughout, -ffp-contract=off, every sum in index order, logf the only library call; every expression below is evaluated in
// the order it is written, so host and device give the same bits but for logf.
//
// COMMON.  For sample m: r = min(action[m][0], 3), t = min(action[m][1], 9), k = min(action[m][2], K - 1), c = 10 r + t;
// e = 1e-6f; D = the number of samples with valid[m] != 0 (valid == NULL: M).  A sample that is not valid contributes nothing
// and its gradient rows, per-sample outputs and new_prio are zeros.  D == 0: every output is zero (the reference's means over
// nothing are NaN).  max(a, b) below is written `a < b ? b : a`, min likewise: a NaN in the first place stays.
//
// PPO.  x_j = pi[m][j][k], val = v[m][min(k, V - 1)], old = prob_old[m], A = adv[m], T = target[m].
//   p = x_c; den = max(old, e); ratio = max(p, e) / den; cl = min(max(ratio, 1 - clip), 1 + clip); pl = min(ratio A, cl A)
//   q_j = x_j + e; l_j = logf(q_j <= e ? e : q_j); H = -(sum over j of q_j l_j)
//   bonus0 = H - cf relu(floor - H); bonus = bonus0 + cr (Hmax - bonus0)
//   value_loss = c1 (sum (val - T)^2 / D); policy_loss = -c2 (sum pl / D); entropy_loss = -c3 (sum bonus / D);
//   loss = (value_loss + policy_loss) + entropy_loss
//   d loss / d v[m][min(k, V - 1)] = (((2 c1) (val - T)) / D) grad_scale
//   d loss / d pi[m][j][k] = (ce e_j [+ pp at j == c]) grad_scale with e_j = -(l_j + [q_j > e]),
//     ce = ((-(c3 / D)) (1 - cr)) (1 + (H < floor ? cf : 0)), pp = (-(c2 / D)) dpl,
//     dpl = ratio A <= cl A ? A rp : A rp [cl == ratio], rp = [p >= e] / den
//   (TensorFlow's tie rules: tf.maximum(const, x) sends the gradient to the constant at a tie — the strict > of e_j —,
//   tf.maximum(p, e) to p — the >= of rp —, and in the unclipped region both arms of the min give the same gradient.)
//   `floor` and `Hmax` come from the host (capi.ppo_entropy_constants): floor = -eps log(eps / 39) - (1 - eps) log(1 - eps) of
//   ppo_epsilon, Hmax = -sum (1/40) log(1/40 + 1e-8).  Deviation: for eps <= 0 or eps >= 1 the reference's floor is NaN; the
//   helper gives 0, which switches the floor term off for every H >= 0.  rescaled_entropy > 1 makes
//   (1 - cr) negative, as in the reference's own arithmetic.
//
// DQN.  q = Q[m][r][t][k], T = target[m], w = weight[m] (NULL: 1), d = q - T.
//   prio = |d|; optimistic != 0: prio = prio + optimistic relu(prio)
//   Dnz = the number of valid samples with w != 0; loss = sum (w (d d)) / Dnz (tf.losses.mean_squared_error's default
//   reduction), 0 when Dnz == 0;  d loss / d Q[m][r][t][k] = (((2 w) d) / Dnz) grad_scale, 0 when Dnz == 0.
//
// PLAN (the planning agent: agents/networks/delta_ppo_nets.py:150-182).  A sample is valid when valid[m] != 0 AND index[m] names an
// entry of the window (batch_index_entry: bit 31 = the mirrored image).  HW = 10 H cells t = 10 y + c; k = min(piece[m], K - 1);
//   raw_t = phi[m][y][c][k]; lowc = raw_t > 1 ? 1 : raw_t; x_t = lowc < e ? e : lowc       (tf.clip_by_value: a tie goes to raw)
//   d_t = plan_rec_delta(record, mirror, y, c, small_fill), s_t = plan_rec_sums(...)     (tetris_plan_traj.h: batch_plan's values)
//   a_t = x_t d_t; b_t = x_t s_t; u_t = s_t + e; m_t = s_t < 1 ? s_t : 1; i_t = x_t (1 - m_t)
//   num = SUM a_t; dn = SUM b_t; S = SUM u_t; I = SUM i_t                                  (SUM: the cell order below)
//   den2 = dn + e; probability = (num + e) / den2
//   den = max(old, e); ratio = max(probability, e) / den; cl, ra, ca, pl as for PPO
//   w_t = s_t / S; y_t = b_t / S + e; l_t = logf(y_t <= e ? e : y_t); Hent = -(SUM y_t l_t)
//   val = v[m][min(k, V - 1)]; dv = val - T
//   value_loss = c1 (sum dv^2 / D); policy_loss = (-c2) (sum pl / D); entropy_loss = (-c3) (sum Hent / D);
//   impossibility_loss = c4 ((sum I / D) / HW); loss = ((value_loss + policy_loss) + impossibility_loss) + entropy_loss
//   d loss / d v[m][min(k, V - 1)] = (((2 c1) dv) / D) grad_scale
//   d loss / d phi[m][y][c][k] = e <= raw_t && raw_t <= 1 ? (((pp dp_t) + (ci (1 - m_t))) + (ce (e_t w_t))) grad_scale : 0 with
//     dp_t = (d_t - probability s_t) / den2, pp = (-(c2 / D)) dpl (dpl, rp as for PPO with p = probability),
//     ci = (c4 / D) / HW, ce = -(c3 / D), e_t = -(l_t + [y_t > e])
//   (s_t, d_t are data.  Negative s_t and a non-positive dn + e or S are no special cases.)
//   SUM, the order of a sample's five sums: cell t belongs to lane t mod 64; a lane starts at +0 and adds its cells in ascending
//   t; the 64 lane sums (lanes without a cell hold +0) go through loss_tree.  The order depends neither on K, nor on the element
//   type, nor on the mirror bit.
//
// STATISTICS, float32 [16]; unused slots are zero.  Means are sums over the valid samples divided by D.
//   PPO: 0 D, 1 loss, 2 value_loss, 3 policy_loss, 4 entropy_loss, 5 mean H, 6 mean H^2, 7 mean bonus, 8 mean val, 9 mean val^2,
//        10 mean T, 11 mean T^2, 12 mean [ratio != cl] (clip_saturation), 13 mean ratio
//   DQN: 0 D, 1 Dnz, 2 loss, 3 mean q, 4 mean q^2, 5 mean T, 6 mean T^2, 7 mean prio
//   PLAN: 0 D, 1 loss, 2 value_loss, 3 policy_loss, 4 entropy_loss, 5 impossibility_loss, 6 mean Hent, 7 mean Hent^2, 8 mean val,
//        9 mean val^2, 10 mean T, 11 mean T^2, 12 mean [ratio != cl] (clip_saturation), 13 mean ratio, 14 mean probability
// The order of a statistic's sum is fixed: the samples of a block of LOSS_BLOCK = 64 (PLAN: PLAN_LOSS_BLOCK = 16) by the tree
// loss_tree (lanes past M add zeros), block b's row into slot b mod LOSS_REDUCE_LANES in ascending b, the slots by the same tree.
// No atomics.
#pragma once
#include <math.h>

#include "tetris_act.h"
#include "tetris_plan.h"
#include "tetris_plan_traj.h"

namespace te {

constexpr int LOSS_PPO = 0, LOSS_DQN = 1, LOSS_PLAN = 2;
constexpr int LOSS_BLOCK = ACT_BLOCK;            // samples per workgroup
constexpr int LOSS_SUMS = 12;                    // floats of a workgroup's partial row (PPO uses 11, DQN 6)
constexpr int LOSS_STATS = TETRIS_LOSS_STATS;
constexpr int LOSS_REDUCE_LANES = 256;
constexpr int LOSS_PPO_TERMS = 6;                // probability, ratio, pl, H, bonus, val
constexpr int PLAN_LOSS_TERMS = 6;               // probability, ratio, pl, Hent, I, val
constexpr int PLAN_LOSS_BLOCK = 16;              // PLAN: samples per workgroup, a multiple of 8 (its run of phi starts on 16 bytes)
constexpr int PLAN_LOSS_LANES = 64;              // the lanes of the cell order
constexpr int PLAN_LOSS_CELLS = (MAX_H * NCOL + PLAN_LOSS_LANES - 1) / PLAN_LOSS_LANES;      // cells of a lane at most (5)

struct LossArgs {
    int head;                    // LOSS_PPO / LOSS_DQN / LOSS_PLAN
    int M, K, V;
    int in_f16, v_f16, grad_f16;
    const void* x;               // pi / Q [M][4][10][K]
    const void* v;               // [M][V] (PPO)
    const uint8_t* action;       // [M][3]: r, t, piece
    const float* old;            // prob_old [M] (PPO)
    const float* adv;            // [M] (PPO)
    const float* target;         // [M]
    const float* weight;         // [M] or NULL (DQN)
    const uint8_t* valid;        // [M] or NULL
    float clip, c1, c2, c3, cf, cr, floor, hmax;      // PPO
    float optimistic;            // DQN
    float grad_scale;
    void* grad_x;                // [M][4][10][K] float32, or binary16 with grad_f16
    void* grad_v;                // [M][V] (PPO), as grad_x
    float* terms;                // PPO: [6][M] or NULL
    float* new_prio;             // DQN: [M]
    float* q;                    // DQN: [M] or NULL
    float* stats;                // [16]
    const uint32_t* count;       // device words D, Dnz (NULL: both are M)
    float* partial;              // [blocks][LOSS_SUMS]
    // PLAN (x: phi [M][H][10][K], grad_x likewise; action is not used)
    int H;
    uint32_t total;              // T * N entries of the window
    const uint32_t* rec;         // [T][N][112]
    const int32_t* index;        // [M]
    const uint8_t* piece;        // piece of sample m: piece[m * piece_stride]
    int piece_stride;
    float small_fill, c4;
};

TE_HD int loss_blocks(int M) { return (M + LOSS_BLOCK - 1) / LOSS_BLOCK; }

// the sum of n = 2^k floats as a fixed tree, in place: v[i] += v[i + n/2], then n/4, ... (a wave's shuffle-down reduction)
TE_HD float loss_tree(float* v, int n) {
    for (int off = n >> 1; off >= 1; off >>= 1)
        for (int i = 0; i < off; i++) v[i] += v[i + off];
    return v[0];
}

// (k, c) of sample m
TE_HD void loss_action(const LossArgs& la, size_t m, int& k, int& c) {
    const uint8_t* a = la.action + 3 * m;
    k = imin((int)a[2], la.K - 1);
    c = 10 * imin((int)a[0], 3) + imin((int)a[1], 9);
}
// (PLAN: and the index names an entry of the window)
TE_HD bool loss_valid(const LossArgs& la, size_t m) {
    const bool ok = la.valid ? la.valid[m] != 0 : true;
    return la.index ? ok && batch_index_entry((uint32_t)la.index[m], la.total).valid : ok;
}

// what sample m adds to D and Dnz
TE_HD void loss_count_sample(const LossArgs& la, size_t m, uint32_t& d, uint32_t& dnz) {
    const bool ok = loss_valid(la, m);
    d += ok ? 1u : 0u;
    dnz += (ok && (la.weight ? la.weight[m] != 0.0f : true)) ? 1u : 0u;
}

TE_HD void loss_zero_sample(float* g, int sg, float* sum, float& gv) {
    for (int j = 0; j < ACT_CANDIDATES; j++) g[j * sg] = 0.0f;
    TE_UNROLL
    for (int i = 0; i < LOSS_SUMS; i++) sum[i] = 0.0f;
    gv = 0.0f;
}

// PPO: valid sample m with piece k and candidate c, D > 0 -> g[40], the value gradient gv, the sample's terms of the sums
TE_HD void loss_ppo_sample(const LossArgs& la, size_t m, int k, int c, float D, const float* x, int sx, float* g, int sg, float* sum, float& gv) {
    const float e = 1e-6f;
    const float val = act_element(la.v, m * (size_t)la.V + (size_t)imin(k, la.V - 1), la.v_f16);
    const float old = la.old[m], A = la.adv[m], T = la.target[m];
    const float p = x[c * sx];
    const float den = old < e ? e : old;
    const float ratio = (p < e ? e : p) / den;
    const float lo = 1.0f - la.clip, hi = 1.0f + la.clip;
    const float low = ratio < lo ? lo : ratio, cl = low > hi ? hi : low;
    const float ra = ratio * A, ca = cl * A;
    const float pl = ca < ra ? ca : ra;
    float s = 0.0f;
    for (int j = 0; j < ACT_CANDIDATES; j++) {
        const float q = x[j * sx] + e;
        const float l = logf(q <= e ? e : q);
        s += q * l;
        g[j * sg] = -(l + (q > e ? 1.0f : 0.0f));
    }
    const float H = -s;
    const float under = la.floor - H;
    const float bonus0 = H - la.cf * (under < 0.0f ? 0.0f : under);
    const float bonus = bonus0 + la.cr * (la.hmax - bonus0);
    const float rp = (p >= e ? 1.0f : 0.0f) / den;
    const float dpl = ra <= ca ? A * rp : A * rp * (cl == ratio ? 1.0f : 0.0f);
    const float ce = ((-(la.c3 / D)) * (1.0f - la.cr)) * (1.0f + (H < la.floor ? la.cf : 0.0f));
    const float pp = (-(la.c2 / D)) * dpl;
    for (int j = 0; j < ACT_CANDIDATES; j++) {
        float v = ce * g[j * sg];
        if (j == c) v = v + pp;
        g[j * sg] = v * la.grad_scale;
    }
    const float dv = val - T;
    gv = (((2.0f * la.c1) * dv) / D) * la.grad_scale;
    sum[0] = dv * dv; sum[1] = pl; sum[2] = bonus; sum[3] = H; sum[4] = H * H; sum[5] = val; sum[6] = val * val;
    sum[7] = T; sum[8] = T * T; sum[9] = ratio != cl ? 1.0f : 0.0f; sum[10] = ratio; sum[11] = 0.0f;
    if (la.terms) {
        const size_t M = (size_t)la.M;
        la.terms[m] = p; la.terms[M + m] = ratio; la.terms[2 * M + m] = pl; la.terms[3 * M + m] = H; la.terms[4 * M + m] = bonus;
        la.terms[5 * M + m] = val;
    }
}

// DQN: valid sample m with candidate c -> g[40] (zeros but g[c]), the sample's terms of the sums, new_prio and q
TE_HD void loss_dqn_sample(const LossArgs& la, size_t m, int c, float Dnz, const float* x, int sx, float* g, int sg, float* sum) {
    const float q = x[c * sx], T = la.target[m], w = la.weight ? la.weight[m] : 1.0f;
    const float d = q - T;
    float prio = u2f(f2u(d) & 0x7FFFFFFFu);
    if (la.optimistic != 0.0f) prio = prio + la.optimistic * (prio < 0.0f ? 0.0f : prio);
    for (int j = 0; j < ACT_CANDIDATES; j++) g[j * sg] = 0.0f;
    g[c * sg] = Dnz > 0.0f ? (((2.0f * w) * d) / Dnz) * la.grad_scale : 0.0f;
    sum[0] = w * (d * d); sum[1] = q; sum[2] = q * q; sum[3] = T; sum[4] = T * T; sum[5] = prio;
    TE_UNROLL
    for (int i = 6; i < LOSS_SUMS; i++) sum[i] = 0.0f;
    la.new_prio[m] = prio;
    if (la.q) la.q[m] = q;
}

// Sample m of either head from its plane x: g[40], gv, sum[LOSS_SUMS]; a sample past M or not valid: zeros (and zeros in its
// per-sample outputs when it lies inside M).  D, Dnz as floats.
TE_HD void loss_sample(const LossArgs& la, long long m, int k, int c, float D, float Dnz, const float* x, int sx, float* g, int sg, float* sum, float& gv) {
    const bool inside = m < (long long)la.M;
    if (inside && loss_valid(la, (size_t)m)) {
        gv = 0.0f;
        if (la.head == LOSS_PPO) loss_ppo_sample(la, (size_t)m, k, c, D, x, sx, g, sg, sum, gv);
        else loss_dqn_sample(la, (size_t)m, c, Dnz, x, sx, g, sg, sum);
        return;
    }
    loss_zero_sample(g, sg, sum, gv);
    if (!inside) return;
    const size_t M = (size_t)la.M, at = (size_t)m;
    if (la.head == LOSS_PPO) {
        if (la.terms)
            for (int i = 0; i < LOSS_PPO_TERMS; i++) la.terms[i * M + at] = 0.0f;
    } else {
        la.new_prio[at] = 0.0f;
        if (la.q) la.q[at] = 0.0f;
    }
}

// the statistics from the sums over all samples
TE_HD void loss_finish(const LossArgs& la, const float* total, float D, float Dnz, float* stats) {
    TE_UNROLL
    for (int i = 0; i < LOSS_STATS; i++) stats[i] = 0.0f;
    if (!(D > 0.0f)) return;
    stats[0] = D;
    if (la.head == LOSS_PLAN) {
        const float vl = la.c1 * (total[0] / D), pol = (-la.c2) * (total[1] / D), ent = (-la.c3) * (total[2] / D);
        const float imp = la.c4 * ((total[11] / D) / (float)(la.H * NCOL));
        stats[1] = ((vl + pol) + imp) + ent; stats[2] = vl; stats[3] = pol; stats[4] = ent; stats[5] = imp;
        stats[6] = total[2] / D; stats[7] = total[3] / D; stats[8] = total[4] / D; stats[9] = total[5] / D; stats[10] = total[6] / D;
        stats[11] = total[7] / D; stats[12] = total[8] / D; stats[13] = total[9] / D; stats[14] = total[10] / D;
    } else if (la.head == LOSS_PPO) {
        const float vl = la.c1 * (total[0] / D), pol = (-la.c2) * (total[1] / D), ent = (-la.c3) * (total[2] / D);
        stats[1] = (vl + pol) + ent; stats[2] = vl; stats[3] = pol; stats[4] = ent;
        stats[5] = total[3] / D; stats[6] = total[4] / D; stats[7] = total[2] / D; stats[8] = total[5] / D; stats[9] = total[6] / D;
        stats[10] = total[7] / D; stats[11] = total[8] / D; stats[12] = total[9] / D; stats[13] = total[10] / D;
    } else {
        stats[1] = Dnz;
        stats[2] = Dnz > 0.0f ? total[0] / Dnz : 0.0f;
        stats[3] = total[1] / D; stats[4] = total[2] / D; stats[5] = total[3] / D; stats[6] = total[4] / D; stats[7] = total[5] / D;
    }
}

// element `at` of a gradient array
TE_HD void loss_store(void* out, size_t at, float v, int f16) {
    if (f16) ((uint16_t*)out)[at] = plan_f32_to_f16(v);
    else ((float*)out)[at] = v;
}

// ---- serial forms (CPU harness; the kernels spread the same steps over a workgroup)
// block b: its samples' outputs, their whole gradient rows, and its partial row
TE_HD void loss_block_serial(const LossArgs& la, int b, float D, float Dnz) {
    float lanes[LOSS_SUMS][LOSS_BLOCK];
    for (int t = 0; t < LOSS_BLOCK; t++) {
        const long long m = (long long)b * LOSS_BLOCK + t;
        float x[ACT_CANDIDATES], g[ACT_CANDIDATES], sum[LOSS_SUMS], gv;
        int k = 0, c = 0;
        if (m < (long long)la.M) {
            loss_action(la, (size_t)m, k, c);
            for (int j = 0; j < ACT_CANDIDATES; j++) x[j] = act_element(la.x, ((size_t)m * ACT_CANDIDATES + j) * la.K + k, la.in_f16);
        }
        loss_sample(la, m, k, c, D, Dnz, x, 1, g, 1, sum, gv);
        for (int i = 0; i < LOSS_SUMS; i++) lanes[i][t] = sum[i];
        if (m >= (long long)la.M) continue;
        for (int j = 0; j < ACT_CANDIDATES; j++)
            for (int kk = 0; kk < la.K; kk++)
                loss_store(la.grad_x, ((size_t)m * ACT_CANDIDATES + j) * la.K + kk, kk == k ? g[j] : 0.0f, la.grad_f16);
        if (la.head == LOSS_PPO)
            for (int kk = 0; kk < la.V; kk++) loss_store(la.grad_v, (size_t)m * la.V + kk, kk == imin(k, la.V - 1) ? gv : 0.0f, la.grad_f16);
    }
    for (int i = 0; i < LOSS_SUMS; i++) la.partial[(size_t)b * LOSS_SUMS + i] = loss_tree(lanes[i], LOSS_BLOCK);
}

// ---- PLAN: the pieces a lane of the kernel and the serial form share.  A sample's work is: per cell plan_cell and its four
// terms -> SUM -> plan_sample_policy -> per cell plan_cell_entropy -> SUM -> plan_sample_finish -> per cell plan_cell_grad.
TE_HD int plan_loss_blocks(int M) { return (M + PLAN_LOSS_BLOCK - 1) / PLAN_LOSS_BLOCK; }
TE_HD int loss_blocks_of(const LossArgs& la) { return la.head == LOSS_PLAN ? plan_loss_blocks(la.M) : loss_blocks(la.M); }
TE_HD int plan_loss_piece(const LossArgs& la, size_t m) { return imin((int)la.piece[m * (size_t)la.piece_stride], la.K - 1); }

struct PlanCell { float x, d, s, b, m1; bool pass; };
// cell t of a sample from its raw phi and its record r (zeros for an entry that names none)
TE_HD PlanCell plan_cell(const uint32_t* r, bool mirror, int t, float raw, float small_fill) {
    const float e = 1e-6f;
    const int y = t / NCOL, c = t - y * NCOL;
    PlanCell pc;
    const float lowc = raw > 1.0f ? 1.0f : raw;
    pc.x = lowc < e ? e : lowc;
    pc.pass = e <= raw && raw <= 1.0f;
    pc.d = plan_rec_delta(r, mirror, y, c, small_fill);
    pc.s = plan_rec_sums(r, mirror, y, c, small_fill);
    pc.b = pc.x * pc.s;
    pc.m1 = pc.s < 1.0f ? pc.s : 1.0f;
    return pc;
}
// a_t, b_t, u_t, i_t
TE_HD void plan_cell_terms(const PlanCell& pc, float* four) {
    four[0] = pc.x * pc.d; four[1] = pc.b; four[2] = pc.s + 1e-6f; four[3] = pc.x * (1.0f - pc.m1);
}
struct PlanSample { float probability, den2, ratio, cl, pl, val, dv, S, Hent, pp, ci, ce; };
// after the first four sums
TE_HD void plan_sample_policy(const LossArgs& la, size_t m, int k, float D, float num, float dn, float S, PlanSample& ps) {
    const float e = 1e-6f;
    const float old = la.old[m], A = la.adv[m];
    ps.val = act_element(la.v, m * (size_t)la.V + (size_t)imin(k, la.V - 1), la.v_f16);
    ps.dv = ps.val - la.target[m];
    ps.S = S;
    ps.den2 = dn + e;
    ps.probability = (num + e) / ps.den2;
    const float p = ps.probability;
    const float den = old < e ? e : old;
    ps.ratio = (p < e ? e : p) / den;
    const float lo = 1.0f - la.clip, hi = 1.0f + la.clip;
    const float low = ps.ratio < lo ? lo : ps.ratio;
    ps.cl = low > hi ? hi : low;
    const float ra = ps.ratio * A, ca = ps.cl * A;
    ps.pl = ca < ra ? ca : ra;
    const float rp = (p >= e ? 1.0f : 0.0f) / den;
    const float dpl = ra <= ca ? A * rp : A * rp * (ps.cl == ps.ratio ? 1.0f : 0.0f);
    ps.pp = (-(la.c2 / D)) * dpl;
    ps.ci = (la.c4 / D) / (float)(la.H * NCOL);
    ps.ce = -(la.c3 / D);
}
// y_t l_t of the entropy sum; l_t and [y_t > e] are kept for the gradient
TE_HD float plan_cell_entropy(const PlanCell& pc, float S, float& l, float& above) {
    const float e = 1e-6f;
    const float y = pc.b / S + e;
    l = logf(y <= e ? e : y);
    above = y > e ? 1.0f : 0.0f;
    return y * l;
}
TE_HD float plan_cell_grad(const LossArgs& la, const PlanSample& ps, const PlanCell& pc, float l, float above) {
    const float dp = (pc.d - ps.probability * pc.s) / ps.den2;
    const float w = pc.s / ps.S;
    const float et = -(l + above);
    const float g = ((ps.pp * dp) + (ps.ci * (1.0f - pc.m1))) + (ps.ce * (et * w));
    return pc.pass ? g * la.grad_scale : 0.0f;
}
// the sample's terms of the statistics, its value gradient and its row of d_terms
TE_HD void plan_sample_finish(const LossArgs& la, size_t m, float D, const PlanSample& ps, float I, float* sum, float& gv) {
    const float T = la.target[m];
    gv = (((2.0f * la.c1) * ps.dv) / D) * la.grad_scale;
    sum[0] = ps.dv * ps.dv; sum[1] = ps.pl; sum[2] = ps.Hent; sum[3] = ps.Hent * ps.Hent; sum[4] = ps.val; sum[5] = ps.val * ps.val;
    sum[6] = T; sum[7] = T * T; sum[8] = ps.ratio != ps.cl ? 1.0f : 0.0f; sum[9] = ps.ratio; sum[10] = ps.probability; sum[11] = I;
    if (la.terms) {
        const size_t M = (size_t)la.M;
        la.terms[m] = ps.probability; la.terms[M + m] = ps.ratio; la.terms[2 * M + m] = ps.pl; la.terms[3 * M + m] = ps.Hent;
        la.terms[4 * M + m] = I; la.terms[5 * M + m] = ps.val;
    }
}
// a sample inside M that is not valid: zeros in its row of d_terms
TE_HD void plan_sample_zero_terms(const LossArgs& la, size_t m) {
    if (la.terms)
        for (int i = 0; i < PLAN_LOSS_TERMS; i++) la.terms[i * (size_t)la.M + m] = 0.0f;
}

// Serial form of sample m (< M) from its piece's plane raw[HW] -> g[HW], gv, sum[LOSS_SUMS]
TE_HD void plan_loss_sample_serial(const LossArgs& la, size_t m, int k, float D, const float* raw, float* g, float* sum, float& gv) {
    const int HW = la.H * NCOL;
    gv = 0.0f;
    for (int i = 0; i < LOSS_SUMS; i++) sum[i] = 0.0f;
    for (int t = 0; t < HW; t++) g[t] = 0.0f;
    if (!loss_valid(la, m) || !(D > 0.0f)) {
        plan_sample_zero_terms(la, m);
        return;
    }
    const BatchEntry en = batch_index_entry((uint32_t)la.index[m], la.total);
    const uint32_t* r = la.rec + (size_t)en.at * PLAN_REC_WORDS;
    float lanes[5][PLAN_LOSS_LANES];
    for (int lane = 0; lane < PLAN_LOSS_LANES; lane++) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int t = lane; t < HW; t += PLAN_LOSS_LANES) {
            float four[4];
            plan_cell_terms(plan_cell(r, en.mirror, t, raw[t], la.small_fill), four);
            for (int i = 0; i < 4; i++) acc[i] += four[i];
        }
        for (int i = 0; i < 4; i++) lanes[i][lane] = acc[i];
    }
    float total[4];
    for (int i = 0; i < 4; i++) total[i] = loss_tree(lanes[i], PLAN_LOSS_LANES);
    PlanSample ps;
    plan_sample_policy(la, m, k, D, total[0], total[1], total[2], ps);
    float l[MAX_H * NCOL], above[MAX_H * NCOL];
    for (int lane = 0; lane < PLAN_LOSS_LANES; lane++) {
        float acc = 0.0f;
        for (int t = lane; t < HW; t += PLAN_LOSS_LANES) acc += plan_cell_entropy(plan_cell(r, en.mirror, t, raw[t], la.small_fill), ps.S, l[t], above[t]);
        lanes[4][lane] = acc;
    }
    ps.Hent = -loss_tree(lanes[4], PLAN_LOSS_LANES);
    for (int t = 0; t < HW; t++) g[t] = plan_cell_grad(la, ps, plan_cell(r, en.mirror, t, raw[t], la.small_fill), l[t], above[t]);
    plan_sample_finish(la, m, D, ps, total[3], sum, gv);
}

// block b of the planning head: its samples' outputs, their whole gradient rows, and its partial row
TE_HD void plan_loss_block_serial(const LossArgs& la, int b, float D) {
    const int HW = la.H * NCOL;
    float lanes[LOSS_SUMS][PLAN_LOSS_BLOCK];
    for (int t = 0; t < PLAN_LOSS_BLOCK; t++) {
        const long long m = (long long)b * PLAN_LOSS_BLOCK + t;
        float raw[MAX_H * NCOL], g[MAX_H * NCOL], sum[LOSS_SUMS], gv = 0.0f;
        for (int i = 0; i < LOSS_SUMS; i++) sum[i] = 0.0f;
        if (m < (long long)la.M) {
            const int k = plan_loss_piece(la, (size_t)m);
            for (int j = 0; j < HW; j++) raw[j] = act_element(la.x, ((size_t)m * HW + j) * la.K + k, la.in_f16);
            plan_loss_sample_serial(la, (size_t)m, k, D, raw, g, sum, gv);
            for (int j = 0; j < HW; j++)
                for (int kk = 0; kk < la.K; kk++) loss_store(la.grad_x, ((size_t)m * HW + j) * la.K + kk, kk == k ? g[j] : 0.0f, la.grad_f16);
            for (int kk = 0; kk < la.V; kk++) loss_store(la.grad_v, (size_t)m * la.V + kk, kk == imin(k, la.V - 1) ? gv : 0.0f, la.grad_f16);
        }
        for (int i = 0; i < LOSS_SUMS; i++) lanes[i][t] = sum[i];
    }
    for (int i = 0; i < LOSS_SUMS; i++) la.partial[(size_t)b * LOSS_SUMS + i] = loss_tree(lanes[i], PLAN_LOSS_BLOCK);
}

// the partial rows of `blocks` workgroups -> stats
TE_HD void loss_reduce_serial(const LossArgs& la, int blocks, float D, float Dnz) {
    float total[LOSS_SUMS];
    for (int i = 0; i < LOSS_SUMS; i++) {
        float slot[LOSS_REDUCE_LANES];
        for (int t = 0; t < LOSS_REDUCE_LANES; t++) {
            float s = 0.0f;
            for (int b = t; b < blocks; b += LOSS_REDUCE_LANES) s += la.partial[(size_t)b * LOSS_SUMS + i];
            slot[t] = s;
        }
        total[i] = loss_tree(slot, LOSS_REDUCE_LANES);
    }
    loss_finish(la, total, D, Dnz, la.stats);
}

}  // namespace te
