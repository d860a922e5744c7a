// Kernel bodies of the network's output heads (include/tetris_hip.h: tetris_q_head_dev, tetris_q_head_grad_dev,
// tetris_policy_head_dev, tetris_policy_head_grad_dev): the fixed arithmetic between a trunk's raw streams and the arrays the
// acting and loss entry points read, with its backward.  The Q head is qva_from_raw_streams (agents/networks/network_utils.py:
// 100-104) as base_architecture.py:53-62 calls it — advantage_range * _A through normalize_advantages (network_utils.py:8-35),
// tanh, Q = _V + A, V = q_to_v(Q) (network_utils.py:95-98).  The policy head is ppo_nets.py:24-33: action_softmax
// (network_utils.py:120-125) over the 40 (r, t) of each piece, and normalize_advantages(_V, tanh, axis=3, inplace=True) of the
// [M, K + 1] value stream (sventon_architectures.py:50).
//
// `__host__ __device__` like tetris_loss.h: tetris_hip.hip wraps these in gfx950 kernels (k_q_head, k_q_head_grad, k_policy_head,
// k_policy_head_grad: tetris_dev_head.h), the CPU harness (tests/cpu_harness) runs them through head_run_serial
// (tetris_host.h) in plain host loops.  float32 throughout, -ffp-contract=off (no fused multiply-adds), the division correctly
// rounded, tanhf and expf the only library calls; every expression below is evaluated in the order it is written, so host and
// device give the same bits but for tanhf and expf.  No atomics: the same call twice gives the same bits.
//
// COMMON.  A sample is 40 K elements x_jk, j = 10 r + t, k the piece, K = 7 or 1, at [m][j][k]; float32, or binary16 (the F16
// flag covers every [M][4][10][K] array of a call, the VALUE_F16 flag every per-sample value array).  A binary16 input is widened
// exactly, an output is rounded to nearest even.  Every sum starts at +0 and adds in ascending index order: over j, then over k.
// max over j is `m = x_0k; for j = 1..39: m = m < x_jk ? x_jk : m`, min likewise with `x_jk < m ? x_jk : m`; over k the same in
// ascending k.  A NaN input gives an unspecified result (no access leaves the arrays whatever the bits).  mask_k = bit k of
// used_pieces, U = (float)popcount(used_pieces); K = 1: used_pieces = 1, U = 1 (create_used_pieces_mask and the
// `piece_mask == 1.0` line of normalize_advantages).  [c] is 1 where c holds, else 0; == compares values (+0 == -0).
//
// Q HEAD, FORWARD.  rho = advantage_range, mode MEAN / MAX / NONE (NONE: what normalize_advantages does for any other string).
//   a_jk = rho a_raw_jk.  v_k = v[m][min(k, Kv - 1)], Kv = 1 or K; v == NULL: v_k = +0 (full_network=False: prio_qnet).
//   MEAN:  mu_k = (sum_j a_jk) / 40;  c = (sum_k mask_k mu_k) / U  (the sum adds the used k only);  d_jk = a_jk - c for EVERY piece.
//   MAX:   lo = min over all (j, k) of a_jk — per piece over j, then over k —, unused pieces included;
//          mx_k = mask_k ? max_j a_jk : lo  (the reference's max over b_jk = mask_k ? a_jk : lo);
//          separate_piece_values: d_jk = a_jk - mx_k;  otherwise c = (sum_k mask_k mx_k) / U, d_jk = a_jk - c.
//   NONE:  d_jk = a_jk.
//   A_jk = tanhf(d_jk);  Q_jk = v_k + A_jk.  Q and A are stored in the element type of the call.
//   V = (sum_k mask_k mq_k) / U with mq_k = max_j Q_jk OF THE STORED Q (binary16: after its rounding), so V is q_to_v of the array
//   the caller holds, exactly.  V is float32 [M].
// Q HEAD, BACKWARD: the gradient of sum G_jk Q_jk with respect to a_raw and v, G = grad_Q.  V and A are forward-only outputs: no
// gradient flows through them (the reference's trainers differentiate Q only).  d, A are recomputed from a_raw — the same function
// of the same input gives the same bits on the same device — so no third stream is read.
//   grad_v: Kv = K: grad_v[m][k] = sum_j G_jk;  Kv = 1: grad_v[m][0] = sum_k (sum_j G_jk), all pieces.
//   gd_jk = G_jk (1 - A_jk A_jk);  S_k = sum_j gd_jk;  S = sum_k S_k (all pieces).
//   n_k = #{j : a_jk == mx_k}, n_lo = #{(j, k) : a_jk == lo}: ties share equally (TensorFlow's reduce_max / reduce_min gradient,
//   torch's amax / amin).
//   NONE:          ga_jk = gd_jk.
//   MEAN:          ga_jk = mask_k ? gd_jk - (S / 40) / U : gd_jk.
//   MAX joint:     ga_jk = mask_k && a_jk == mx_k ? gd_jk - (S / U) / n_k : gd_jk.
//   MAX separate:  ga_jk = mask_k && a_jk == mx_k ? gd_jk - S_k / n_k : gd_jk;  then, with R = sum over the unused k of S_k — their
//                  planes lean on lo —, every (j, k) with a_jk == lo, used or not: ga_jk = ga_jk - R / n_lo.
//   grad_a_jk = rho ga_jk.
//
// POLICY HEAD, FORWARD.  x = the logits [M][4][10][K], w = the value stream [M][W], W = 1 or K + 1.
//   mx_k = max_j x_jk;  u_jk = expf(x_jk - mx_k);  s_k = sum_j u_jk;  pi_jk = u_jk / s_k.
//   W = 1: v_0 = tanhf(w_0) (the reference's corner case).  W = K + 1: c = (sum_{k = 1..K} w_k) / K;  v_(k-1) = tanhf(w_0 + (w_k - c)):
//   v is [M][K].  This is the reference's mean over ALL K entries, used or not: with axis=3 the mean is taken along the piece axis
//   itself, _mean_a is one number c per sample, and its mask cancels: (sum_k mask_k c) / U = c.  The reference evaluates that
//   identity in float32 — U additions of c and a division — and can land one unit in the last place of c beside it; here c is
//   used as it is.
// POLICY HEAD, BACKWARD, from the stored outputs pi and v and the gradients g = grad_pi, gv = grad_v.  No library call:
//   dot_k = sum_j g_jk pi_jk;  grad_x_jk = pi_jk (g_jk - dot_k).
//   gt_k = gv_k (1 - v_k v_k).  W = 1: grad_w_0 = gt_0.  W = K + 1: T = sum_k gt_k;  grad_w_0 = T;  grad_w_k = gt_(k-1) - T / K.
//
// OUTPUTS.  Every element of every output that is given is written, nothing past M.
#pragma once
#include <math.h>

#include "tetris_act.h"
#include "tetris_loss.h"

namespace te {

constexpr int HEAD_Q = 0, HEAD_POLICY = 1;
constexpr int HEAD_MEAN = TETRIS_HEAD_MEAN, HEAD_MAX = TETRIS_HEAD_MAX, HEAD_NONE = TETRIS_HEAD_NONE;
constexpr int HEAD_BLOCK = 16;                   // samples per workgroup
constexpr int HEAD_THREADS = 256;                // its threads: at K = 7 a thread per (sample, piece) for 112 of them
constexpr int HEAD_PIECES = 8;                   // floats of a sample's per-piece numbers in LDS
constexpr int HEAD_PER = ACT_CANDIDATES * 7;     // elements of a sample at most

struct HeadArgs {
    int head, grad;              // HEAD_Q / HEAD_POLICY; 0: forward, 1: backward
    int M, K, W;                 // samples, n_pieces; Q: Kv (0: no v), policy: the width of w
    int mode, separate, f16, v_f16;
    uint32_t mask;               // used_pieces
    float U, rho;
    const void* x;               // Q: a_raw; policy: the logits (forward), pi (backward)
    const void* v;               // Q: v [M][Kv] or NULL; policy: w [M][W] (forward), v (backward)
    const void* g;               // backward: grad_Q / grad_pi
    const void* gv;              // policy backward: grad_v
    void* out;                   // Q / pi (forward), grad_a / grad_x (backward)
    void* out_v;                 // policy: v (forward), grad_w (backward); Q backward: grad_v or NULL
    void* out_A;                 // Q forward: A or NULL
    float* V;                    // Q forward: [M]
};

TE_HD int head_blocks(int M) { return (M + HEAD_BLOCK - 1) / HEAD_BLOCK; }
TE_HD bool head_used(const HeadArgs& h, int k) { return ((h.mask >> k) & 1u) != 0u; }
// the value as the call's big arrays hold it
TE_HD float head_rounded(float v, int f16) { return f16 ? act_f16_to_f32(plan_f32_to_f16(v)) : v; }

// plane k of a sample's image x[j * K + k]: its sum, its maximum and minimum and how many elements equal them
struct HeadPlane { float sum, mx, mn; int nmx, nmn; };
TE_HD HeadPlane head_plane(const float* x, int K, int k) {
    HeadPlane p;
    const float x0 = x[k];
    p.sum = 0.0f + x0; p.mx = x0; p.mn = x0; p.nmx = 1; p.nmn = 1;
    for (int j = 1; j < ACT_CANDIDATES; j++) {
        const float v = x[j * K + k];
        p.sum += v;
        if (p.mx < v) { p.mx = v; p.nmx = 1; } else if (v == p.mx) p.nmx++;
        if (v < p.mn) { p.mn = v; p.nmn = 1; } else if (v == p.mn) p.nmn++;
    }
    return p;
}
TE_HD float head_plane_max(const float* x, int K, int k) {
    float m = x[k];
    for (int j = 1; j < ACT_CANDIDATES; j++) {
        const float v = x[j * K + k];
        m = m < v ? v : m;
    }
    return m;
}
TE_HD float head_plane_sum(const float* x, int K, int k) {
    float s = 0.0f;
    for (int j = 0; j < ACT_CANDIDATES; j++) s += x[j * K + k];
    return s;
}
// sum_j g_jk x_jk
TE_HD float head_plane_dot(const float* g, const float* x, int K, int k) {
    float s = 0.0f;
    for (int j = 0; j < ACT_CANDIDATES; j++) s += g[j * K + k] * x[j * K + k];
    return s;
}

// ---- Q head.  What a sample's elements need of its planes: what is subtracted from piece k, the planes' maxima and the minimum
// for the tie tests, v_k, and in the backward pass the shares
struct HeadQSample {
    float sub[HEAD_PIECES], mx[HEAD_PIECES], v[HEAD_PIECES], share[HEAD_PIECES];
    float lo, rshare;
    int nlo;
};
TE_HD void head_q_center(const HeadArgs& h, size_t m, const HeadPlane* p, HeadQSample& q) {
    for (int k = 0; k < h.K; k++) {
        q.sub[k] = 0.0f; q.mx[k] = p[k].mx; q.share[k] = 0.0f;
        q.v[k] = h.v ? act_element(h.v, m * (size_t)h.W + (size_t)imin(k, h.W - 1), h.v_f16) : 0.0f;
    }
    q.lo = 0.0f; q.rshare = 0.0f; q.nlo = 1;
    if (h.mode == HEAD_MEAN) {
        float c = 0.0f;
        for (int k = 0; k < h.K; k++)
            if (head_used(h, k)) c += p[k].sum / 40.0f;
        c = c / h.U;
        for (int k = 0; k < h.K; k++) q.sub[k] = c;
    } else if (h.mode == HEAD_MAX) {
        float lo = p[0].mn;
        for (int k = 1; k < h.K; k++) lo = p[k].mn < lo ? p[k].mn : lo;
        int nlo = 0;
        for (int k = 0; k < h.K; k++) nlo += p[k].mn == lo ? p[k].nmn : 0;
        q.lo = lo; q.nlo = nlo;
        float c = 0.0f;
        for (int k = 0; k < h.K; k++) {
            q.mx[k] = head_used(h, k) ? p[k].mx : lo;
            if (head_used(h, k)) c += q.mx[k];
        }
        c = c / h.U;
        for (int k = 0; k < h.K; k++) q.sub[k] = h.separate ? q.mx[k] : c;
    }
}
TE_HD float head_q_A(const HeadArgs& h, float a, float sub) { return tanhf(h.mode == HEAD_NONE ? a : a - sub); }
// V from the planes' maxima of the stored Q
TE_HD float head_q_value(const HeadArgs& h, const float* mq) {
    float s = 0.0f;
    for (int k = 0; k < h.K; k++)
        if (head_used(h, k)) s += mq[k];
    return s / h.U;
}
// grad_v of sample m from sum_j G_jk
TE_HD void head_q_grad_v(const HeadArgs& h, size_t m, const float* sg) {
    if (!h.out_v) return;
    if (h.W == 1) {
        float s = 0.0f;
        for (int k = 0; k < h.K; k++) s += sg[k];
        loss_store(h.out_v, m, s, h.v_f16);
    } else {
        for (int k = 0; k < h.K; k++) loss_store(h.out_v, m * (size_t)h.K + (size_t)k, sg[k], h.v_f16);
    }
}
TE_HD float head_q_gd(float G, float A) { return G * (1.0f - A * A); }
// the shares from S_k = sum_j gd_jk; p[k].nmx = n_k
TE_HD void head_q_shares(const HeadArgs& h, const float* S, const HeadPlane* p, HeadQSample& q) {
    float total = 0.0f, R = 0.0f;
    for (int k = 0; k < h.K; k++) {
        total += S[k];
        if (!head_used(h, k)) R += S[k];
    }
    for (int k = 0; k < h.K; k++) {
        float s = 0.0f;
        if (head_used(h, k)) {
            if (h.mode == HEAD_MEAN) s = (total / 40.0f) / h.U;
            else if (h.mode == HEAD_MAX) s = h.separate ? S[k] / (float)p[k].nmx : (total / h.U) / (float)p[k].nmx;
        }
        q.share[k] = s;
    }
    q.rshare = R / (float)q.nlo;
}
TE_HD float head_q_grad_a(const HeadArgs& h, const HeadQSample& q, int k, float a, float gd) {
    float ga = gd;
    if (h.mode == HEAD_MEAN) {
        if (head_used(h, k)) ga = gd - q.share[k];
    } else if (h.mode == HEAD_MAX) {
        if (head_used(h, k) && a == q.mx[k]) ga = gd - q.share[k];
        if (h.separate && a == q.lo) ga = ga - q.rshare;
    }
    return h.rho * ga;
}

// ---- policy head: the value stream of sample m (a thread per sample in the kernels)
TE_HD void head_policy_value(const HeadArgs& h, size_t m) {
    if (h.W == 1) {
        loss_store(h.out_v, m, tanhf(act_element(h.v, m, h.v_f16)), h.v_f16);
        return;
    }
    const size_t at = m * (size_t)h.W;
    const float w0 = act_element(h.v, at, h.v_f16);
    float c = 0.0f;
    for (int k = 1; k <= h.K; k++) c += act_element(h.v, at + (size_t)k, h.v_f16);
    c = c / (float)h.K;
    for (int k = 1; k <= h.K; k++)
        loss_store(h.out_v, m * (size_t)h.K + (size_t)(k - 1), tanhf(w0 + (act_element(h.v, at + (size_t)k, h.v_f16) - c)), h.v_f16);
}
TE_HD float head_policy_gt(const HeadArgs& h, size_t at) {
    const float v = act_element(h.v, at, h.v_f16), gv = act_element(h.gv, at, h.v_f16);
    return gv * (1.0f - v * v);
}
TE_HD void head_policy_value_grad(const HeadArgs& h, size_t m) {
    if (h.W == 1) {
        loss_store(h.out_v, m, head_policy_gt(h, m), h.v_f16);
        return;
    }
    const size_t at = m * (size_t)h.K;
    float T = 0.0f;
    for (int k = 0; k < h.K; k++) T += head_policy_gt(h, at + (size_t)k);
    loss_store(h.out_v, m * (size_t)h.W, T, h.v_f16);
    const float share = T / (float)h.K;
    for (int k = 0; k < h.K; k++) loss_store(h.out_v, m * (size_t)h.W + (size_t)(k + 1), head_policy_gt(h, at + (size_t)k) - share, h.v_f16);
}

// ---- serial forms of a sample (CPU harness; the kernels spread the same steps over a workgroup's LDS image of HEAD_BLOCK samples)
TE_HD void head_load_sample(const void* src, size_t m, int K, int f16, float scale, float* x) {
    const size_t per = (size_t)ACT_CANDIDATES * K;
    for (size_t e = 0; e < per; e++) x[e] = act_element(src, m * per + e, f16) * scale;
}

TE_HD void head_q_sample_serial(const HeadArgs& h, size_t m) {
    const int K = h.K, per = ACT_CANDIDATES * K;
    float a[HEAD_PER];
    HeadPlane p[HEAD_PIECES];
    HeadQSample q;
    head_load_sample(h.x, m, K, h.f16, h.rho, a);
    for (int k = 0; k < K; k++) p[k] = head_plane(a, K, k);
    head_q_center(h, m, p, q);
    if (!h.grad) {
        for (int e = 0; e < per; e++) {
            const int k = e % K;
            const float A = head_q_A(h, a[e], q.sub[k]), Q = q.v[k] + A;
            if (h.out_A) loss_store(h.out_A, m * (size_t)per + e, A, h.f16);
            loss_store(h.out, m * (size_t)per + e, Q, h.f16);
            a[e] = head_rounded(Q, h.f16);
        }
        float mq[HEAD_PIECES];
        for (int k = 0; k < K; k++) mq[k] = head_plane_max(a, K, k);
        h.V[m] = head_q_value(h, mq);
        return;
    }
    float g[HEAD_PER], S[HEAD_PIECES];
    head_load_sample(h.g, m, K, h.f16, 1.0f, g);
    for (int k = 0; k < K; k++) S[k] = head_plane_sum(g, K, k);
    head_q_grad_v(h, m, S);
    for (int e = 0; e < per; e++) g[e] = head_q_gd(g[e], head_q_A(h, a[e], q.sub[e % K]));
    for (int k = 0; k < K; k++) S[k] = head_plane_sum(g, K, k);
    head_q_shares(h, S, p, q);
    for (int e = 0; e < per; e++) loss_store(h.out, m * (size_t)per + e, head_q_grad_a(h, q, e % K, a[e], g[e]), h.f16);
}

TE_HD void head_policy_sample_serial(const HeadArgs& h, size_t m) {
    const int K = h.K, per = ACT_CANDIDATES * K;
    float x[HEAD_PER];
    head_load_sample(h.x, m, K, h.f16, 1.0f, x);
    if (!h.grad) {
        float red[HEAD_PIECES];
        for (int k = 0; k < K; k++) red[k] = head_plane_max(x, K, k);
        for (int e = 0; e < per; e++) x[e] = expf(x[e] - red[e % K]);
        for (int k = 0; k < K; k++) red[k] = head_plane_sum(x, K, k);
        for (int e = 0; e < per; e++) loss_store(h.out, m * (size_t)per + e, x[e] / red[e % K], h.f16);
        head_policy_value(h, m);
        return;
    }
    float g[HEAD_PER], dot[HEAD_PIECES];
    head_load_sample(h.g, m, K, h.f16, 1.0f, g);
    for (int k = 0; k < K; k++) dot[k] = head_plane_dot(g, x, K, k);
    for (int e = 0; e < per; e++) loss_store(h.out, m * (size_t)per + e, x[e] * (g[e] - dot[e % K]), h.f16);
    head_policy_value_grad(h, m);
}

}  // namespace te
