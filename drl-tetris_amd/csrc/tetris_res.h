// Kernel bodies of one layer of the reference's residual_block (include/tetris_hip.h: tetris_res_layer_dev,
// tetris_res_layer_grad_x_dev, tetris_res_layer_grad_w_dev): agents/networks/builders/build_blocks.py:8-64 — each layer is
// conv2d(3 x 3, 'same'), then peephole_join(x, y, mode = "add" | "truncate_add") (agents/networks/network_utils.py:52-64), then
// elu — with its backward.  resblock / resblock_kbd stack three such blocks in front of the advantage stream
// (agents/networks/builders/sventon_architectures.py:31, 36, 40).
//
// `__host__ __device__` like tetris_kbd.h: the serial forms below are what the CPU harness (tests/cpu_harness) runs through
// res_run_serial (tetris_host.h); tetris_hip.hip computes the same sums on the matrix cores of gfx950 (tetris_dev_res.h) in an
// order of its own.
//
// SHAPES.  The image is 12 columns wide, Hp rows in 4..33.  Ci is a multiple of 8 in 8..512 (8 consecutive channels are one
// fragment of the matrix unit, so a fragment never straddles a kernel tap and every image row is 16-byte aligned in both element
// types); Co is a multiple of 32 in 32..512.
//   x     [M][Hp][12][Ci]     NHWC (the memory of a channels_last torch tensor)
//   w     [3][3][Ci][Co]      HWIO, the reference variable's own layout
//   bias  [Co]                float32
//   out   [M][Hp][12][Cout]   Cout = Co (join NONE), max(Ci, Co) (ADD), min(Ci, Co) (TRUNCATE_ADD)
//   y     = out, as saved by the caller: an input of the two gradient calls (read only with ELU)
//   g     [M][Hp][12][Cout]   gradient with respect to out
// x, w, out, y, g and grad_x are float32, or all binary16 with the F16 flag.  bias, grad_w and grad_b are always float32.
//
// FORWARD, for c < Cout, with x read as 0 outside the image:
//   z[m][h][j][o] = bias[o] + sum_(a, b in 0..2) sum_ci x[m][h + a - 1][j + b - 1][ci] w[a][b][ci][o]
//   p[c]          = (c < Co ? z[c] : 0) + (join != NONE and c < Ci ? x[m][h][j][c] : 0)
//   out[c]        = act == ELU ? (p > 0 ? p : expm1f(p)) : p
// This is peephole_join as written in the reference: with ADD and Ci > Co, channels Co..Ci are x passed through (and activated);
// with TRUNCATE_ADD and Co > Ci, the convolution's upper channels are dropped.  Every product and sum is float32, and p is not
// rounded before the activation.  The result is rounded once, to nearest even, to the element type.
//
// GRADIENTS of sum g out:
//   e[c]       = round_T( g[c] (act == ELU and y[c] <= 0 ? y[c] + 1 : 1) )    for c < Cout; round_T is the identity in float32
//                (the product g (y + 1) is formed as fma(g, y, g): one float32 rounding, y + 1 itself is not rounded)
//   gz[o]      = o < min(Co, Cout) ? e[o] : 0
//   grad_x[m][h][j][ci] = sum_(a, b) sum_o gz[m][h - a + 1][j - b + 1][o] w[a][b][ci][o]      (gz = 0 outside the image)
//                         + (join != NONE and ci < Cout ? e[m][h][j][ci] : 0)
//   grad_w[a][b][ci][o] = sum_m sum_h sum_j x[m][h + a - 1][j + b - 1][ci] gz[m][h][j][o]
//   grad_b[o]           = sum_m sum_h sum_j gz[m][h][j][o]
// ELU's derivative is taken from the stored output: exp(p) = y + 1 for p <= 0, and at y = 0 both branches give 1.  e is rounded to
// the element type because that is what the matrix unit consumes in binary16, and what autograd's elu_backward would hand on.
//
// The serial forms sum in ascending (a, b, ci) — the forward from bias[o] —, (a, b, o) and (m, h, j), leaving out the terms
// outside the image.  The order of the device's sums is the matrix unit's and is not specified.  No float atomics on either side: a
// second call gives the same bytes.
//
// OUTPUTS.  Every element of every output is written and nothing past it.  Nothing outside x, w, bias, y or g is read: the zero
// border is never a wrapped or out-of-range read.
#pragma once
#include "tetris_act.h"
#include "tetris_loss.h"

namespace te {

constexpr int RES_FWD = 0, RES_GRAD_X = 1, RES_GRAD_W = 2;
constexpr int RES_JOIN_NONE = 0, RES_JOIN_ADD = 1, RES_JOIN_TRUNCATE_ADD = 2;
constexpr int RES_ACT_NONE = 0, RES_ACT_ELU = 1;
constexpr int RES_W = 12, RES_TAPS = 9, RES_MAX_C = 512;
constexpr int RES_ROWS = 8;            // image rows per workgroup of the forward and grad_x kernels, and per pass of grad_w: 96 positions = six 16-row tiles
constexpr int RES_W_SAMPLES = 64;      // samples per partial sum of grad_w
constexpr int RES_W_CHANNELS = 32;     // input and output channels per workgroup of the grad_w kernel

struct ResArgs {
    int op;                      // RES_FWD / RES_GRAD_X / RES_GRAD_W
    int M, Hp, Ci, Co, Cout, Cz; // Cz = min(Co, Cout): the convolution's channels that reach out
    int join, elu, f16;
    int f16_in;                  // the element type of the arrays read: f16, but 0 where the serial runner has widened them once
    const void* x;               // forward, grad_w; grad_x never reads it
    const void* w;               // forward, grad_x
    const float* bias;           // forward
    const void* y;               // grad_x, grad_w with ELU
    const void* g;               // grad_x, grad_w
    void* out;                   // forward: out; grad_x: grad_x
    float* grad_w;               // grad_w
    float* grad_b;               // grad_w
    // the device's scratch (tetris_lib_agent.h: launch_res): w repacked for the matrix unit [9][NP][KP], or grad_w's partial sums
    const void* packed;
    float* partial;
    int chunks, N, K, NP, KP;    // the product's output channels and reduction length per tap, and both padded to 32
};

TE_HD int res_cout(int Ci, int Co, int join) { return join == RES_JOIN_NONE ? Co : join == RES_JOIN_ADD ? imax(Ci, Co) : imin(Ci, Co); }
TE_HD int res_bands(int Hp) { return (Hp + RES_ROWS - 1) / RES_ROWS; }
TE_HD int res_w_chunks(int M) { return (M + RES_W_SAMPLES - 1) / RES_W_SAMPLES; }
TE_HD int res_pad32(int n) { return (n + 31) / 32 * 32; }
// element (m, h, j, c) of an NHWC array of C channels
TE_HD size_t res_at(const ResArgs& a, size_t m, int h, int j, int c, int C) { return ((m * a.Hp + (size_t)h) * RES_W + (size_t)j) * C + (size_t)c; }
TE_HD size_t res_w_at(const ResArgs& a, int ta, int tb, int ci, int o) { return (((size_t)ta * 3 + (size_t)tb) * a.Ci + (size_t)ci) * a.Co + (size_t)o; }
TE_HD float res_act(float p, int elu) { return elu && !(p > 0.0f) ? expm1f(p) : p; }
// g (y + 1 or 1), rounded to the element type
TE_HD float res_e(float g, float y, int elu, int f16) {
    const float p = elu && y <= 0.0f ? fmaf(g, y, g) : g;          // g (y + 1) with one rounding
    return f16 ? act_f16_to_f32(plan_f32_to_f16(p)) : p;
}
TE_HD float res_e_at(const ResArgs& a, size_t at) {
    return res_e(act_element(a.g, at, a.f16_in), a.elu ? act_element(a.y, at, a.f16_in) : 1.0f, a.elu, a.f16);
}

// ---- serial forms (CPU harness)
// the 12 Cout outputs of row h of sample m
TE_HD void res_forward_row_serial(const ResArgs& a, size_t m, int h) {
    for (int j = 0; j < RES_W; j++) {
        float acc[RES_MAX_C];
        for (int o = 0; o < a.Cz; o++) acc[o] = a.bias[o];
        for (int ta = 0; ta < 3; ta++)
            for (int tb = 0; tb < 3; tb++) {
                const int hh = h + ta - 1, jj = j + tb - 1;
                if (hh < 0 || hh >= a.Hp || jj < 0 || jj >= RES_W) continue;
                for (int ci = 0; ci < a.Ci; ci++) {
                    const float xv = act_element(a.x, res_at(a, m, hh, jj, ci, a.Ci), a.f16_in);
                    const size_t wrow = res_w_at(a, ta, tb, ci, 0);
                    for (int o = 0; o < a.Cz; o++) acc[o] += xv * act_element(a.w, wrow + (size_t)o, a.f16_in);
                }
            }
        for (int c = 0; c < a.Cout; c++) {
            float p = c < a.Cz ? acc[c] : 0.0f;
            if (a.join != RES_JOIN_NONE && c < a.Ci) p += act_element(a.x, res_at(a, m, h, j, c, a.Ci), a.f16_in);
            loss_store(a.out, res_at(a, m, h, j, c, a.Cout), res_act(p, a.elu), a.f16);
        }
    }
}
// the 12 Ci elements of grad_x of row h of sample m
TE_HD void res_grad_x_row_serial(const ResArgs& a, size_t m, int h) {
    for (int j = 0; j < RES_W; j++) {
        float acc[RES_MAX_C];
        for (int ci = 0; ci < a.Ci; ci++) acc[ci] = 0.0f;
        for (int ta = 0; ta < 3; ta++)
            for (int tb = 0; tb < 3; tb++) {
                const int hh = h - ta + 1, jj = j - tb + 1;
                if (hh < 0 || hh >= a.Hp || jj < 0 || jj >= RES_W) continue;
                for (int o = 0; o < a.Cz; o++) {
                    const float ev = res_e_at(a, res_at(a, m, hh, jj, o, a.Cout));
                    for (int ci = 0; ci < a.Ci; ci++) acc[ci] += ev * act_element(a.w, res_w_at(a, ta, tb, ci, o), a.f16_in);
                }
            }
        for (int ci = 0; ci < a.Ci; ci++) {
            float s = acc[ci];
            if (a.join != RES_JOIN_NONE && ci < a.Cout) s += res_e_at(a, res_at(a, m, h, j, ci, a.Cout));
            loss_store(a.out, res_at(a, m, h, j, ci, a.Ci), s, a.f16);
        }
    }
}
// row (a, b, ci) of grad_w: its Co elements
TE_HD void res_grad_w_row_serial(const ResArgs& a, int ta, int tb, int ci) {
    float acc[RES_MAX_C];
    for (int o = 0; o < a.Co; o++) acc[o] = 0.0f;
    for (size_t m = 0; m < (size_t)a.M; m++)
        for (int h = 0; h < a.Hp; h++)
            for (int j = 0; j < RES_W; j++) {
                const int hh = h + ta - 1, jj = j + tb - 1;
                if (hh < 0 || hh >= a.Hp || jj < 0 || jj >= RES_W) continue;
                const float xv = act_element(a.x, res_at(a, m, hh, jj, ci, a.Ci), a.f16_in);
                const size_t at = res_at(a, m, h, j, 0, a.Cout);
                for (int o = 0; o < a.Cz; o++) acc[o] += xv * res_e_at(a, at + (size_t)o);
            }
    const size_t wrow = res_w_at(a, ta, tb, ci, 0);
    for (int o = 0; o < a.Co; o++) a.grad_w[wrow + (size_t)o] = acc[o];
}
TE_HD void res_grad_b_serial(const ResArgs& a) {
    for (int o = 0; o < a.Co; o++) {
        float s = 0.0f;
        if (o < a.Cz)
            for (size_t m = 0; m < (size_t)a.M; m++)
                for (int h = 0; h < a.Hp; h++)
                    for (int j = 0; j < RES_W; j++) s += res_e_at(a, res_at(a, m, h, j, o, a.Cout));
        a.grad_b[o] = s;
    }
}

}  // namespace te
