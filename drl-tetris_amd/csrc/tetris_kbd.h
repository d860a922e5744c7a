// Kernel bodies of the keyboard convolution (include/tetris_hip.h: tetris_kbd_conv_dev, tetris_kbd_conv_grad_x_dev,
// tetris_kbd_conv_grad_w_dev): the last learned layer of the reference's resblock_kbd (agents/networks/builders/
// sventon_architectures.py:71-73), keyboard_conv (agents/networks/builders/build_blocks.py:68-83) — a "valid" convolution whose
// kernel is as tall as the image and three columns wide (build_blocks.py:69-78), then n_rot = 4 channel slices concatenated along
// the rotation axis (build_blocks.py:79-80) — with its backward.  kbd_activation (build_blocks.py:81-82) stays with
// tetris_q_head_dev / tetris_policy_head_dev.
//
// `__host__ __device__` like tetris_head.h: the serial forms below are what the CPU harness (tests/cpu_harness) runs through
// kbd_run_serial (tetris_host.h); tetris_hip.hip computes the same sums on the matrix cores of gfx950 (tetris_dev_kbd.h) in an
// order of its own.
//
// SHAPES.  T = 10 translations, K = n_pieces in 1..7, O = 4 K output channels, o = r K + k; Hp in 4..33 image rows, 12 image
// columns, C a multiple of 32 in 32..512 channels.
//   x     [M][Hp][12][C]   NHWC, contiguous: the memory of a torch channels_last tensor of shape [M, C, Hp, 12]
//   w     [Hp][3][C][O]    HWIO, the reference variable's own layout
//   bias  [O]              float32
//   out   [M][4][10][K]    what tetris_q_head_dev, tetris_policy_head_dev, tetris_select_eval_dev and the loss heads take
//   g     [M][4][10][K]    the gradient with respect to out
// x, w, out, g and grad_x are float32, or all binary16 with the F16 flag; bias, grad_w and grad_b are always float32.
//
// FORWARD.   out[m][r][t][k] = bias[o] + sum_h sum_d sum_c x[m][h][t + d][c] w[h][d][c][o],  d in 0..2.
//   The slices and the concat of build_blocks.py:79-80 are the index map o -> (r, k) = (o / K, o % K) and nothing else.
// GRADIENTS of sum g out:
//   grad_x[m][h][j][c] = sum over d with 0 <= j - d <= 9, sum_o g[m][r][j - d][k] w[h][d][c][o]
//   grad_w[h][d][c][o] = sum_m sum_t x[m][h][t + d][c] g[m][r][t][k]
//   grad_b[o]          = sum_m sum_t g[m][r][t][k]
// ARITHMETIC.  A binary16 input is widened exactly; every product is formed and every sum accumulated in float32, and the result is
// rounded once, to nearest even, to the element type of its array.  The serial form sums from +0 in ascending (h, d, c) — the
// forward starts from bias[o] —, (d, o) and (m, t); the order of the device's sums is the matrix unit's and is not specified.
// No atomics on either side: the same call twice gives the same bits.
//
// OUTPUTS.  Every element of every output is written, nothing past it; nothing behind the end of x, w, bias or g is read.
#pragma once
#include "tetris_act.h"
#include "tetris_loss.h"

namespace te {

constexpr int KBD_FWD = 0, KBD_GRAD_X = 1, KBD_GRAD_W = 2;
constexpr int KBD_T = 10, KBD_W = 12, KBD_D = 3, KBD_ROT = 4;      // translations, image columns, kernel columns, rotations
constexpr int KBD_OP = 32;                                          // O padded to the matrix unit's tiles
#ifndef TETRIS_KBD_BLOCK
#define TETRIS_KBD_BLOCK 16
#endif
constexpr int KBD_BLOCK = TETRIS_KBD_BLOCK;      // samples per workgroup of the forward and grad_x kernels (a multiple of 8; DESIGN.md §4 has the measurement)
constexpr int KBD_W_GROUP = 8;                   // samples of one pass of the grad_w kernel: 96 image columns = three 32-deep matrix steps
constexpr int KBD_W_SAMPLES = 256;               // samples per partial sum of grad_w (a multiple of KBD_W_GROUP)
constexpr int KBD_W_CHANNELS = 128;              // channels per workgroup of the grad_w kernel
static_assert(KBD_BLOCK % 8 == 0 && KBD_BLOCK >= 8 && KBD_BLOCK <= 32, "10 and 12 rows per sample fill whole 16-row tiles");

struct KbdArgs {
    int op;                      // KBD_FWD / KBD_GRAD_X / KBD_GRAD_W
    int M, K, O, Hp, C, f16;
    const void* x;               // forward, grad_w
    const void* w;               // forward, grad_x
    const float* bias;           // forward
    const void* g;               // grad_x, grad_w
    void* out;                   // forward: out; grad_x: grad_x
    float* grad_w;               // grad_w
    float* grad_b;               // grad_w
    // the device's scratch (tetris_lib_agent.h: launch_kbd): w repacked for the matrix unit, or grad_w's partial sums
    const void* packed;
    float* partial;
    int chunks;
};

TE_HD int kbd_blocks(int M) { return (M + KBD_BLOCK - 1) / KBD_BLOCK; }
TE_HD int kbd_w_chunks(int M) { return (M + KBD_W_SAMPLES - 1) / KBD_W_SAMPLES; }
// element (r, t, k) of a sample's [4][10][K] image from the output channel o = r K + k
TE_HD size_t kbd_out_at(size_t m, int o, int t, int K) { return ((m * KBD_ROT + (size_t)(o / K)) * KBD_T + (size_t)t) * K + (size_t)(o % K); }
TE_HD size_t kbd_x_at(const KbdArgs& a, size_t m, int h, int j, int c) { return ((m * a.Hp + (size_t)h) * KBD_W + (size_t)j) * a.C + (size_t)c; }
TE_HD size_t kbd_w_at(const KbdArgs& a, int h, int d, int c, int o) { return (((size_t)h * KBD_D + (size_t)d) * a.C + (size_t)c) * a.O + (size_t)o; }

// ---- serial forms (CPU harness)
// the 10 O outputs of sample m
TE_HD void kbd_forward_sample_serial(const KbdArgs& a, size_t m) {
    for (int t = 0; t < KBD_T; t++) {
        float acc[KBD_OP];
        for (int o = 0; o < a.O; o++) acc[o] = a.bias[o];
        for (int h = 0; h < a.Hp; h++)
            for (int d = 0; d < KBD_D; d++)
                for (int c = 0; c < a.C; c++) {
                    const float xv = act_element(a.x, kbd_x_at(a, m, h, t + d, c), a.f16);
                    const size_t wrow = kbd_w_at(a, h, d, c, 0);
                    for (int o = 0; o < a.O; o++) acc[o] += xv * act_element(a.w, wrow + (size_t)o, a.f16);
                }
        for (int o = 0; o < a.O; o++) loss_store(a.out, kbd_out_at(m, o, t, a.K), acc[o], a.f16);
    }
}
// the Hp 12 C elements of grad_x of sample m
TE_HD void kbd_grad_x_sample_serial(const KbdArgs& a, size_t m) {
    for (int h = 0; h < a.Hp; h++)
        for (int j = 0; j < KBD_W; j++)
            for (int c = 0; c < a.C; c++) {
                float s = 0.0f;
                for (int d = 0; d < KBD_D; d++) {
                    const int t = j - d;
                    if (t < 0 || t >= KBD_T) continue;
                    const size_t wrow = kbd_w_at(a, h, d, c, 0);
                    for (int o = 0; o < a.O; o++) s += act_element(a.g, kbd_out_at(m, o, t, a.K), a.f16) * act_element(a.w, wrow + (size_t)o, a.f16);
                }
                loss_store(a.out, kbd_x_at(a, m, h, j, c), s, a.f16);
            }
}
// row (h, d, c) of grad_w: its O elements
TE_HD void kbd_grad_w_row_serial(const KbdArgs& a, int h, int d, int c) {
    float acc[KBD_OP];
    for (int o = 0; o < a.O; o++) acc[o] = 0.0f;
    for (size_t m = 0; m < (size_t)a.M; m++)
        for (int t = 0; t < KBD_T; t++) {
            const float xv = act_element(a.x, kbd_x_at(a, m, h, t + d, c), a.f16);
            for (int o = 0; o < a.O; o++) acc[o] += xv * act_element(a.g, kbd_out_at(m, o, t, a.K), a.f16);
        }
    const size_t wrow = kbd_w_at(a, h, d, c, 0);
    for (int o = 0; o < a.O; o++) a.grad_w[wrow + (size_t)o] = acc[o];
}
TE_HD void kbd_grad_b_serial(const KbdArgs& a) {
    for (int o = 0; o < a.O; o++) {
        float s = 0.0f;
        for (size_t m = 0; m < (size_t)a.M; m++)
            for (int t = 0; t < KBD_T; t++) s += act_element(a.g, kbd_out_at(m, o, t, a.K), a.f16);
        a.grad_b[o] = s;
    }
}

}  // namespace te
