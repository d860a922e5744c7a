// Kernels of libtetris_hip.so, part 10: one residual layer on the matrix cores — 3 x 3 'same' convolution, peephole join, ELU —
// forward and gradients (definition and serial forms: tetris_res.h).  Needs tetris_dev_vec.h and tetris_dev_kbd.h, whose fragment
// convention it keeps: a lane's fragment of either operand is 8 consecutive reduction indices 8 (lane / 16) .. + 7 of row or
// column lane % 16, for binary16 (one v_mfma_f32_16x16x32_f16) and float32 (eight v_mfma_f32_16x16x4_f32) alike, so float32
// shares every load and layout with binary16.
//
//   k_res_pack     w -> the batch's scratch, [9][NP][KP] in the element type, the reduction index contiguous, both padded to 32
//                  with zeros written out: the forward's [tap][o][ci], and for grad_x the kernel rotated by 180 degrees with ci
//                  and o exchanged, [8 - tap][ci][o] — a 'same' convolution's input gradient is a 'same' convolution of gz with
//                  that kernel, so one product kernel serves both.
//   k_res_conv     a workgroup of 4 waves takes a band of RES_ROWS image rows of one sample — 96 positions, six 16-column tiles
//                  — and 128 output channels.  The reduction runs over chunks of 32 input channels: the band's rows with their
//                  halo, [RES_ROWS + 2][14][32], go to LDS with the border zeros (and the zeros of a channel tail, and of the
//                  rows past the image) written out, so the fragment of position (h, j) for tap (a, b) is the 16-byte read at
//                  [h + a][j + b][8 q ..] with no mask.  Two stages: the next chunk's global loads are in flight (in registers)
//                  while the matrix unit works on this one; one barrier a stage.  grad_x forms e from g and y on the way in.
//                  The product is taken transposed — rows output channels (A = packed w through L2), columns positions — and
//                  two row tiles are interleaved as in k_kbd_grad_x, so a lane ends with 8 consecutive channels of one
//                  position: bias in the accumulators' initial value, the join's x (or e) added from global memory, ELU, one
//                  rounding, one 16-byte store in binary16, two in float32.  Wave (wm, wn) takes position tiles 3 wm .. + 2
//                  and channels 64 wn .. + 63.  The pass-through channels Co..Ci of ADD are copied and activated by the
//                  workgroups of the first channel block.
//   k_res_grad_w   workgroup (chunk of RES_W_SAMPLES samples, block of 32 input channels, block of 32 output channels), all
//                  nine taps.  The reduction runs over positions, a band of RES_ROWS rows of a sample a pass, each image row
//                  padded to 16 columns so that a fragment is 8 columns of one row: both operands are transposed on their way
//                  into LDS, x once with a halo row above and below (a tap's row offset is then an aligned offset), gz three
//                  times, shifted by a tap's column offset, the slots no shift reaches staying zero.  Wave (ci tile, o tile)
//                  keeps the nine taps' partials in accumulators over the chunk and writes them to the batch's scratch;
//                  grad_b's partial is the row sums of the unshifted gz, taken by the workgroups of the first input block.
//   k_res_grad_w_reduce   adds the partials in ascending chunk order: no float atomics, a second call gives the same bytes.
constexpr int RES_THREADS = 256;
constexpr int RES_NB = 128;                                        // output channels per workgroup of k_res_conv
constexpr int RES_SROWS = RES_ROWS + 2, RES_SCOLS = RES_W + 2;     // a stage: the band with its halo
constexpr int RES_TILES = RES_ROWS * RES_W / 16;                   // position tiles of a band
static_assert(RES_ROWS * RES_W % 32 == 0 && RES_TILES % 2 == 0 && RES_ROWS % 2 == 0, "whole tiles, half of them a wave row; two image rows a matrix step");

// v[0..8) += the 8 elements of a fragment as float32
template <bool F16>
__device__ __forceinline__ void res_add_frag(const KbdFrag<F16>& f, float v[8]) {
    if constexpr (F16) {
        v[0] += vec_f16_to_f32((uint16_t)(f.v.x & 0xFFFFu)); v[1] += vec_f16_to_f32((uint16_t)(f.v.x >> 16));
        v[2] += vec_f16_to_f32((uint16_t)(f.v.y & 0xFFFFu)); v[3] += vec_f16_to_f32((uint16_t)(f.v.y >> 16));
        v[4] += vec_f16_to_f32((uint16_t)(f.v.z & 0xFFFFu)); v[5] += vec_f16_to_f32((uint16_t)(f.v.z >> 16));
        v[6] += vec_f16_to_f32((uint16_t)(f.v.w & 0xFFFFu)); v[7] += vec_f16_to_f32((uint16_t)(f.v.w >> 16));
    } else {
        v[0] += u2f(f.lo.x); v[1] += u2f(f.lo.y); v[2] += u2f(f.lo.z); v[3] += u2f(f.lo.w);
        v[4] += u2f(f.hi.x); v[5] += u2f(f.hi.y); v[6] += u2f(f.hi.z); v[7] += u2f(f.hi.w);
    }
}
template <bool F16, class P>
__device__ __forceinline__ void res_add8(const P* p, float v[8]) { res_add_frag<F16>(kbd_frag<F16>(p), v); }
// v[0..8), rounded once -> 8 consecutive elements at p
template <bool F16, class P>
__device__ __forceinline__ void res_store8(P* p, const float v[8]) {
    if constexpr (F16) {
        u32x4 o;
        o.x = kbd_bits<true>(v[0]) | kbd_bits<true>(v[1]) << 16; o.y = kbd_bits<true>(v[2]) | kbd_bits<true>(v[3]) << 16;
        o.z = kbd_bits<true>(v[4]) | kbd_bits<true>(v[5]) << 16; o.w = kbd_bits<true>(v[6]) | kbd_bits<true>(v[7]) << 16;
        __builtin_nontemporal_store(o, (u32x4*)p);
    } else {
        const u32x4 o0 = {f2u(v[0]), f2u(v[1]), f2u(v[2]), f2u(v[3])}, o1 = {f2u(v[4]), f2u(v[5]), f2u(v[6]), f2u(v[7])};
        __builtin_nontemporal_store(o0, (u32x4*)p);
        __builtin_nontemporal_store(o1, (u32x4*)p + 1);
    }
}
// e of one element in float32: g (y + 1) with one rounding
__device__ __forceinline__ float res_e_f32(float g, float y) { return y <= 0.0f ? __builtin_fmaf(g, y, g) : g; }
__device__ __forceinline__ uint32_t res_e_pair(uint32_t g, uint32_t y) {
    const float lo = res_e_f32(vec_f16_to_f32((uint16_t)(g & 0xFFFFu)), vec_f16_to_f32((uint16_t)(y & 0xFFFFu)));
    const float hi = res_e_f32(vec_f16_to_f32((uint16_t)(g >> 16)), vec_f16_to_f32((uint16_t)(y >> 16)));
    return kbd_bits<true>(lo) | kbd_bits<true>(hi) << 16;
}
// the 16-byte vector of e at element `at` of g (and y): g itself without ELU
template <bool F16>
__device__ __forceinline__ u32x4 res_e_vec(const ResArgs& a, size_t at) {
    typedef typename KbdType<F16>::T T;
    const u32x4 g = *(const u32x4*)((const T*)a.g + at);
    if (!a.elu) return g;
    const u32x4 y = *(const u32x4*)((const T*)a.y + at);
    u32x4 r;
    if constexpr (F16) {
        r.x = res_e_pair(g.x, y.x); r.y = res_e_pair(g.y, y.y); r.z = res_e_pair(g.z, y.z); r.w = res_e_pair(g.w, y.w);
    } else {
        r.x = f2u(res_e_f32(u2f(g.x), u2f(y.x))); r.y = f2u(res_e_f32(u2f(g.y), u2f(y.y)));
        r.z = f2u(res_e_f32(u2f(g.z), u2f(y.z))); r.w = f2u(res_e_f32(u2f(g.w), u2f(y.w)));
    }
    return r;
}

// ---- w -> scratch [9][NP][KP].  A thread an element.
template <bool F16, bool FWD>
__global__ __launch_bounds__(RES_THREADS) void k_res_pack(ResArgs a, void* dst) {
    typedef typename KbdType<F16>::T T;
    const size_t total = (size_t)RES_TAPS * a.NP * a.KP, i = (size_t)blockIdx.x * RES_THREADS + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % a.KP), n = (int)((i / a.KP) % a.NP), t = (int)(i / ((size_t)a.KP * a.NP));
    T v = 0;
    if (n < a.N && k < a.K) {
        if constexpr (FWD) v = ((const T*)a.w)[res_w_at(a, t / 3, t % 3, k, n)];
        else v = ((const T*)a.w)[res_w_at(a, 2 - t / 3, 2 - t % 3, n, k)];
    }
    ((T*)dst)[i] = v;
}

// ---- the product of the forward and of grad_x: blockIdx.x = (sample, band), blockIdx.y = block of RES_NB output channels
template <bool F16, bool FWD>
__global__ __launch_bounds__(RES_THREADS) void k_res_conv(ResArgs a) {
    typedef KbdType<F16> TY;
    typedef typename TY::T T;
    constexpr int EPV = TY::EPV, RS = 32 + TY::PAD, VPR = 32 / EPV;
    constexpr int NV = RES_SROWS * RES_SCOLS * VPR, VPT = (NV + RES_THREADS - 1) / RES_THREADS, MT = RES_TILES / 2;
    __shared__ __attribute__((aligned(16))) T lds[2][RES_SROWS * RES_SCOLS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4, wm = wave & 1, wn = wave >> 1;
    const int bands = res_bands(a.Hp), band = (int)(blockIdx.x % (unsigned)bands), h0 = band * RES_ROWS, nb0 = blockIdx.y * RES_NB;
    const size_t m = blockIdx.x / (unsigned)bands;
    const int CS = FWD ? a.Ci : a.Cout;            // channels of the array that is staged
    const int stages = a.KP / 32;
    u32x4 regs[VPT];

    auto load = [&](int st) {
#pragma unroll
        for (int i = 0; i < VPT; i++) {
            const int v = tid + i * RES_THREADS;
            if (v < NV) {
                const int cv = v % VPR, sp = v / VPR, sc = sp % RES_SCOLS, sr = sp / RES_SCOLS;
                const int h = h0 + sr - 1, j = sc - 1, c = st * 32 + cv * EPV;
                u32x4 val = {0u, 0u, 0u, 0u};
                if (h >= 0 && h < a.Hp && j >= 0 && j < RES_W && c < a.K) {
                    const size_t at = res_at(a, m, h, j, c, CS);
                    if constexpr (FWD) val = *(const u32x4*)((const T*)a.x + at);
                    else val = res_e_vec<F16>(a, at);
                }
                regs[i] = val;
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < VPT; i++) {
            const int v = tid + i * RES_THREADS;
            if (v < NV) *(u32x4*)&lds[buf][(v / VPR) * RS + (v % VPR) * EPV] = regs[i];
        }
    };

    // this wave's two pairs of channel tiles (32 channels a pair) and three position tiles
    bool pv[2];
    int cbase[2], posbase[MT];
    kbd_f32x4 acc[MT][2][2];
#pragma unroll
    for (int pi = 0; pi < 2; pi++) {
        cbase[pi] = nb0 + (2 * wn + pi) * 32;
        pv[pi] = cbase[pi] < a.NP;
    }
#pragma unroll
    for (int t = 0; t < MT; t++) {
        const int p = (MT * wm + t) * 16 + li;
        posbase[t] = ((p / RES_W) * RES_SCOLS + p % RES_W) * RS;
#pragma unroll
        for (int pi = 0; pi < 2; pi++)
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int c = cbase[pi] + 8 * q + 4 * u + r;
                    acc[t][pi][u][r] = FWD && c < a.N ? a.bias[c] : 0.0f;
                }
    }

    load(0);
    store(0);
    __syncthreads();
    const T* wp = (const T*)a.packed;
    for (int st = 0; st < stages; st++) {
        if (st + 1 < stages) load(st + 1);
        const T* buf = lds[st & 1];
        if (pv[0]) {
            for (int tap = 0; tap < RES_TAPS; tap++) {
                const int toff = ((tap / 3) * RES_SCOLS + tap % 3) * RS + 8 * q;
                KbdFrag<F16> wf[2][2];
#pragma unroll
                for (int pi = 0; pi < 2; pi++)
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        const int c = (pv[pi] ? cbase[pi] : cbase[0]) + (li >> 2) * 8 + u * 4 + (li & 3);
                        wf[pi][u] = kbd_frag<F16>(wp + ((size_t)tap * a.NP + c) * a.KP + st * 32 + 8 * q);
                    }
#pragma unroll
                for (int t = 0; t < MT; t++) {
                    const KbdFrag<F16> xf = kbd_frag<F16>(buf + posbase[t] + toff);
                    acc[t][0][0] = kbd_mma<F16>(wf[0][0], xf, acc[t][0][0]);
                    acc[t][0][1] = kbd_mma<F16>(wf[0][1], xf, acc[t][0][1]);
                    if (pv[1]) {
                        acc[t][1][0] = kbd_mma<F16>(wf[1][0], xf, acc[t][1][0]);
                        acc[t][1][1] = kbd_mma<F16>(wf[1][1], xf, acc[t][1][1]);
                    }
                }
            }
        }
        if (st + 1 < stages) store((st + 1) & 1);
        __syncthreads();
    }

#pragma unroll
    for (int t = 0; t < MT; t++) {
        const int p = (MT * wm + t) * 16 + li, h = h0 + p / RES_W, j = p % RES_W;
#pragma unroll
        for (int pi = 0; pi < 2; pi++) {
            const int cg = cbase[pi] + 8 * q;
            if (h < a.Hp && cg < a.N) {
                float v[8];
#pragma unroll
                for (int r = 0; r < 4; r++) { v[r] = acc[t][pi][0][r]; v[4 + r] = acc[t][pi][1][r]; }
                if constexpr (FWD) {
                    if (a.join != RES_JOIN_NONE && cg < a.Ci) res_add8<F16>((const T*)a.x + res_at(a, m, h, j, cg, a.Ci), v);
                    if (a.elu) {
#pragma unroll
                        for (int r = 0; r < 8; r++) v[r] = res_act(v[r], 1);
                    }
                    res_store8<F16>((T*)a.out + res_at(a, m, h, j, cg, a.Cout), v);
                } else {
                    if (a.join != RES_JOIN_NONE && cg < a.Cout) {
                        KbdFrag<F16> e;
                        if constexpr (F16) e.v = res_e_vec<F16>(a, res_at(a, m, h, j, cg, a.Cout));
                        else { e.lo = res_e_vec<F16>(a, res_at(a, m, h, j, cg, a.Cout)); e.hi = res_e_vec<F16>(a, res_at(a, m, h, j, cg + 4, a.Cout)); }
                        res_add_frag<F16>(e, v);
                    }
                    res_store8<F16>((T*)a.out + res_at(a, m, h, j, cg, a.Ci), v);
                }
            }
        }
    }
    // ADD with Ci > Co: channels Co..Ci are x, activated
    if constexpr (FWD) {
        if (blockIdx.y == 0 && a.Cout > a.Co) {
            const int nvec = (a.Cout - a.Co) / 8;
            for (int i = tid; i < RES_ROWS * RES_W * nvec; i += RES_THREADS) {
                const int p = i / nvec, c = a.Co + (i - p * nvec) * 8, h = h0 + p / RES_W, j = p % RES_W;
                if (h >= a.Hp) continue;
                float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                res_add8<F16>((const T*)a.x + res_at(a, m, h, j, c, a.Ci), v);
                if (a.elu) {
#pragma unroll
                    for (int r = 0; r < 8; r++) v[r] = res_act(v[r], 1);
                }
                res_store8<F16>((T*)a.out + res_at(a, m, h, j, c, a.Cout), v);
            }
        }
    }
}

// ---- grad_w: the partial of (chunk, input block, output block) = blockIdx (x, y, z)
template <bool F16>
__global__ __launch_bounds__(RES_THREADS) void k_res_grad_w(ResArgs a) {
    typedef KbdType<F16> TY;
    typedef typename TY::T T;
    constexpr int EPV = TY::EPV, CB = RES_W_CHANNELS, NCV = CB / EPV;
    constexpr int XR = RES_SROWS * 16 + TY::PAD, GR = RES_ROWS * 16 + TY::PAD, KS = RES_ROWS / 2;
    __shared__ __attribute__((aligned(16))) T xt[CB * XR];                    // [ci][row with halo][16]
    __shared__ __attribute__((aligned(16))) T gt[3 * CB * GR];                // [b][o][row][16]: gz[row][column - b + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4, cit = wave & 1, ot = wave >> 1;
    const int chunk = blockIdx.x, ci0 = blockIdx.y * CB, o0 = blockIdx.z * CB, nci = imin(CB, a.Ci - ci0), bands = res_bands(a.Hp);
    const size_t m_begin = (size_t)chunk * RES_W_SAMPLES, m_end = m_begin + (size_t)imin(RES_W_SAMPLES, a.M - chunk * RES_W_SAMPLES);
    const bool bias_block = blockIdx.y == 0;
    kbd_f32x4 acc[3][3];
#pragma unroll
    for (int ta = 0; ta < 3; ta++)
#pragma unroll
        for (int tb = 0; tb < 3; tb++) acc[ta][tb] = kbd_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float bsum = 0.0f;
    // the padding columns and the slots that no column shift reaches stay zero
    for (int i = tid; i < CB * XR; i += RES_THREADS) xt[i] = 0;
    for (int i = tid; i < 3 * CB * GR; i += RES_THREADS) gt[i] = 0;

    for (size_t m = m_begin; m < m_end; m++)
        for (int band = 0; band < bands; band++) {
            const int h0 = band * RES_ROWS;
            __syncthreads();                 // the last pass's fragments are read (first pass: the zeros are written)
            for (int i = tid; i < RES_SROWS * RES_W * NCV; i += RES_THREADS) {
                const int cv = i % NCV, sp = i / NCV, j = sp % RES_W, sr = sp / RES_W, h = h0 + sr - 1, c = cv * EPV;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (h >= 0 && h < a.Hp && c < nci) v = __builtin_nontemporal_load((const u32x4*)((const T*)a.x + res_at(a, m, h, j, ci0 + c, a.Ci)));
                T* dst = xt + c * XR + sr * 16 + j;
                if constexpr (F16) {
                    dst[0] = (T)(v.x & 0xFFFFu); dst[XR] = (T)(v.x >> 16); dst[2 * XR] = (T)(v.y & 0xFFFFu); dst[3 * XR] = (T)(v.y >> 16);
                    dst[4 * XR] = (T)(v.z & 0xFFFFu); dst[5 * XR] = (T)(v.z >> 16); dst[6 * XR] = (T)(v.w & 0xFFFFu); dst[7 * XR] = (T)(v.w >> 16);
                } else {
                    dst[0] = v.x; dst[XR] = v.y; dst[2 * XR] = v.z; dst[3 * XR] = v.w;
                }
            }
            for (int i = tid; i < RES_ROWS * RES_W * NCV; i += RES_THREADS) {
                const int cv = i % NCV, sp = i / NCV, j = sp % RES_W, hl = sp / RES_W, h = h0 + hl, c = cv * EPV;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (h < a.Hp && o0 + c < a.Cz) v = res_e_vec<F16>(a, res_at(a, m, h, j, o0 + c, a.Cout));
#pragma unroll
                for (int tb = 0; tb < 3; tb++) {
                    const int jp = j + tb - 1;
                    if (jp < 0) continue;
                    T* dst = gt + (tb * CB + c) * GR + hl * 16 + jp;
                    if constexpr (F16) {
                        dst[0] = (T)(v.x & 0xFFFFu); dst[GR] = (T)(v.x >> 16); dst[2 * GR] = (T)(v.y & 0xFFFFu); dst[3 * GR] = (T)(v.y >> 16);
                        dst[4 * GR] = (T)(v.z & 0xFFFFu); dst[5 * GR] = (T)(v.z >> 16); dst[6 * GR] = (T)(v.w & 0xFFFFu); dst[7 * GR] = (T)(v.w >> 16);
                    } else {
                        dst[0] = v.x; dst[GR] = v.y; dst[2 * GR] = v.z; dst[3 * GR] = v.w;
                    }
                }
            }
            __syncthreads();
            if (bias_block && tid < CB) {
                for (int pos = 0; pos < RES_ROWS * 16; pos++) {
                    const T v = gt[(CB + tid) * GR + pos];
                    if constexpr (F16) bsum += vec_f16_to_f32(v); else bsum += u2f(v);
                }
            }
            if (cit * 16 < nci) {
#pragma unroll
                for (int ks = 0; ks < KS; ks++) {
                    const int off = (2 * ks + (q >> 1)) * 16 + 8 * (q & 1);
                    KbdFrag<F16> gf[3];
#pragma unroll
                    for (int tb = 0; tb < 3; tb++) gf[tb] = kbd_frag<F16>(gt + (tb * CB + ot * 16 + li) * GR + off);
#pragma unroll
                    for (int ta = 0; ta < 3; ta++) {
                        const KbdFrag<F16> xf = kbd_frag<F16>(xt + (cit * 16 + li) * XR + ta * 16 + off);
#pragma unroll
                        for (int tb = 0; tb < 3; tb++) acc[ta][tb] = kbd_mma<F16>(xf, gf[tb], acc[ta][tb]);
                    }
                }
            }
        }

    const size_t per = (size_t)RES_TAPS * a.Ci * a.Co;
    float* part = a.partial + (size_t)chunk * per;
#pragma unroll
    for (int ta = 0; ta < 3; ta++)
#pragma unroll
        for (int tb = 0; tb < 3; tb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int ci = ci0 + cit * 16 + 4 * q + r;
                if (ci < a.Ci) part[((size_t)(ta * 3 + tb) * a.Ci + ci) * a.Co + o0 + ot * 16 + li] = acc[ta][tb][r];
            }
    if (bias_block && tid < CB) a.partial[(size_t)a.chunks * per + (size_t)chunk * a.Co + o0 + tid] = bsum;
}

// the partials in ascending chunk order -> grad_w and grad_b.  A thread an element; the last Co are the bias
__global__ __launch_bounds__(RES_THREADS) void k_res_grad_w_reduce(ResArgs a) {
    const size_t per = (size_t)RES_TAPS * a.Ci * a.Co, i = (size_t)blockIdx.x * RES_THREADS + threadIdx.x;
    if (i >= per + (size_t)a.Co) return;
    float s = 0.0f;
    if (i < per) {
        for (int ch = 0; ch < a.chunks; ch++) s += a.partial[(size_t)ch * per + i];
        a.grad_w[i] = s;
    } else {
        const size_t o = i - per;
        for (int ch = 0; ch < a.chunks; ch++) s += a.partial[(size_t)a.chunks * per + (size_t)ch * a.Co + o];
        a.grad_b[o] = s;
    }
}
