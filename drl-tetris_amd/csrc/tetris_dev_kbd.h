// Kernels of libtetris_hip.so, part 9: the keyboard convolution on the matrix cores, forward and gradients (definition and serial
// forms: tetris_kbd.h).  Needs tetris_dev_vec.h.
//
// All three products are GEMMs of the matrix unit's 16 x 16 tiles, 32 reduction indices a step: one v_mfma_f32_16x16x32_f16 for
// binary16, eight v_mfma_f32_16x16x4_f32 for float32 (exact f32 at the vector rate), through one set of kernels templated on the
// element type.  A lane's fragment of either operand is the SAME 8 consecutive reduction indices 8 (lane / 16) .. + 7 of row or
// column lane % 16 in both types: the binary16 instruction takes them as they are; float32 instruction i of the eight takes
// element i of each lane, so its four reduction indices are {8 q + i}, the same for both operands — a sum over the reduction
// index does not care which instruction adds which term.  Accumulators: column lane % 16, rows 4 (lane / 16) + register.
// O = 4 K <= 28 output channels are padded to two 16-column tiles, the padding zero.
//
//   k_kbd_pack     w -> the batch's scratch, transposed for the fragment loads and zero-padded to 32 output channels, in the element
//                  type: [Hp][3][32][C] for the forward (8 consecutive c per lane), [Hp][C][3][32] for grad_x (8 consecutive o).
//                  The padding is written there, so no kernel reads w past its end.
//   k_kbd_fwd      a workgroup of 5 waves takes KBD_BLOCK consecutive samples: 10 KBD_BLOCK output rows (m, t) = 5 KBD_BLOCK / 8
//                  tiles, wave v the tiles v, v + 5, ..., both column tiles.  It walks h and, within h, chunks of channels that
//                  fit the stage: x[m][h][.][chunk] goes to LDS in memory order, rows of 12 KBD_BLOCK (sample, column) padded by
//                  16 bytes against bank conflicts, so the A operand of output row (m, t) for kernel column d is the row
//                  12 m + t + d: the three-fold reuse costs no second global read.  Two stages: the next one's global loads are
//                  in flight (in registers) while the matrix unit works on this one; one barrier a stage.  B comes from the
//                  packed w through L2.  The accumulators start at bias.  Samples past M are neither loaded nor stored (their
//                  rows of the tiles hold whatever LDS held: rows of a product do not mix).
//   k_kbd_grad_x   the transposed product, so that a lane's accumulators are consecutive channels: rows c (A = packed w), columns
//                  (m, j), 12 KBD_BLOCK of them, reduction (d, o) = 96.  The B operand is built in LDS from g with the zeros of
//                  the border columns and of the padding written out.  Two row tiles are interleaved — row i of tile u is channel
//                  8 (i / 4) + 4 u + i % 4 — so a lane ends with 8 consecutive channels: one 16-byte store in binary16, two in float32.
//   k_kbd_grad_w   workgroup (chunk of KBD_W_SAMPLES samples, h, block of 128 channels); reduction over (m, j), 96 for a group of 8
//                  samples: A = x transposed on its way into LDS (rows c), B_d[(m, j)][o] = g[m][o][j - d] or 0, built in LDS, one
//                  per kernel column d, so x is staged once for all three.  The 3 x 128 x 32 float32 partial stays in accumulators
//                  over the chunk and goes to the batch's scratch; grad_b's partial is the row sums of B_0, taken by 32 threads of
//                  the workgroups of h = 0.
//   k_kbd_grad_w_reduce   adds the partials in ascending chunk order: no float atomics, a second call gives the same bytes.
typedef float kbd_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 kbd_f16x8 __attribute__((ext_vector_type(8)));

constexpr int KBD_FWD_WAVES = 5, KBD_FWD_THREADS = 64 * KBD_FWD_WAVES;
constexpr int KBD_THREADS = 256;
constexpr int KBD_KX = KBD_D * KBD_OP;           // grad_x's reduction indices (d, o), padded
constexpr int KBD_KW = KBD_W_GROUP * KBD_W;      // grad_w's reduction indices (m, j) of a group
static_assert(KBD_KX % 32 == 0 && KBD_KW % 32 == 0, "whole matrix steps");

template <bool F16> struct KbdType {
    typedef std::conditional_t<F16, uint16_t, uint32_t> T;        // an element's bits
    static constexpr int ES = F16 ? 2 : 4, EPV = 16 / ES, PAD = EPV;       // bytes, elements per 16-byte vector, elements of row padding in LDS
};
// 8 consecutive elements
template <bool F16> struct KbdFrag;
template <> struct KbdFrag<true> { u32x4 v; };
template <> struct KbdFrag<false> { u32x4 lo, hi; };

template <bool F16, class P>
__device__ __forceinline__ KbdFrag<F16> kbd_frag(const P* p) {
    KbdFrag<F16> f;
    if constexpr (F16) f.v = *(const u32x4*)p;
    else { f.lo = *(const u32x4*)p; f.hi = *((const u32x4*)p + 1); }
    return f;
}
template <bool F16>
__device__ __forceinline__ kbd_f32x4 kbd_mma(const KbdFrag<F16>& a, const KbdFrag<F16>& b, kbd_f32x4 c) {
    if constexpr (F16) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(kbd_f16x8, a.v), __builtin_bit_cast(kbd_f16x8, b.v), c, 0, 0, 0);
    } else {
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(u2f(a.lo.x), u2f(b.lo.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(u2f(a.lo.y), u2f(b.lo.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(u2f(a.lo.z), u2f(b.lo.z), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(u2f(a.lo.w), u2f(b.lo.w), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(u2f(a.hi.x), u2f(b.hi.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(u2f(a.hi.y), u2f(b.hi.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(u2f(a.hi.z), u2f(b.hi.z), c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_16x16x4f32(u2f(a.hi.w), u2f(b.hi.w), c, 0, 0, 0);
    }
}
// float32 -> the element's bits, to nearest even
template <bool F16>
__device__ __forceinline__ uint32_t kbd_bits(float v) {
    if constexpr (F16) return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v);
    else return f2u(v);
}
// element (o, t) of sample m of a [M][4][10][K] array, as bits
template <bool F16>
__device__ __forceinline__ typename KbdType<F16>::T kbd_g_bits(const void* g, size_t m, int o, int t, int K) {
    return ((const typename KbdType<F16>::T*)g)[kbd_out_at(m, o, t, K)];
}

// ---- w -> scratch.  FWD: [Hp][3][32][C]; otherwise [Hp][C][3][32].  A thread an element.
template <bool F16, bool FWD>
__global__ __launch_bounds__(KBD_THREADS) void k_kbd_pack(KbdArgs a, void* dst) {
    typedef typename KbdType<F16>::T T;
    const size_t total = (size_t)a.Hp * KBD_D * KBD_OP * a.C, i = (size_t)blockIdx.x * KBD_THREADS + threadIdx.x;
    if (i >= total) return;
    int h, d, c, o;
    if constexpr (FWD) {
        c = (int)(i % a.C); o = (int)((i / a.C) % KBD_OP);
        const int hd = (int)(i / ((size_t)a.C * KBD_OP));
        h = hd / KBD_D; d = hd % KBD_D;
    } else {
        o = (int)(i % KBD_OP); d = (int)((i / KBD_OP) % KBD_D); c = (int)((i / KBD_KX) % a.C); h = (int)(i / ((size_t)KBD_KX * a.C));
    }
    ((T*)dst)[i] = o < a.O ? ((const T*)a.w)[kbd_w_at(a, h, d, c, o)] : (T)0;
}

// ---- forward
// channels per stage: the largest multiple of 32 that divides C and fits
template <bool F16, int S>
__device__ __forceinline__ int kbd_stage_channels(int C) {
    constexpr int MAX = (F16 ? 2048 : 1024) / S;
    int cch = 32;
    for (int k = 64; k <= MAX; k += 32)
        if (C % k == 0) cch = k;
    return cch;
}
template <bool F16, int S>
__global__ __launch_bounds__(KBD_FWD_THREADS) void k_kbd_fwd(KbdArgs a) {
    typedef KbdType<F16> TY;
    typedef typename TY::T T;
    constexpr int ES = TY::ES, EPV = TY::EPV, PAD = TY::PAD;
    constexpr int MAXC = (F16 ? 2048 : 1024) / S, ROWS = S * KBD_W, STAGE = ROWS * (MAXC + PAD);
    constexpr int VPT = (ROWS * MAXC / EPV + KBD_FWD_THREADS - 1) / KBD_FWD_THREADS, TPW = S / 8;
    __shared__ __attribute__((aligned(16))) T lds[2][STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;
    const int C = a.C, Hp = a.Hp, cch = kbd_stage_channels<F16, S>(C), rs = cch + PAD, vpr = cch / EPV;
    const int m0 = blockIdx.x * S, ns = imin(S, a.M - m0), nvec = ns * KBD_W * vpr;
    const int per_h = C / cch, stages = Hp * per_h;
    const char* xs = (const char*)a.x;
    u32x4 regs[VPT];

    auto load = [&](int st) {
        const int h = st / per_h, cc = st - h * per_h;
#pragma unroll
        for (int i = 0; i < VPT; i++) {
            const int v = tid + i * KBD_FWD_THREADS;
            if (v < nvec) {
                const int row = v / vpr, cv = v - row * vpr, s = row / KBD_W, j = row - s * KBD_W;
                regs[i] = __builtin_nontemporal_load((const u32x4*)(xs + (kbd_x_at(a, (size_t)(m0 + s), h, j, cc * cch + cv * EPV)) * ES));
            }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < VPT; i++) {
            const int v = tid + i * KBD_FWD_THREADS;
            if (v < nvec) {
                const int row = v / vpr, cv = v - row * vpr;
                *(u32x4*)&lds[buf][row * rs + cv * EPV] = regs[i];
            }
        }
    };

    kbd_f32x4 acc[TPW][2];
    int rowbase[TPW];
#pragma unroll
    for (int tp = 0; tp < TPW; tp++) {
        const int R = (wave + KBD_FWD_WAVES * tp) * 16 + li, s = R / KBD_T, t = R - s * KBD_T;
        rowbase[tp] = (s * KBD_W + t) * rs;
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            const int o = nt * 16 + li;
            const float bv = o < a.O ? a.bias[o] : 0.0f;
            acc[tp][nt] = kbd_f32x4{bv, bv, bv, bv};
        }
    }

    load(0);
    store(0);
    __syncthreads();
    const T* wp = (const T*)a.packed;
    for (int st = 0; st < stages; st++) {
        if (st + 1 < stages) load(st + 1);
        const int h = st / per_h, cc = st - h * per_h;
        const T* buf = lds[st & 1];
        for (int d = 0; d < KBD_D; d++) {
            const T* wrow = wp + ((size_t)(h * KBD_D + d) * KBD_OP + li) * C + cc * cch + 8 * q;
            for (int c32 = 0; c32 < cch; c32 += 32) {
                const KbdFrag<F16> b0 = kbd_frag<F16>(wrow + c32), b1 = kbd_frag<F16>(wrow + (size_t)16 * C + c32);
#pragma unroll
                for (int tp = 0; tp < TPW; tp++) {
                    const KbdFrag<F16> af = kbd_frag<F16>(buf + rowbase[tp] + d * rs + c32 + 8 * q);
                    acc[tp][0] = kbd_mma<F16>(af, b0, acc[tp][0]);
                    acc[tp][1] = kbd_mma<F16>(af, b1, acc[tp][1]);
                }
            }
        }
        if (st + 1 < stages) store((st + 1) & 1);
        __syncthreads();
    }

#pragma unroll
    for (int tp = 0; tp < TPW; tp++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            const int o = nt * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int R = (wave + KBD_FWD_WAVES * tp) * 16 + 4 * q + r, s = R / KBD_T, t = R - s * KBD_T;
                if (o < a.O && s < ns) {
                    const size_t at = kbd_out_at((size_t)(m0 + s), o, t, a.K);
                    if constexpr (F16) ((uint16_t*)a.out)[at] = (uint16_t)kbd_bits<true>(acc[tp][nt][r]);
                    else ((float*)a.out)[at] = acc[tp][nt][r];
                }
            }
        }
}

// ---- grad_x
template <bool F16, int S>
__global__ __launch_bounds__(KBD_THREADS) void k_kbd_grad_x(KbdArgs a) {
    typedef KbdType<F16> TY;
    typedef typename TY::T T;
    constexpr int PAD = TY::PAD, COLS = S * KBD_W, RS = KBD_KX + PAD, NCT = COLS / 16;
    __shared__ __attribute__((aligned(16))) T gx[COLS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;
    const int C = a.C, m0 = blockIdx.x * S, ns = imin(S, a.M - m0);
    for (int i = tid; i < COLS * KBD_KX; i += KBD_THREADS) {
        const int col = i / KBD_KX, k = i - col * KBD_KX, s = col / KBD_W, j = col - s * KBD_W, d = k / KBD_OP, o = k - d * KBD_OP, t = j - d;
        T v = 0;
        if (s < ns && o < a.O && t >= 0 && t < KBD_T) v = kbd_g_bits<F16>(a.g, (size_t)(m0 + s), o, t, a.K);
        gx[col * RS + k] = v;
    }
    __syncthreads();
    const T* wp = (const T*)a.packed;
    const int per_h = C / 32, pairs = a.Hp * per_h;
    for (int cp = wave; cp < pairs; cp += KBD_THREADS / 64) {
        const int h = cp / per_h, c0 = (cp - h * per_h) * 32;
        KbdFrag<F16> af[2][KBD_KX / 32];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int c = c0 + (li >> 2) * 8 + u * 4 + (li & 3);
#pragma unroll
            for (int ks = 0; ks < KBD_KX / 32; ks++) af[u][ks] = kbd_frag<F16>(wp + ((size_t)h * C + c) * KBD_KX + ks * 32 + 8 * q);
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {
            kbd_f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int ks = 0; ks < KBD_KX / 32; ks++) {
                const KbdFrag<F16> bf = kbd_frag<F16>(gx + (ct * 16 + li) * RS + ks * 32 + 8 * q);
                acc0 = kbd_mma<F16>(af[0][ks], bf, acc0);
                acc1 = kbd_mma<F16>(af[1][ks], bf, acc1);
            }
            const int col = ct * 16 + li, s = col / KBD_W, j = col - s * KBD_W;
            if (s < ns) {
                const size_t at = kbd_x_at(a, (size_t)(m0 + s), h, j, c0 + 8 * q);
                if constexpr (F16) {
                    u32x4 v;
                    v.x = kbd_bits<true>(acc0[0]) | kbd_bits<true>(acc0[1]) << 16; v.y = kbd_bits<true>(acc0[2]) | kbd_bits<true>(acc0[3]) << 16;
                    v.z = kbd_bits<true>(acc1[0]) | kbd_bits<true>(acc1[1]) << 16; v.w = kbd_bits<true>(acc1[2]) | kbd_bits<true>(acc1[3]) << 16;
                    __builtin_nontemporal_store(v, (u32x4*)((uint16_t*)a.out + at));
                } else {
                    const u32x4 v0 = {f2u(acc0[0]), f2u(acc0[1]), f2u(acc0[2]), f2u(acc0[3])}, v1 = {f2u(acc1[0]), f2u(acc1[1]), f2u(acc1[2]), f2u(acc1[3])};
                    __builtin_nontemporal_store(v0, (u32x4*)((float*)a.out + at));
                    __builtin_nontemporal_store(v1, (u32x4*)((float*)a.out + at) + 1);
                }
            }
        }
    }
}

// ---- grad_w: the partial of (chunk, h, channel block) = blockIdx (x, y, z)
template <bool F16>
__global__ __launch_bounds__(KBD_THREADS) void k_kbd_grad_w(KbdArgs a) {
    typedef KbdType<F16> TY;
    typedef typename TY::T T;
    constexpr int ES = TY::ES, EPV = TY::EPV, PAD = TY::PAD, RS = KBD_KW + PAD, CB = KBD_W_CHANNELS, KS = KBD_KW / 32;
    __shared__ __attribute__((aligned(16))) T xt[CB * RS];                       // [c][(s, j)]
    __shared__ __attribute__((aligned(16))) T gt[KBD_D * KBD_OP * RS];           // [d][o][(s, j)]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q = lane >> 4;
    const int C = a.C, chunk = blockIdx.x, h = blockIdx.y, cb0 = blockIdx.z * CB, nch = imin(CB, C - cb0);
    const int m_begin = chunk * KBD_W_SAMPLES, m_end = imin(a.M, m_begin + KBD_W_SAMPLES);
    const bool bias_block = blockIdx.y == 0 && blockIdx.z == 0;
    const char* xs = (const char*)a.x;
    kbd_f32x4 acc[2][KBD_D][2];
#pragma unroll
    for (int ci = 0; ci < 2; ci++)
#pragma unroll
        for (int d = 0; d < KBD_D; d++)
#pragma unroll
            for (int nt = 0; nt < 2; nt++) acc[ci][d][nt] = kbd_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float bsum = 0.0f;

    for (int mg = m_begin; mg < m_end; mg += KBD_W_GROUP) {
        __syncthreads();                 // the last group's fragments are read
        // x[mg .. mg + 8)[h][.][cb0 .. cb0 + nch) -> xt, transposed; zeros for the samples past the end
        if constexpr (F16) {
            const int ncv = nch / EPV;
            for (int i = tid; i < ncv * (KBD_KW / 2); i += KBD_THREADS) {
                const int cv = i / (KBD_KW / 2), kp = i - cv * (KBD_KW / 2), pos = 2 * kp, s = pos / KBD_W, j = pos - s * KBD_W;
                u32x4 va = {0u, 0u, 0u, 0u}, vb = {0u, 0u, 0u, 0u};
                if (mg + s < m_end) {
                    const u32x4* p = (const u32x4*)(xs + kbd_x_at(a, (size_t)(mg + s), h, j, cb0 + cv * EPV) * ES);
                    va = __builtin_nontemporal_load(p);
                    vb = __builtin_nontemporal_load((const u32x4*)((const char*)p + (size_t)C * ES));
                }
                uint32_t* dst = (uint32_t*)xt + (cv * EPV) * (RS / 2) + kp;
                dst[0 * (RS / 2)] = (va.x & 0xFFFFu) | (vb.x << 16);  dst[1 * (RS / 2)] = (va.x >> 16) | (vb.x & 0xFFFF0000u);
                dst[2 * (RS / 2)] = (va.y & 0xFFFFu) | (vb.y << 16);  dst[3 * (RS / 2)] = (va.y >> 16) | (vb.y & 0xFFFF0000u);
                dst[4 * (RS / 2)] = (va.z & 0xFFFFu) | (vb.z << 16);  dst[5 * (RS / 2)] = (va.z >> 16) | (vb.z & 0xFFFF0000u);
                dst[6 * (RS / 2)] = (va.w & 0xFFFFu) | (vb.w << 16);  dst[7 * (RS / 2)] = (va.w >> 16) | (vb.w & 0xFFFF0000u);
            }
        } else {
            const int ncv = nch / EPV;
            for (int i = tid; i < ncv * KBD_KW; i += KBD_THREADS) {
                const int cv = i / KBD_KW, pos = i - cv * KBD_KW, s = pos / KBD_W, j = pos - s * KBD_W;
                u32x4 va = {0u, 0u, 0u, 0u};
                if (mg + s < m_end) va = __builtin_nontemporal_load((const u32x4*)(xs + kbd_x_at(a, (size_t)(mg + s), h, j, cb0 + cv * EPV) * ES));
                T* dst = xt + (cv * EPV) * RS + pos;
                dst[0] = va.x; dst[RS] = va.y; dst[2 * RS] = va.z; dst[3 * RS] = va.w;
            }
        }
        // g -> gt[d][o][(s, j)] = g[mg + s][o][j - d], zeros outside
        for (int i = tid; i < KBD_D * KBD_OP * KBD_KW; i += KBD_THREADS) {
            const int row = i / KBD_KW, pos = i - row * KBD_KW, d = row / KBD_OP, o = row - d * KBD_OP, s = pos / KBD_W, j = pos - s * KBD_W, t = j - d;
            T v = 0;
            if (mg + s < m_end && o < a.O && t >= 0 && t < KBD_T) v = kbd_g_bits<F16>(a.g, (size_t)(mg + s), o, t, a.K);
            gt[row * RS + pos] = v;
        }
        __syncthreads();
        if (bias_block && tid < KBD_OP) {
            for (int pos = 0; pos < KBD_KW; pos++) {
                const T v = gt[tid * RS + pos];
                if constexpr (F16) bsum += vec_f16_to_f32(v); else bsum += u2f(v);
            }
        }
#pragma unroll
        for (int ci = 0; ci < 2; ci++) {
            const int ct = wave + ci * (KBD_THREADS / 64);
            if (ct * 16 < nch) {
#pragma unroll
                for (int ks = 0; ks < KS; ks++) {
                    const KbdFrag<F16> af = kbd_frag<F16>(xt + (ct * 16 + li) * RS + ks * 32 + 8 * q);
#pragma unroll
                    for (int d = 0; d < KBD_D; d++)
#pragma unroll
                        for (int nt = 0; nt < 2; nt++) {
                            const KbdFrag<F16> bf = kbd_frag<F16>(gt + ((d * KBD_OP + nt * 16 + li) * RS + ks * 32 + 8 * q));
                            acc[ci][d][nt] = kbd_mma<F16>(af, bf, acc[ci][d][nt]);
                        }
                }
            }
        }
    }

    float* part = a.partial + (size_t)chunk * ((size_t)a.Hp * KBD_D * C * KBD_OP);
#pragma unroll
    for (int ci = 0; ci < 2; ci++) {
        const int ct = wave + ci * (KBD_THREADS / 64);
        if (ct * 16 < nch) {
#pragma unroll
            for (int d = 0; d < KBD_D; d++)
#pragma unroll
                for (int nt = 0; nt < 2; nt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int c = cb0 + ct * 16 + 4 * q + r;
                        part[(((size_t)h * KBD_D + d) * C + c) * KBD_OP + nt * 16 + li] = acc[ci][d][nt][r];
                    }
        }
    }
    if (bias_block && tid < KBD_OP) a.partial[(size_t)a.chunks * ((size_t)a.Hp * KBD_D * C * KBD_OP) + (size_t)chunk * KBD_OP + tid] = bsum;
}

// the partials in ascending chunk order -> grad_w and grad_b.  A thread a (row, padded column); the last 32 are the bias
__global__ __launch_bounds__(KBD_THREADS) void k_kbd_grad_w_reduce(KbdArgs a) {
    const size_t per = (size_t)a.Hp * KBD_D * a.C * KBD_OP, i = (size_t)blockIdx.x * KBD_THREADS + threadIdx.x;
    if (i >= per + KBD_OP) return;
    float s = 0.0f;
    if (i < per) {
        for (int ch = 0; ch < a.chunks; ch++) s += a.partial[(size_t)ch * per + i];
        const int o = (int)(i % KBD_OP);
        if (o < a.O) a.grad_w[(i / KBD_OP) * a.O + o] = s;
    } else {
        const int o = (int)(i - per);
        for (int ch = 0; ch < a.chunks; ch++) s += a.partial[(size_t)a.chunks * per + (size_t)ch * KBD_OP + o];
        if (o < a.O) a.grad_b[o] = s;
    }
}
