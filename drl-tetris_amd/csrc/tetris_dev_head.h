// Kernels of libtetris_hip.so, part 8: the network's output heads, Q / V / A and policy, with gradients (bodies: tetris_head.h).
// Needs tetris_dev_vec.h.

// ---- the output heads (tetris_head.h).  One launch per call.  A workgroup takes HEAD_BLOCK = 16 consecutive samples — 16 x 40 K
// contiguous elements, a multiple of 16 bytes for every K and element type — and keeps them in LDS as float32 in memory order
// (the image: element e of the block at word e), so streaming in and out is a linear walk of 16-byte vectors, one vector per lane
// and trip.  The work then alternates between two shapes, a barrier between them:
//   elements: every lane takes the 4 (binary16: 8) elements of one vector — a - sub, tanhf, expf, the division, the gradient
//     terms — and, in the last such pass, packs and stores the output vector;
//   planes: thread (sample, piece), 112 of the 256 at K = 7, walks its 40 elements of the image with stride K in ascending j —
//     sum, maximum, minimum and tie counts, or a dot product — and thread `sample` combines a sample's K plane results.
// The orders of tetris_head.h are kept whoever does the work.  LDS: 17.5 KB per image (the backward kernels hold two), 5 KB of
// plane results.  No atomics, no workgroup waits for another.
struct HeadImage {
    alignas(16) float x[HEAD_BLOCK * HEAD_PER];
    float red[HEAD_BLOCK][HEAD_PIECES];
};
struct HeadQShared {
    HeadPlane plane[HEAD_BLOCK][HEAD_PIECES];
    HeadQSample q[HEAD_BLOCK];
};
static_assert(HEAD_BLOCK * 7 <= HEAD_THREADS, "a thread per (sample, piece)");
static_assert((HEAD_BLOCK * ACT_CANDIDATES * 2) % 16 == 0, "a block's run starts on 16 bytes for every K and element type");

// the block's run of a big array -> the image, times `scale`
template <bool F16>
__device__ __forceinline__ void head_stream_in(const void* src, int K, int m0, int ng, float scale, float* image) {
    constexpr int EPV = F16 ? 8 : 4;
    const int per = ACT_CANDIDATES * K, nvec = ng * per / EPV;
    const u32x4* run = (const u32x4*)((const char*)src + (size_t)m0 * per * (F16 ? 2 : 4));
#pragma unroll 2
    for (int v = threadIdx.x; v < nvec; v += HEAD_THREADS) {
        const u32x4 q = __builtin_nontemporal_load(run + v);
#pragma unroll
        for (int j = 0; j < EPV; j++) image[v * EPV + j] = vec_element<F16>(q, j, vec_f16_to_f32) * scale;
    }
}
// vector v of the block's run of a big array from EPV floats
template <bool F16>
__device__ __forceinline__ void head_store_vector(void* dst, int K, int m0, int v, const float* vals) {
    constexpr int EPV = F16 ? 8 : 4;
    u32x4 q = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < EPV; j++) vec_put<F16>(q, j, vals[j]);
    __builtin_nontemporal_store(q, (u32x4*)((char*)dst + (size_t)m0 * (ACT_CANDIDATES * K) * (F16 ? 2 : 4)) + v);
}
// f(v, e0, s, k) for every vector v of the block: e0 its first element in the image, s its sample, k the piece of that element
template <bool F16, class F>
__device__ __forceinline__ void head_for_vectors(int K, int ng, F&& f) {
    constexpr int EPV = F16 ? 8 : 4;
    const int per = ACT_CANDIDATES * K, nvec = ng * per / EPV;
    for (int v = threadIdx.x; v < nvec; v += HEAD_THREADS) {
        const int e0 = v * EPV, s = e0 / per;
        f(v, e0, s, (e0 - s * per) % K);
    }
}

template <bool F16>
__device__ __forceinline__ void q_head_block(const HeadArgs& h, HeadImage& im, HeadQShared& sh) {
    constexpr int EPV = F16 ? 8 : 4;
    const int t = threadIdx.x, K = h.K, per = ACT_CANDIDATES * K, m0 = blockIdx.x * HEAD_BLOCK, ng = imin(HEAD_BLOCK, h.M - m0);
    const int ps = t / K, pk = t - ps * K;                    // the plane of thread t < ng K
    head_stream_in<F16>(h.x, K, m0, ng, h.rho, im.x);
    __syncthreads();
    if (t < ng * K) sh.plane[ps][pk] = head_plane(im.x + ps * per, K, pk);
    __syncthreads();
    if (t < ng) head_q_center(h, (size_t)(m0 + t), sh.plane[t], sh.q[t]);
    __syncthreads();
    head_for_vectors<F16>(K, ng, [&](int v, int e0, int s, int k) {
        float Q[EPV], A[EPV];
#pragma unroll
        for (int j = 0; j < EPV; j++) {
            A[j] = head_q_A(h, im.x[e0 + j], sh.q[s].sub[k]);
            Q[j] = sh.q[s].v[k] + A[j];
            k = k + 1 == K ? 0 : k + 1;
        }
        head_store_vector<F16>(h.out, K, m0, v, Q);
        if (h.out_A) head_store_vector<F16>(h.out_A, K, m0, v, A);
#pragma unroll
        for (int j = 0; j < EPV; j++) im.x[e0 + j] = F16 ? vec_f16_to_f32(plan_f32_to_f16(Q[j])) : Q[j];
    });
    __syncthreads();
    if (t < ng * K) im.red[ps][pk] = head_plane_max(im.x + ps * per, K, pk);
    __syncthreads();
    if (t < ng) h.V[m0 + t] = head_q_value(h, im.red[t]);
}

template <bool F16>
__device__ __forceinline__ void q_head_grad_block(const HeadArgs& h, HeadImage& im, float* g, HeadQShared& sh) {
    constexpr int EPV = F16 ? 8 : 4;
    const int t = threadIdx.x, K = h.K, per = ACT_CANDIDATES * K, m0 = blockIdx.x * HEAD_BLOCK, ng = imin(HEAD_BLOCK, h.M - m0);
    const int ps = t / K, pk = t - ps * K;
    head_stream_in<F16>(h.x, K, m0, ng, h.rho, im.x);
    head_stream_in<F16>(h.g, K, m0, ng, 1.0f, g);
    __syncthreads();
    if (t < ng * K) {
        sh.plane[ps][pk] = head_plane(im.x + ps * per, K, pk);
        im.red[ps][pk] = head_plane_sum(g + ps * per, K, pk);
    }
    __syncthreads();
    if (t < ng) {
        head_q_center(h, (size_t)(m0 + t), sh.plane[t], sh.q[t]);
        head_q_grad_v(h, (size_t)(m0 + t), im.red[t]);
    }
    __syncthreads();
    head_for_vectors<F16>(K, ng, [&](int, int e0, int s, int k) {
#pragma unroll
        for (int j = 0; j < EPV; j++) {
            g[e0 + j] = head_q_gd(g[e0 + j], head_q_A(h, im.x[e0 + j], sh.q[s].sub[k]));
            k = k + 1 == K ? 0 : k + 1;
        }
    });
    __syncthreads();
    if (t < ng * K) im.red[ps][pk] = head_plane_sum(g + ps * per, K, pk);
    __syncthreads();
    if (t < ng) head_q_shares(h, im.red[t], sh.plane[t], sh.q[t]);
    __syncthreads();
    head_for_vectors<F16>(K, ng, [&](int v, int e0, int s, int k) {
        float ga[EPV];
#pragma unroll
        for (int j = 0; j < EPV; j++) {
            ga[j] = head_q_grad_a(h, sh.q[s], k, im.x[e0 + j], g[e0 + j]);
            k = k + 1 == K ? 0 : k + 1;
        }
        head_store_vector<F16>(h.out, K, m0, v, ga);
    });
}

template <bool F16>
__device__ __forceinline__ void policy_head_block(const HeadArgs& h, HeadImage& im) {
    constexpr int EPV = F16 ? 8 : 4;
    const int t = threadIdx.x, K = h.K, per = ACT_CANDIDATES * K, m0 = blockIdx.x * HEAD_BLOCK, ng = imin(HEAD_BLOCK, h.M - m0);
    const int ps = t / K, pk = t - ps * K;
    head_stream_in<F16>(h.x, K, m0, ng, 1.0f, im.x);
    __syncthreads();
    if (t < ng * K) im.red[ps][pk] = head_plane_max(im.x + ps * per, K, pk);
    __syncthreads();
    head_for_vectors<F16>(K, ng, [&](int, int e0, int s, int k) {
#pragma unroll
        for (int j = 0; j < EPV; j++) {
            im.x[e0 + j] = expf(im.x[e0 + j] - im.red[s][k]);
            k = k + 1 == K ? 0 : k + 1;
        }
    });
    __syncthreads();
    if (t < ng * K) im.red[ps][pk] = head_plane_sum(im.x + ps * per, K, pk);
    __syncthreads();
    head_for_vectors<F16>(K, ng, [&](int v, int e0, int s, int k) {
        float pi[EPV];
#pragma unroll
        for (int j = 0; j < EPV; j++) {
            pi[j] = im.x[e0 + j] / im.red[s][k];
            k = k + 1 == K ? 0 : k + 1;
        }
        head_store_vector<F16>(h.out, K, m0, v, pi);
    });
    if (t < ng) head_policy_value(h, (size_t)(m0 + t));
}

template <bool F16>
__device__ __forceinline__ void policy_head_grad_block(const HeadArgs& h, HeadImage& im, float* g) {
    constexpr int EPV = F16 ? 8 : 4;
    const int t = threadIdx.x, K = h.K, per = ACT_CANDIDATES * K, m0 = blockIdx.x * HEAD_BLOCK, ng = imin(HEAD_BLOCK, h.M - m0);
    const int ps = t / K, pk = t - ps * K;
    head_stream_in<F16>(h.x, K, m0, ng, 1.0f, im.x);
    head_stream_in<F16>(h.g, K, m0, ng, 1.0f, g);
    __syncthreads();
    if (t < ng * K) im.red[ps][pk] = head_plane_dot(g + ps * per, im.x + ps * per, K, pk);
    __syncthreads();
    head_for_vectors<F16>(K, ng, [&](int v, int e0, int s, int k) {
        float gx[EPV];
#pragma unroll
        for (int j = 0; j < EPV; j++) {
            gx[j] = im.x[e0 + j] * (g[e0 + j] - im.red[s][k]);
            k = k + 1 == K ? 0 : k + 1;
        }
        head_store_vector<F16>(h.out, K, m0, v, gx);
    });
    if (t < ng) head_policy_value_grad(h, (size_t)(m0 + t));
}

__global__ __launch_bounds__(HEAD_THREADS) void k_q_head(HeadArgs h) {
    __shared__ HeadImage im;
    __shared__ HeadQShared sh;
    vec_with_f16(h.f16 != 0, [](auto F16, auto&&... a) { q_head_block<F16()>(a...); }, h, im, sh);
}
__global__ __launch_bounds__(HEAD_THREADS) void k_q_head_grad(HeadArgs h) {
    __shared__ HeadImage im;
    __shared__ __attribute__((aligned(16))) float g[HEAD_BLOCK * HEAD_PER];
    __shared__ HeadQShared sh;
    if (h.f16) q_head_grad_block<true>(h, im, g, sh); else q_head_grad_block<false>(h, im, g, sh);      // (written out: through vec_with_f16 its code moved)
}
__global__ __launch_bounds__(HEAD_THREADS) void k_policy_head(HeadArgs h) {
    __shared__ HeadImage im;
    vec_with_f16(h.f16 != 0, [](auto F16, auto&&... a) { policy_head_block<F16()>(a...); }, h, im);
}
__global__ __launch_bounds__(HEAD_THREADS) void k_policy_head_grad(HeadArgs h) {
    __shared__ HeadImage im;
    __shared__ __attribute__((aligned(16))) float g[HEAD_BLOCK * HEAD_PER];
    vec_with_f16(h.f16 != 0, [](auto F16, auto&&... a) { policy_head_grad_block<F16()>(a...); }, h, im, g);
}
