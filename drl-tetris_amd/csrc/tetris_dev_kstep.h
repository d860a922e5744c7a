// Kernels of libtetris_hip.so, part 7: the k-step target estimator (bodies: tetris_kstep.h).  Needs tetris_dev_vec.h.

// ---- the k-step target estimator (tetris_kstep.h).  Two launches in Q mode.  k_kstep_values works on the M n (sample, step) rows
// of Q, not on samples: a workgroup takes KSTEP_ROWS = 32 consecutive rows whatever n is — 32 x 40 K contiguous elements, 35 KB in
// float32 at K = 7 —, streams them into LDS as they lie with 16-byte loads, four in flight per lane, then thread (row, piece) walks
// its 40 elements of the image (stride K: the seven lanes of a row read consecutive words, the rows of a wave start 24 banks
// apart) and leaves the maximum in LDS, and thread `row` takes the masked mean into vals.  k_kstep_estimate is a lane per sample
// over vals (or, in V mode, over v itself) and the sample's k + 1 rows of reward and done; the discounts come from the kernel
// arguments, indexed by the loop counter, which is uniform.  No atomics, no workgroup waits for another.
template <bool F16>
__device__ __forceinline__ float kstep_lds_element(const uint32_t* image, int at) {
    if (F16) return vec_f16_to_f32(reinterpret_cast<const uint16_t*>(image)[at]);
    return u2f(image[at]);
}

template <int K, bool F16>
__device__ __forceinline__ void kstep_values_block(const KstepArgs& a, uint32_t* image, float* best_of) {
    constexpr int EPV = F16 ? 8 : 4, PER = ACT_CANDIDATES * K, LOADS = 4;
    static_assert(PER % EPV == 0, "a 16-byte vector must not cross two rows");
    const int t = threadIdx.x;
    const long long rows = (long long)a.M * a.n, r0 = (long long)blockIdx.x * KSTEP_ROWS;
    const int nr = rows - r0 < KSTEP_ROWS ? (int)(rows - r0) : KSTEP_ROWS;
    const u32x4* src = (const u32x4*)((const char*)a.x + (size_t)r0 * PER * (F16 ? 2 : 4));
    u32x4* dst = reinterpret_cast<u32x4*>(image);
    const int nvec = nr * (PER / EPV);
    for (int v0 = t; v0 < nvec; v0 += KSTEP_VALUE_THREADS * LOADS) {
        u32x4 q[LOADS];
#pragma unroll
        for (int u = 0; u < LOADS; u++) {
            const int v = v0 + u * KSTEP_VALUE_THREADS;
            if (v < nvec) q[u] = __builtin_nontemporal_load(src + v);
        }
#pragma unroll
        for (int u = 0; u < LOADS; u++) {
            const int v = v0 + u * KSTEP_VALUE_THREADS;
            if (v < nvec) dst[v] = q[u];
        }
    }
    __syncthreads();
    if (t < nr * K) {
        const int row = t / K, p = t - row * K, at = row * PER + p;
        float best = kstep_lds_element<F16>(image, at);
#pragma unroll 8
        for (int c = 1; c < ACT_CANDIDATES; c++) {
            const float x = kstep_lds_element<F16>(image, at + c * K);
            best = best < x ? x : best;
        }
        best_of[row * KSTEP_PIECES + p] = best;
    }
    __syncthreads();
    if (t < nr) {
        const size_t row = (size_t)r0 + (size_t)t;
        a.vals[row] = kstep_valid(a, row / (size_t)a.n) ? kstep_mean(a, K, best_of + t * KSTEP_PIECES, 1) : 0.0f;
    }
}

__global__ __launch_bounds__(KSTEP_VALUE_THREADS) void k_kstep_values(KstepArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t image[KSTEP_ROWS * ACT_CANDIDATES * 7];
    __shared__ float best_of[KSTEP_ROWS * KSTEP_PIECES];
    static_assert(KSTEP_ROWS * 7 <= KSTEP_VALUE_THREADS, "a thread per (row, piece)");
    vec_with_k_f16(a.K, a.f16 != 0, [](auto K, auto F16, auto&&... v) { kstep_values_block<K(), F16()>(v...); }, a, image, best_of);
}

__global__ __launch_bounds__(KSTEP_THREADS) void k_kstep_estimate(KstepArgs a) {
    const size_t j = (size_t)blockIdx.x * KSTEP_THREADS + threadIdx.x;
    if (j < (size_t)a.M) kstep_sample(a, j);
}
