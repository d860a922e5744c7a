// Kernels of libtetris_hip.so, part 5: the acting, window and replay half of tetris_lib_agent.h: acting on a network's evaluation,
// the trainers' loss heads, trajectory windows, a window's states, sample sets and minibatches, the planning agent's windows, experience replay and its radix
// sort.  Needs
// tetris_dev_observe.h (obs_row_words, obs_row_halves).  Every kernel here has one named block size: its launch bounds and its
// launch in tetris_lib_agent.h both use it.

// ---- acting on a network's evaluation (tetris_act.h).  A workgroup takes ACT_BLOCK consecutive games: it loads their piece
// indices, streams their contiguous ACT_BLOCK x 40 K elements of action_eval with 16-byte loads (every cache line is touched
// whichever piece a game holds, so it is read once, coalesced, instead of 40 strided elements per lane), keeps the elements of
// each game's piece and lays them into LDS candidate-major with a stride of ACT_LDS_STRIDE floats; then one lane per game
// chooses from its column.  RANK's 40 x 40 comparisons are spread over the workgroup's lanes, one (game, candidate) pair at a
// time.
struct ActShared {
    float x[ACT_CANDIDATES * ACT_LDS_STRIDE];     // the values, [c][game]
    float m[ACT_CANDIDATES * ACT_LDS_STRIDE];     // the weights of the sampling modes
    float table[ACT_CANDIDATES];
    int piece[ACT_BLOCK];
};
typedef uint32_t act_u32x4 __attribute__((ext_vector_type(4)));

// element j of a 16-byte vector as float32 (j is not a constant: selects, no indexed registers)
template <bool F16>
__device__ __forceinline__ float act_vector_element(const act_u32x4& q, int j) {
    const int w = F16 ? j >> 1 : j;
    const uint32_t word = w == 0 ? q.x : w == 1 ? q.y : w == 2 ? q.z : q.w;
    return F16 ? act_f16_to_f32((uint16_t)((j & 1) ? word >> 16 : word & 0xFFFFu)) : u2f(word);
}

// The block's elements, 16 bytes per lane and load.  Element e of the block belongs to game e / (40 K), candidate (e mod 40 K) / K
// and piece e mod K; 40 K is a multiple of the 4 or 8 elements of a vector, so a vector lies inside one game and (K = 7) holds
// at most two elements of the game's piece: only those are converted and stored.
template <int NT, int K, bool F16>
__device__ __forceinline__ void act_gather(const void* eval, int g0, int ng, ActShared& sh) {
    constexpr int EPV = F16 ? 8 : 4, PER_GAME = ACT_CANDIDATES * K;
    static_assert(PER_GAME % EPV == 0, "a 16-byte vector must not cross two games");
    const act_u32x4* src = (const act_u32x4*)((const char*)eval + (size_t)g0 * PER_GAME * (F16 ? 2 : 4));
    const int nvec = ng * (PER_GAME / EPV);
#pragma unroll 4
    for (int v = threadIdx.x; v < nvec; v += NT) {
        const act_u32x4 q = src[v];
        const int e0 = v * EPV, game = e0 / PER_GAME, rem = e0 - game * PER_GAME;
        if (K == 1) {
#pragma unroll
            for (int j = 0; j < EPV; j++) sh.x[(rem + j) * ACT_LDS_STRIDE + game] = act_vector_element<F16>(q, j);
        } else {
            int j = sh.piece[game] - rem % K;                 // the first element of the vector that belongs to the piece
            j = j < 0 ? j + K : j;
            if (j < EPV) sh.x[((rem + j) / K) * ACT_LDS_STRIDE + game] = act_vector_element<F16>(q, j);
            if (EPV > K && j + K < EPV) sh.x[((rem + j + K) / K) * ACT_LDS_STRIDE + game] = act_vector_element<F16>(q, j + K);
        }
    }
}

// the gather for K = 7 or 1 and either element type; sh.piece holds the games' pieces
template <int NT>
__device__ __forceinline__ void act_gather_any(const void* eval, int K, bool f16, int g0, int ng, ActShared& sh) {
    if (K == 7) {
        if (f16) act_gather<NT, 7, true>(eval, g0, ng, sh); else act_gather<NT, 7, false>(eval, g0, ng, sh);
    } else {
        if (f16) act_gather<NT, 1, true>(eval, g0, ng, sh); else act_gather<NT, 1, false>(eval, g0, ng, sh);
    }
}

// games g0 .. g0 + ng - 1 by a workgroup of NT threads: every thread passes the barriers; thread t < ng chooses for game g0 + t
// and writes its outputs
template <int NT>
__device__ __forceinline__ void act_block_choose(const ActArgs& aa, int g0, int ng, ActShared& sh) {
    static_assert(NT % ACT_BLOCK == 0 && NT >= ACT_BLOCK, "whole waves of ACT_BLOCK lanes");
    const int t = threadIdx.x;
    if (t < ACT_BLOCK) sh.piece[t] = t < ng ? act_piece_of(geo_of(aa.a), (size_t)(g0 + t), safe_player(aa.player, g0 + t, aa.a.n_players), aa.K) : 0;
    if (t < ACT_CANDIDATES) sh.table[t] = aa.table[t];
    __syncthreads();
    act_gather_any<NT>(aa.action_eval, aa.K, aa.eval_f16 != 0, g0, ng, sh);
    __syncthreads();
    const bool rank = aa.mode == ACT_RANK;
    if (rank) {                                       // lane = (game, candidate): its 39 rivals from LDS, conflict-free
        const int g = t & (ACT_BLOCK - 1);
        if (g < ng)
            for (int c = t / ACT_BLOCK; c < ACT_CANDIDATES; c += NT / ACT_BLOCK)
                sh.m[c * ACT_LDS_STRIDE + g] = sh.table[act_rank(sh.x + g, ACT_LDS_STRIDE, c) - 1];
        __syncthreads();
    }
    if (t >= ng) return;
    const int c = act_choose(aa, g0 + t, sh.table, sh.x + t, ACT_LDS_STRIDE, sh.m + t, ACT_LDS_STRIDE, rank);
    act_write(aa, g0 + t, sh.piece[t], c, sh.x + t, ACT_LDS_STRIDE);
}

// tetris_select_eval_dev: the choice and its outputs
constexpr int ACT_THREADS = 256;
__global__ __launch_bounds__(ACT_THREADS) void k_act_select(ActArgs aa) {
    __shared__ ActShared sh;
    const int g0 = blockIdx.x * ACT_BLOCK, ng = imin(ACT_BLOCK, aa.a.n - g0);
    act_block_choose<ACT_THREADS>(aa, g0, ng, sh);
}

// ---- loss heads (tetris_loss.h).  The same access pattern, there and back: a workgroup takes LOSS_BLOCK = ACT_BLOCK consecutive
// samples, whose pieces come from the action array; act_gather streams their contiguous 64 x 40 K elements of pi / Q into the
// first LDS plane; one lane per sample (wave 0) computes the head from its column and leaves its 40 gradient values in the second
// plane; then the whole workgroup writes the block's gradient region as 16-byte vectors — zeros but the pieces' elements, which
// come from LDS — in memory order, so no lane issues 40 strided stores.  The lanes' terms of the statistics are reduced across
// wave 0 by shuffles in the order of loss_tree into the workgroup's partial row; k_loss_reduce sums the rows.  D / Dnz come
// from k_loss_count through a device word when a valid mask or weights are given.  No workgroup waits for another.
struct LossShared {
    ActShared act;                  // x: the values, m: the gradients, piece: the samples' pieces
    float gv[LOSS_BLOCK];           // PPO: the value gradients
};

// 0 | val into element j of a zeroed 16-byte vector (j is not a constant: selects, no indexed registers)
template <bool F16>
__device__ __forceinline__ void act_vector_put(act_u32x4& q, int j, float val) {
    const int w = F16 ? j >> 1 : j;
    const uint32_t bits = F16 ? (uint32_t)plan_f32_to_f16(val) << ((j & 1) * 16) : f2u(val);
    q.x |= w == 0 ? bits : 0u; q.y |= w == 1 ? bits : 0u; q.z |= w == 2 ? bits : 0u; q.w |= w == 3 ? bits : 0u;
}

// The opposite direction of act_gather: the block's ng x 40 K gradient elements, 16 bytes per lane and store.  The elements of
// a sample's piece are sh.m[candidate][sample], all others zero.
template <int NT, int K, bool F16>
__device__ __forceinline__ void loss_scatter(void* grad, int g0, int ng, const ActShared& sh) {
    constexpr int EPV = F16 ? 8 : 4, PER = ACT_CANDIDATES * K;
    static_assert(PER % EPV == 0, "a 16-byte vector must not cross two samples");
    act_u32x4* dst = (act_u32x4*)((char*)grad + (size_t)g0 * PER * (F16 ? 2 : 4));
    const int nvec = ng * (PER / EPV);
#pragma unroll 4
    for (int v = threadIdx.x; v < nvec; v += NT) {
        const int e0 = v * EPV, s = e0 / PER, rem = e0 - s * PER;
        act_u32x4 q = {0u, 0u, 0u, 0u};
        if (K == 1) {
#pragma unroll
            for (int j = 0; j < EPV; j++) act_vector_put<F16>(q, j, sh.m[(rem + j) * ACT_LDS_STRIDE + s]);
        } else {
            int j = sh.piece[s] - rem % K;                    // the first element of the vector that belongs to the piece
            j = j < 0 ? j + K : j;
            if (j < EPV) act_vector_put<F16>(q, j, sh.m[((rem + j) / K) * ACT_LDS_STRIDE + s]);
            if (EPV > K && j + K < EPV) act_vector_put<F16>(q, j + K, sh.m[((rem + j + K) / K) * ACT_LDS_STRIDE + s]);
        }
        __builtin_nontemporal_store(q, dst + v);
    }
}

constexpr int LOSS_THREADS = 256;
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_head(LossArgs la) {
    __shared__ LossShared sh;
    static_assert(LOSS_BLOCK == 64, "wave 0 holds a lane per sample");
    const int t = threadIdx.x, g0 = blockIdx.x * LOSS_BLOCK, ng = imin(LOSS_BLOCK, la.M - g0);
    int k = 0, c = 0;
    if (t < LOSS_BLOCK) {
        if (t < ng) loss_action(la, (size_t)(g0 + t), k, c);
        sh.act.piece[t] = k;
    }
    __syncthreads();
    act_gather_any<LOSS_THREADS>(la.x, la.K, la.in_f16 != 0, g0, ng, sh.act);
    __syncthreads();
    if (t < LOSS_BLOCK) {                                    // wave 0, every lane: lanes past ng add zeros to the sums
        const float D = la.count ? (float)la.count[0] : (float)la.M, Dnz = la.count ? (float)la.count[1] : (float)la.M;
        float sum[LOSS_SUMS], gv;
        loss_sample(la, t < ng ? (long long)(g0 + t) : (long long)la.M, k, c, D, Dnz, sh.act.x + t, ACT_LDS_STRIDE, sh.act.m + t, ACT_LDS_STRIDE, sum, gv);
        sh.gv[t] = gv;
#pragma unroll
        for (int i = 0; i < LOSS_SUMS; i++) {
            float s = sum[i];
#pragma unroll
            for (int off = LOSS_BLOCK / 2; off >= 1; off >>= 1) s += __shfl_down(s, off, LOSS_BLOCK);
            if (t == 0) la.partial[(size_t)blockIdx.x * LOSS_SUMS + i] = s;
        }
    }
    __syncthreads();
    if (la.K == 7) {
        if (la.grad_f16) loss_scatter<LOSS_THREADS, 7, true>(la.grad_x, g0, ng, sh.act); else loss_scatter<LOSS_THREADS, 7, false>(la.grad_x, g0, ng, sh.act);
    } else {
        if (la.grad_f16) loss_scatter<LOSS_THREADS, 1, true>(la.grad_x, g0, ng, sh.act); else loss_scatter<LOSS_THREADS, 1, false>(la.grad_x, g0, ng, sh.act);
    }
    if (la.head == LOSS_PPO)                                 // the block's ng x V value gradients, in memory order
        for (int e = t; e < ng * la.V; e += LOSS_THREADS) {
            const int s = e / la.V, kk = e - s * la.V;
            loss_store(la.grad_v, (size_t)g0 * la.V + e, kk == imin(sh.act.piece[s], la.V - 1) ? sh.gv[s] : 0.0f, la.grad_f16);
        }
}

// D and Dnz of the call, by one workgroup: a lane per sample and trip, the lanes' counts through LDS (integer adds)
constexpr int LOSS_COUNT_THREADS = 1024;
__global__ __launch_bounds__(LOSS_COUNT_THREADS) void k_loss_count(LossArgs la, uint32_t* count) {
    __shared__ uint32_t total[2];
    if (threadIdx.x < 2) total[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t d = 0u, dnz = 0u;
#pragma unroll 4
    for (int m = threadIdx.x; m < la.M; m += LOSS_COUNT_THREADS) loss_count_sample(la, (size_t)m, d, dnz);
    atomicAdd(&total[0], d);
    atomicAdd(&total[1], dnz);
    __syncthreads();
    if (threadIdx.x < 2) count[threadIdx.x] = total[threadIdx.x];
}

// the partial rows of the head's workgroups -> stats, by one workgroup, in the order of loss_reduce_serial
__global__ __launch_bounds__(LOSS_REDUCE_LANES) void k_loss_reduce(LossArgs la, int blocks) {
    __shared__ float slot[LOSS_SUMS][LOSS_REDUCE_LANES];
    const int t = threadIdx.x;
    float s[LOSS_SUMS];
#pragma unroll
    for (int i = 0; i < LOSS_SUMS; i++) s[i] = 0.0f;
    for (int b = t; b < blocks; b += LOSS_REDUCE_LANES) {
#pragma unroll
        for (int i = 0; i < LOSS_SUMS; i++) s[i] += la.partial[(size_t)b * LOSS_SUMS + i];
    }
#pragma unroll
    for (int i = 0; i < LOSS_SUMS; i++) slot[i][t] = s[i];
    __syncthreads();
    for (int off = LOSS_REDUCE_LANES / 2; off >= 1; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int i = 0; i < LOSS_SUMS; i++) slot[i][t] += slot[i][t + off];
        }
        __syncthreads();
    }
    if (t == 0) {
        float total[LOSS_SUMS];
#pragma unroll
        for (int i = 0; i < LOSS_SUMS; i++) total[i] = slot[i][0];
        const float D = la.count ? (float)la.count[0] : (float)la.M, Dnz = la.count ? (float)la.count[1] : (float)la.M;
        loss_finish(la, total, D, Dnz, la.stats);
    }
}

// ---- the k-step target estimator (tetris_kstep.h).  Two launches in Q mode.  k_kstep_values works on the M n (sample, step) rows
// of Q, not on samples: a workgroup takes KSTEP_ROWS = 32 consecutive rows whatever n is — 32 x 40 K contiguous elements, 35 KB in
// float32 at K = 7 —, streams them into LDS as they lie with 16-byte loads, four in flight per lane, then thread (row, piece) walks
// its 40 elements of the image (stride K: the seven lanes of a row read consecutive words, the rows of a wave start 24 banks
// apart) and leaves the maximum in LDS, and thread `row` takes the masked mean into vals.  k_kstep_estimate is a lane per sample
// over vals (or, in V mode, over v itself) and the sample's k + 1 rows of reward and done; the discounts come from the kernel
// arguments, indexed by the loop counter, which is uniform.  No atomics, no workgroup waits for another.
template <bool F16>
__device__ __forceinline__ float kstep_lds_element(const uint32_t* image, int at) {
    if (F16) return (float)__builtin_bit_cast(_Float16, reinterpret_cast<const uint16_t*>(image)[at]);      // (exact)
    return u2f(image[at]);
}

template <int K, bool F16>
__device__ __forceinline__ void kstep_values_block(const KstepArgs& a, uint32_t* image, float* best_of) {
    constexpr int EPV = F16 ? 8 : 4, PER = ACT_CANDIDATES * K, LOADS = 4;
    static_assert(PER % EPV == 0, "a 16-byte vector must not cross two rows");
    const int t = threadIdx.x;
    const long long rows = (long long)a.M * a.n, r0 = (long long)blockIdx.x * KSTEP_ROWS;
    const int nr = rows - r0 < KSTEP_ROWS ? (int)(rows - r0) : KSTEP_ROWS;
    const act_u32x4* src = (const act_u32x4*)((const char*)a.x + (size_t)r0 * PER * (F16 ? 2 : 4));
    act_u32x4* dst = reinterpret_cast<act_u32x4*>(image);
    const int nvec = nr * (PER / EPV);
    for (int v0 = t; v0 < nvec; v0 += KSTEP_VALUE_THREADS * LOADS) {
        act_u32x4 q[LOADS];
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
    if (a.K == 7) {
        if (a.f16) kstep_values_block<7, true>(a, image, best_of); else kstep_values_block<7, false>(a, image, best_of);
    } else {
        if (a.f16) kstep_values_block<1, true>(a, image, best_of); else kstep_values_block<1, false>(a, image, best_of);
    }
}

__global__ __launch_bounds__(KSTEP_THREADS) void k_kstep_estimate(KstepArgs a) {
    const size_t j = (size_t)blockIdx.x * KSTEP_THREADS + threadIdx.x;
    if (j < (size_t)a.M) kstep_sample(a, j);
}

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
    const act_u32x4* run = (const act_u32x4*)((const char*)src + (size_t)m0 * per * (F16 ? 2 : 4));
#pragma unroll 2
    for (int v = threadIdx.x; v < nvec; v += HEAD_THREADS) {
        const act_u32x4 q = __builtin_nontemporal_load(run + v);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < EPV; j++) {
            const float x = F16 ? (float)__builtin_bit_cast(_Float16, (uint16_t)((j & 1) ? w[j >> 1] >> 16 : w[j >> 1] & 0xFFFFu)) : u2f(w[j]);      // (exact)
            image[v * EPV + j] = x * scale;
        }
    }
}
// vector v of the block's run of a big array from EPV floats
template <bool F16>
__device__ __forceinline__ void head_store_vector(void* dst, int K, int m0, int v, const float* vals) {
    constexpr int EPV = F16 ? 8 : 4;
    act_u32x4 q = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < EPV; j++) act_vector_put<F16>(q, j, vals[j]);
    __builtin_nontemporal_store(q, (act_u32x4*)((char*)dst + (size_t)m0 * (ACT_CANDIDATES * K) * (F16 ? 2 : 4)) + v);
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
        for (int j = 0; j < EPV; j++) im.x[e0 + j] = F16 ? (float)__builtin_bit_cast(_Float16, plan_f32_to_f16(Q[j])) : Q[j];
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
    if (h.f16) q_head_block<true>(h, im, sh); else q_head_block<false>(h, im, sh);
}
__global__ __launch_bounds__(HEAD_THREADS) void k_q_head_grad(HeadArgs h) {
    __shared__ HeadImage im;
    __shared__ __attribute__((aligned(16))) float g[HEAD_BLOCK * HEAD_PER];
    __shared__ HeadQShared sh;
    if (h.f16) q_head_grad_block<true>(h, im, g, sh); else q_head_grad_block<false>(h, im, g, sh);
}
__global__ __launch_bounds__(HEAD_THREADS) void k_policy_head(HeadArgs h) {
    __shared__ HeadImage im;
    if (h.f16) policy_head_block<true>(h, im); else policy_head_block<false>(h, im);
}
__global__ __launch_bounds__(HEAD_THREADS) void k_policy_head_grad(HeadArgs h) {
    __shared__ HeadImage im;
    __shared__ __attribute__((aligned(16))) float g[HEAD_BLOCK * HEAD_PER];
    if (h.f16) policy_head_grad_block<true>(h, im, g); else policy_head_grad_block<false>(h, im, g);
}

// ---- the planning loss head (tetris_loss.h: PLAN).  A sample is HW K contiguous elements — 5 600 bytes at H = 20, K = 7 in
// float32 — so a workgroup takes PLAN_LOSS_BLOCK = 16 consecutive samples (a multiple of 8: its run of phi and of grad_phi starts
// on 16 bytes for every H, K and element type), four per wave:
//   a. lane t < 16: the sample's piece, whether it is valid, whether it is the mirrored image;
//   b. the whole workgroup streams the block's contiguous run of phi in with 16-byte loads and drops the elements of each
//      sample's piece into its LDS plane [sample][cell] (a vector may straddle two samples: the element walk carries sample, cell
//      and piece index along, one division per vector); 28 consecutive lanes per sample read the record's 28 quads once, zeros
//      for an index that names no entry;
//   c. a wave per sample at a time: lane l holds cells l, l + 64, .. (at most PLAN_LOSS_CELLS = 5) in registers across both passes —
//      the four sums of pass one and the entropy sum of pass two are reduced by shuffles in the order of loss_tree and handed back
//      to every lane — and leaves g_t in the plane it read raw_t from; lane 0 writes the sample's terms;
//   d. the workgroup streams the block's gradient run out as 16-byte non-temporal stores in memory order, zeros but the pieces'
//      elements from LDS; the run's last elements, where it is no multiple of 16 bytes (a short last block), leave one by one.
// Thread i < LOSS_SUMS adds the block's 16 sample terms of sum i by loss_tree into the partial row; k_loss_count and k_loss_reduce
// serve as for the other heads.  LDS: 20 KB of planes, 7 KB of records, 1 KB of the rest.  No atomics, no workgroup waits for
// another.
constexpr int PLAN_LOSS_THREADS = 256;
constexpr int PLAN_LOSS_PITCH = 320;             // floats of a sample's LDS plane (MAX_H * NCOL = 310 cells)
static_assert(PLAN_LOSS_PITCH >= MAX_H * NCOL && PLAN_LOSS_CELLS * PLAN_LOSS_LANES >= MAX_H * NCOL, "a plane holds every height");
static_assert(PLAN_LOSS_BLOCK % 8 == 0 && PLAN_LOSS_BLOCK % (PLAN_LOSS_THREADS / 64) == 0, "aligned runs; whole rounds of the waves");
struct PlanLossShared {
    alignas(16) uint32_t rec[PLAN_LOSS_BLOCK * PLAN_REC_WORDS];
    float x[PLAN_LOSS_BLOCK * PLAN_LOSS_PITCH];      // raw_t, then g_t
    float sum[LOSS_SUMS][PLAN_LOSS_BLOCK];
    float gv[PLAN_LOSS_BLOCK];
    int piece[PLAN_LOSS_BLOCK];
    uint32_t flags[PLAN_LOSS_BLOCK];                 // bit 0: a valid sample, bit 1: the mirrored image
};

// b and d: the walk over the block's run.  PUT = false: phi -> planes; PUT = true: planes -> grad_phi.
template <int K, bool F16, bool PUT>
__device__ __forceinline__ void plan_loss_stream(const LossArgs& la, int g0, int ng, PlanLossShared& sh) {
    constexpr uint32_t EPV = F16 ? 8 : 4;
    const uint32_t PER = (uint32_t)la.H * NCOL * K, total = (uint32_t)ng * PER, nvec = total / EPV;
    void* whole = PUT ? la.grad_x : const_cast<void*>(la.x);
    act_u32x4* run = (act_u32x4*)((char*)whole + (size_t)g0 * PER * (F16 ? 2 : 4));
#pragma unroll 2
    for (uint32_t v = threadIdx.x; v < nvec; v += PLAN_LOSS_THREADS) {
        act_u32x4 q = {0u, 0u, 0u, 0u};
        if (!PUT) q = run[v];
        const uint32_t e0 = v * EPV;
        uint32_t s = e0 / PER, rem = e0 - s * PER;
        uint32_t cell = rem / K, kk = rem - cell * K;
#pragma unroll
        for (int j = 0; j < (int)EPV; j++) {
            if ((int)kk == sh.piece[s]) {
                if (PUT) act_vector_put<F16>(q, j, sh.x[s * PLAN_LOSS_PITCH + cell]);
                else sh.x[s * PLAN_LOSS_PITCH + cell] = act_vector_element<F16>(q, j);
            }
            kk++; rem++;
            if (kk == K) { kk = 0u; cell++; }
            if (rem == PER && j + 1 < (int)EPV) { rem = 0u; cell = 0u; kk = 0u; s++; }
        }
        if (PUT) __builtin_nontemporal_store(q, run + v);
    }
    for (uint32_t e = nvec * EPV + threadIdx.x; e < total; e += PLAN_LOSS_THREADS) {
        const uint32_t s = e / PER, rem = e - s * PER, cell = rem / K, kk = rem - cell * K;
        const size_t at = (size_t)g0 * PER + e;
        if (PUT) loss_store(la.grad_x, at, (int)kk == sh.piece[s] ? sh.x[s * PLAN_LOSS_PITCH + cell] : 0.0f, F16 ? 1 : 0);
        else if ((int)kk == sh.piece[s]) sh.x[s * PLAN_LOSS_PITCH + cell] = act_element(la.x, at, F16 ? 1 : 0);
    }
}
template <bool PUT>
__device__ __forceinline__ void plan_loss_stream_any(const LossArgs& la, int g0, int ng, PlanLossShared& sh) {
    const bool f16 = PUT ? la.grad_f16 != 0 : la.in_f16 != 0;
    if (la.K == 7) {
        if (f16) plan_loss_stream<7, true, PUT>(la, g0, ng, sh); else plan_loss_stream<7, false, PUT>(la, g0, ng, sh);
    } else {
        if (f16) plan_loss_stream<1, true, PUT>(la, g0, ng, sh); else plan_loss_stream<1, false, PUT>(la, g0, ng, sh);
    }
}
// a wave's sum in the order of loss_tree, handed to every lane
__device__ __forceinline__ float plan_loss_wave_sum(float s) {
#pragma unroll
    for (int off = PLAN_LOSS_LANES / 2; off >= 1; off >>= 1) s += __shfl_down(s, off, PLAN_LOSS_LANES);
    return __shfl(s, 0, PLAN_LOSS_LANES);
}

__global__ __launch_bounds__(PLAN_LOSS_THREADS) void k_plan_loss_head(LossArgs la) {
    __shared__ PlanLossShared sh;
    static_assert(PLAN_LOSS_LANES == 64, "a wave holds a lane per residue of the cell order");
    const int t = threadIdx.x, g0 = blockIdx.x * PLAN_LOSS_BLOCK, ng = imin(PLAN_LOSS_BLOCK, la.M - g0);
    const int HW = la.H * NCOL;
    if (t < PLAN_LOSS_BLOCK) {                                                           // a
        int k = 0;
        uint32_t flags = 0u;
        if (t < ng) {
            const size_t m = (size_t)(g0 + t);
            k = plan_loss_piece(la, m);
            const BatchEntry en = batch_index_entry((uint32_t)la.index[m], la.total);
            flags = (loss_valid(la, m) ? 1u : 0u) | (en.mirror ? 2u : 0u);
        }
        sh.piece[t] = k;
        sh.flags[t] = flags;
    }
    __syncthreads();
    plan_loss_stream_any<false>(la, g0, ng, sh);                                         // b
    for (int e = t; e < ng * PLAN_REC_QUADS; e += PLAN_LOSS_THREADS) {
        const int j = e / PLAN_REC_QUADS, q = e - j * PLAN_REC_QUADS;
        const BatchEntry en = batch_index_entry((uint32_t)la.index[g0 + j], la.total);
        // (an entry that names no sample has at = 0: entry 0 is loaded and dropped word by word, as in k_traj_plan_batch)
        act_u32x4 w = reinterpret_cast<const act_u32x4*>(la.rec + (size_t)en.at * PLAN_REC_WORDS)[q];
        const uint32_t keep = en.valid ? ~0u : 0u;
        w.x &= keep; w.y &= keep; w.z &= keep; w.w &= keep;
        *reinterpret_cast<act_u32x4*>(sh.rec + j * PLAN_REC_WORDS + 4 * q) = w;
    }
    __syncthreads();
    const float D = la.count ? (float)la.count[0] : (float)la.M;
    const int lane = t & (PLAN_LOSS_LANES - 1), wave = __builtin_amdgcn_readfirstlane(t >> 6);
    for (int s = wave; s < ng; s += PLAN_LOSS_THREADS / PLAN_LOSS_LANES) {               // c
        const size_t m = (size_t)(g0 + s);
        float* plane = sh.x + s * PLAN_LOSS_PITCH;
        float sum[LOSS_SUMS], gv = 0.0f;
#pragma unroll
        for (int i = 0; i < LOSS_SUMS; i++) sum[i] = 0.0f;
        if ((sh.flags[s] & 1u) && D > 0.0f) {
            const uint32_t* r = sh.rec + s * PLAN_REC_WORDS;
            const bool mirror = (sh.flags[s] & 2u) != 0u;
            PlanCell pc[PLAN_LOSS_CELLS];
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < PLAN_LOSS_CELLS; c++) {
                const int cell = lane + c * PLAN_LOSS_LANES;
                const bool live = cell < HW;
                pc[c] = plan_cell(r, mirror, live ? cell : 0, live ? plane[cell] : 0.0f, la.small_fill);
                float four[4];
                plan_cell_terms(pc[c], four);
#pragma unroll
                for (int i = 0; i < 4; i++) acc[i] += live ? four[i] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 4; i++) acc[i] = plan_loss_wave_sum(acc[i]);
            PlanSample ps;
            plan_sample_policy(la, m, sh.piece[s], D, acc[0], acc[1], acc[2], ps);
            float l[PLAN_LOSS_CELLS], above[PLAN_LOSS_CELLS], ent = 0.0f;
#pragma unroll
            for (int c = 0; c < PLAN_LOSS_CELLS; c++) {
                const bool live = lane + c * PLAN_LOSS_LANES < HW;
                const float term = plan_cell_entropy(pc[c], ps.S, l[c], above[c]);
                ent += live ? term : 0.0f;
            }
            ps.Hent = -plan_loss_wave_sum(ent);
#pragma unroll
            for (int c = 0; c < PLAN_LOSS_CELLS; c++) {
                const int cell = lane + c * PLAN_LOSS_LANES;
                if (cell < HW) plane[cell] = plan_cell_grad(la, ps, pc[c], l[c], above[c]);
            }
            if (lane == 0) plan_sample_finish(la, m, D, ps, acc[3], sum, gv);
        } else {
            for (int cell = lane; cell < HW; cell += PLAN_LOSS_LANES) plane[cell] = 0.0f;
            if (lane == 0) plan_sample_zero_terms(la, m);
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < LOSS_SUMS; i++) sh.sum[i][s] = sum[i];
            sh.gv[s] = gv;
        }
    }
    if (t >= ng && t < PLAN_LOSS_BLOCK) {                    // the samples past M of a last, short block add zeros
#pragma unroll
        for (int i = 0; i < LOSS_SUMS; i++) sh.sum[i][t] = 0.0f;
    }
    __syncthreads();
    if (t < LOSS_SUMS) {
        float v[PLAN_LOSS_BLOCK];
#pragma unroll
        for (int i = 0; i < PLAN_LOSS_BLOCK; i++) v[i] = sh.sum[t][i];
        la.partial[(size_t)blockIdx.x * LOSS_SUMS + t] = loss_tree(v, PLAN_LOSS_BLOCK);
    }
    plan_loss_stream_any<true>(la, g0, ng, sh);                                          // d
    for (int e = t; e < ng * la.V; e += PLAN_LOSS_THREADS) {
        const int s = e / la.V, kk = e - s * la.V;
        loss_store(la.grad_v, (size_t)g0 * la.V + e, kk == imin(sh.piece[s], la.V - 1) ? sh.gv[s] : 0.0f, la.grad_f16);
    }
}

// ---- trajectory windows (tetris_traj.h).  Recording is one lane per game.
constexpr int TRAJ_LANE_THREADS = 256;      // k_traj_record and k_traj_observe: a lane per record
__global__ __launch_bounds__(TRAJ_LANE_THREADS) void k_traj_record(TrajRecordArgs ra) {
    const int i = blockIdx.x * TRAJ_LANE_THREADS + threadIdx.x;
    if (i < ra.n) traj_record_game(ra, i);
}

// The backward recurrence is sequential in t per game, so a lane that read its rows from memory as it went would pay a memory
// round trip per row with 64-1 024 waves on the whole GPU.  A workgroup of five waves takes TRAJ_BLOCK consecutive games:
// waves 1-4 stream tiles of TRAJ_TILE rows x 64 games — wave 1 the rewards, 2 value[0], 3 value[1], 4 the dones, each lane 16
// independent loads of its game's column, every load of a wave one contiguous 256 bytes (64 for the dones) — last tile first
// into one half of a double-buffered LDS image while wave 0, one lane per game, walks the other half backward and stores
// adv / target / closed, a contiguous row segment per store.  LDS rows are 64 words: lane l reads and writes bank l mod 32 of
// its half-wave, no conflicts.  Any N (lanes past N load nothing and store nothing), any rows (the last tile is the short one).
constexpr int TRAJ_THREADS = 5 * 64;      // one scanning wave and one loading wave per array
struct TrajShared {
    uint32_t w[2][4][TRAJ_TILE][TRAJ_BLOCK];      // [buffer][reward, value 0, value 1, done][row][game]
};

// rows t0 .. t0 + nr - 1 of array `which`, game g, into one buffer's column `lane` (all 16 loads issued before the first store;
// constant indices after unrolling: registers, no scratch)
__device__ __forceinline__ void traj_load_tile(const TrajAdvArgs& aa, int which, int g, bool live, int t0, int nr, int lane,
                                               uint32_t (*dst)[TRAJ_TILE][TRAJ_BLOCK]) {
    uint32_t v[TRAJ_TILE];
    const size_t at = (size_t)t0 * aa.n + g;
    if (which == 3) {
        const uint8_t* src = aa.done + at;
#pragma unroll
        for (int j = 0; j < TRAJ_TILE; j++) v[j] = (live && j < nr) ? (uint32_t)src[(size_t)j * aa.n] : 0u;
    } else {
        const float* src = (which == 0 ? aa.reward : which == 1 ? aa.value : aa.value + aa.plane) + at;
#pragma unroll
        for (int j = 0; j < TRAJ_TILE; j++) v[j] = (live && j < nr) ? f2u(src[(size_t)j * aa.n]) : 0u;
    }
#pragma unroll
    for (int j = 0; j < TRAJ_TILE; j++) dst[which][j][lane] = v[j];
}

__global__ __launch_bounds__(TRAJ_THREADS) void k_traj_advantages(TrajAdvArgs aa) {
    __shared__ TrajShared sh;
    const int lane = threadIdx.x & (TRAJ_BLOCK - 1), wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / TRAJ_BLOCK);
    const int g = blockIdx.x * TRAJ_BLOCK + lane;
    const bool live = g < aa.n;
    const int ntiles = (aa.rows + TRAJ_TILE - 1) / TRAJ_TILE;
    TrajScan s;
    traj_scan_begin(s, (wave == 0 && live && aa.boot) ? aa.boot[g] : 0.0f);
    if (wave != 0) traj_load_tile(aa, wave - 1, g, live, (ntiles - 1) * TRAJ_TILE, aa.rows - (ntiles - 1) * TRAJ_TILE, lane, sh.w[0]);
    __syncthreads();
    int cur = 0;
    for (int k = ntiles - 1; k >= 0; k--, cur ^= 1) {
        const int t0 = k * TRAJ_TILE, nr = imin(TRAJ_TILE, aa.rows - t0);
        if (wave == 0) {
#pragma unroll 4
            for (int j = nr - 1; j >= 0; j--) {
                float adv, target;
                traj_scan_row(s, aa, u2f(sh.w[cur][0][j][lane]), u2f(sh.w[cur][1][j][lane]), u2f(sh.w[cur][2][j][lane]),
                              sh.w[cur][3][j][lane] != 0u, adv, target);
                if (live) {
                    const size_t at = (size_t)(t0 + j) * aa.n + g;
                    aa.adv[at] = adv;
                    aa.target[at] = target;
                    if (aa.closed) aa.closed[at] = (uint8_t)s.seen;
                }
            }
        } else if (k > 0) {
            traj_load_tile(aa, wave - 1, g, live, t0 - TRAJ_TILE, TRAJ_TILE, lane, sh.w[cur ^ 1]);
        }
        __syncthreads();
    }
}

// ---- a window's states and sample sets (tetris_batch.h)
// tetris_traj_observe_dev: one lane per (game, slot) record
__global__ __launch_bounds__(TRAJ_LANE_THREADS) void k_traj_observe(TrajObserveArgs oa) {
    const int i = blockIdx.x * TRAJ_LANE_THREADS + threadIdx.x;
    if (i < oa.n) traj_observe_slot(oa, i, (int)blockIdx.y);
}

// tetris_traj_select_dev in three launches, none of which waits for another workgroup: the non-zero bytes of every workgroup's
// SELECT_ELEMS mask bytes (16 per lane, one 16-byte load); the exclusive scan of those counts by ONE workgroup, SELECT_THREADS
// counts per trip with a carry; the scatter, in which every workgroup repeats its count, scans its lanes' counts and writes
// its entries from its offset on — in ascending order whatever the order the workgroups run in.
template <int NT>
__device__ __forceinline__ uint32_t select_block_scan(uint32_t v, uint32_t* s, uint32_t& sum) {      // -> exclusive prefix of v
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const uint32_t add = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const uint32_t incl = s[t];
    sum = s[NT - 1];
    __syncthreads();
    return incl - v;
}
__global__ __launch_bounds__(SELECT_THREADS) void k_select_count(TrajSelectArgs sa) {
    __shared__ uint32_t s[SELECT_THREADS];
    const uint32_t base = (uint32_t)blockIdx.x * (uint32_t)SELECT_ELEMS + (uint32_t)threadIdx.x * 16u;
    uint32_t sum;
    select_block_scan<SELECT_THREADS>((uint32_t)__builtin_popcount(select_bits(sa, base)), s, sum);
    if (threadIdx.x == 0) sa.blocks[blockIdx.x] = (int32_t)sum;
}
__global__ __launch_bounds__(SELECT_THREADS) void k_select_scan(TrajSelectArgs sa) {
    __shared__ uint32_t s[SELECT_THREADS];
    uint32_t carry = 0u;
    for (int first = 0; first < sa.nblocks; first += SELECT_THREADS) {
        const int k = first + (int)threadIdx.x;
        uint32_t sum;
        const uint32_t excl = select_block_scan<SELECT_THREADS>(k < sa.nblocks ? (uint32_t)sa.blocks[k] : 0u, s, sum);
        if (k < sa.nblocks) sa.blocks[k] = (int32_t)(carry + excl);
        carry += sum;
    }
    if (threadIdx.x == 0) {
        sa.blocks[sa.nblocks] = (int32_t)carry;
        *sa.count = (int32_t)(sa.augment ? 2u * carry : carry);
    }
}
__global__ __launch_bounds__(SELECT_THREADS) void k_select_scatter(TrajSelectArgs sa) {
    __shared__ uint32_t s[SELECT_THREADS];
    const uint32_t base = (uint32_t)blockIdx.x * (uint32_t)SELECT_ELEMS + (uint32_t)threadIdx.x * 16u;
    const uint32_t bits = select_bits(sa, base);
    uint32_t sum;
    const uint32_t excl = select_block_scan<SELECT_THREADS>((uint32_t)__builtin_popcount(bits), s, sum);
    const long long k = (long long)(uint32_t)sa.blocks[sa.nblocks];
    select_emit(sa, base, bits, (long long)(uint32_t)sa.blocks[blockIdx.x] + excl, k);
    // the rest of d_index, up to cap: -1
    const long long step = (long long)gridDim.x * SELECT_THREADS;
    for (long long p = (sa.augment ? 2 * k : k) + (long long)blockIdx.x * SELECT_THREADS + threadIdx.x; p < sa.cap; p += step) sa.index[p] = -1;
}

// tetris_traj_batch_dev.  A workgroup of one wave takes BATCH_BLOCK consecutive samples of one slot (blockIdx.y): a lane reads
// its sample's record with three 16-byte loads — 48 contiguous bytes, one or two cache lines, wherever the index points — and
// expands the ten column words into its row of an LDS tile that is laid out as the workgroup's slice of `visual` itself (row
// pitch H * 10 bytes, not padded: rows start 50 / 55 words apart, at most two lanes per LDS bank while they are written, as in
// k_observe_packed).  The mirror image is the choice of the source column of every tile column — selects between registers,
// no second pass.  The tile leaves as 16-byte LDS reads -> 16-byte streaming stores, one contiguous run of 64 * H * 10 bytes
// (a multiple of 16 for every H); a slice of `visual` that does not start on 16 bytes leaves as dwords or bytes.  The slot-0
// workgroup also writes the samples' row entries.
__global__ __launch_bounds__(BATCH_BLOCK) void k_traj_batch(TrajBatchArgs ba) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tile[];      // BATCH_BLOCK * H * 10 bytes
    const int lane = threadIdx.x, sl = blockIdx.y, first = blockIdx.x * BATCH_BLOCK, j = first + lane;
    const int nb = imin(BATCH_BLOCK, ba.m - first), cells = ba.H * NCOL;
    if (j < ba.m) {
        const BatchEntry en = batch_entry(ba, j);
        const Quad* rec = reinterpret_cast<const Quad*>(ba.obs + ((size_t)en.at * ba.n_slots + sl) * OBS_WORDS);
        const Quad zero = {0u, 0u, 0u, 0u};
        const Quad a = en.valid ? rec[0] : zero, b = en.valid ? rec[1] : zero, c = en.valid ? rec[2] : zero;
        if (ba.visual) {
            const bool mi = en.mirror;
            uint32_t col[NCOL] = {mi ? c.y : a.x, mi ? c.x : a.y, mi ? b.w : a.z, mi ? b.z : a.w, mi ? b.y : b.x,
                                  mi ? b.x : b.y, mi ? a.w : b.z, mi ? a.z : b.w, mi ? a.y : c.x, mi ? a.x : c.y};
            if (ba.H % 2 == 0) obs_row_words(col, ba.H, s_tile + (size_t)lane * (cells / 4));
            else obs_row_halves(col, ba.H, reinterpret_cast<uint16_t*>(s_tile) + (size_t)lane * (cells / 2));
        }
        uint32_t v0, v1, v2, piece;
        batch_scalars(en, c.z, c.w, v0, v1, v2, piece);
        batch_store_vector(ba, sl, j, v0, v1, v2, piece);
        if (sl == 0) batch_store_entry(ba, j, en);
    }
    if (!ba.visual) return;
    __syncthreads();
    uint8_t* out = ba.visual + ((size_t)sl * ba.m + first) * (size_t)cells;
    const uint32_t bytes = (uint32_t)nb * (uint32_t)cells;
    const uint8_t* tile = reinterpret_cast<const uint8_t*>(s_tile);
    uint32_t done = 0u;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if ((((uintptr_t)out) & 15u) == 0) {
        done = bytes & ~15u;
        for (uint32_t k = 16u * (uint32_t)lane; k < done; k += 16u * BATCH_BLOCK)
            __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(tile + k), reinterpret_cast<u32x4*>(out + k));
    } else if ((((uintptr_t)out) & 3u) == 0) {
        done = bytes & ~3u;
        for (uint32_t k = 4u * (uint32_t)lane; k < done; k += 4u * BATCH_BLOCK)
            *reinterpret_cast<uint32_t*>(out + k) = *reinterpret_cast<const uint32_t*>(tile + k);
    }
    for (uint32_t k = done + (uint32_t)lane; k < bytes; k += BATCH_BLOCK) out[k] = tile[k];
}

// ---- the planning agent's windows (tetris_plan_traj.h)
// tetris_traj_record_plan_dev.  A workgroup takes PLAN_RECORD_GAMES = G consecutive games (S = threads / G slices):
//   a. lane t < G: player, count, choice and the row's scalar arrays; `before` of the G games from the observation records
//      (48-byte runs, 48 P bytes apart) into LDS, column-major [10][G];
//   b. thread = (game, slice): lists k = s, s + S, ..: ten independent column loads, coalesced over the games of a slice (d_cols
//      is game-minor), the popcounts against `before`, the kind into an LDS byte [L][G];
//   c. thread = (game, column): the nine bit-sliced counters over the NORMAL lists — the loop of k_plan_choose's phase E, its
//      loads coalesced over games again and served by L2 — the counts of the kinds, the chosen list's word, and all of it into an
//      LDS image of the G records;
//   d. the G records are G x 448 contiguous bytes of the window's row: 16-byte LDS reads -> 16-byte stores in memory order.
// The LDS image has a pitch of PLAN_REC_PITCH = 116 words per record: a multiple of four, so the 16-byte reads of (d) stay
// aligned, and 4 x 29, so the 32 games of a lane group, which write the same word of their records in (c), spread over eight
// banks instead of the two a pitch of 112 gives.  LDS: 14.5 KB of records, 1.25 KB of `before`, L G bytes of kinds (8 KB at 256
// lists).  No workgroup waits for another.
constexpr int PLAN_REC_PITCH = PLAN_REC_WORDS + 4;
static_assert(PLAN_RECORD_THREADS % PLAN_RECORD_GAMES == 0 && PLAN_RECORD_GAMES <= 64, "whole slices of G lanes");
__host__ __device__ constexpr size_t plan_record_lds_bytes(int L) {
    return ((size_t)PLAN_RECORD_GAMES * PLAN_REC_PITCH + (size_t)(NCOL + 3) * PLAN_RECORD_GAMES) * 4 + (size_t)L * PLAN_RECORD_GAMES;
}
__global__ __launch_bounds__(PLAN_RECORD_THREADS) void k_traj_record_plan(PlanRecordArgs ra) {
    extern __shared__ __attribute__((aligned(16))) uint32_t plan_record_lds[];
    constexpr int G = PLAN_RECORD_GAMES, S = PLAN_RECORD_THREADS / G;
    uint32_t* s_rec = plan_record_lds;                                   // [G][PLAN_REC_PITCH]
    uint32_t* s_before = s_rec + G * PLAN_REC_PITCH;                     // [10][G]
    int* s_player = reinterpret_cast<int*>(s_before + NCOL * G);         // [G] each
    int *s_count = s_player + G, *s_choice = s_count + G;
    uint8_t* s_kind = reinterpret_cast<uint8_t*>(s_choice + G);          // [L][G]
    const int t = (int)threadIdx.x, g0 = (int)blockIdx.x * G, ng = imin(G, ra.n - g0);
    const int P = ra.n_players, L = ra.max_lists;
    const size_t n = (size_t)ra.n;
    const bool packed = ra.rec != nullptr;
    if (t < ng) {                                                                        // a
        const int i = g0 + t, p = safe_player(ra.player, i, P);
        const int count = packed ? plan_clamp_count(ra.count[i], L) : 0;
        const int choice = packed ? plan_record_choice(ra.choice[i], count) : ra.choice[i];
        s_player[t] = p; s_count[t] = count; s_choice[t] = choice;
        plan_record_row(ra, i, p, choice);
    }
    if (!packed) return;
    const uint32_t mask = plan_row_mask(ra.H);
    for (int u = t; u < ng * NCOL; u += PLAN_RECORD_THREADS) {
        const int g = u / NCOL, c = u - g * NCOL;
        s_before[c * G + g] = ra.obs[(size_t)(g0 + g) * P * OBS_WORDS + c] & mask;
    }
    __syncthreads();
    {                                                                                   // b
        const int g = t % G, s = t / G, i = g0 + g;
        if (g < ng) {
            const int p = s_player[g], count = s_count[g];
            uint32_t before[NCOL];
            TE_UNROLL
            for (int c = 0; c < NCOL; c++) before[c] = s_before[c * G + g];
            for (int k = s; k < count; k += S) {
                const uint32_t* src = ra.cols + ((size_t)k * P + p) * NCOL * n + i;
                uint32_t after[NCOL];
                TE_UNROLL
                for (int c = 0; c < NCOL; c++) after[c] = src[(size_t)c * n] & mask;
                s_kind[k * G + g] = (uint8_t)plan_list_kind(k, count, plan_list_sum(after, before));
            }
        }
    }
    __syncthreads();
    for (int u = t; u < NCOL * G; u += PLAN_RECORD_THREADS) {                            // c
        const int g = u % G, c = u / G, i = g0 + g;
        if (g >= ng) continue;
        const int p = s_player[g], count = s_count[g], choice = s_choice[g];
        const uint32_t* src = ra.cols + ((size_t)p * NCOL + c) * n + i;
        const size_t step = (size_t)P * NCOL * n;
        uint32_t plane[CHOOSE_COUNT_PLANES];
        TE_UNROLL
        for (int j = 0; j < CHOOSE_COUNT_PLANES; j++) plane[j] = 0u;
        int n_small = 0, n_normal = 0;
#pragma unroll 4
        for (int k = 0; k < count; k++) {
            const uint32_t word = src[(size_t)k * step] & mask;
            const int kind = s_kind[k * G + g];
            n_small += kind == PLAN_LIST_SMALL;
            n_normal += kind == PLAN_LIST_NORMAL;
            plan_count_add(plane, kind == PLAN_LIST_NORMAL ? word : 0u);
        }
        const int kind = count > 0 ? (int)s_kind[choice * G + g] : (int)PLAN_LIST_PAST;
        uint32_t aw = 0u;
        if (kind == PLAN_LIST_NORMAL) aw = src[(size_t)choice * step] & mask;
        uint32_t* r = s_rec + g * PLAN_REC_PITCH;
        r[PLAN_REC_BEFORE + c] = s_before[c * G + g];
        r[PLAN_REC_AFTER + c] = aw;
        TE_UNROLL
        for (int j = 0; j < CHOOSE_COUNT_PLANES; j++) r[PLAN_REC_PLANES + CHOOSE_COUNT_PLANES * c + j] = plane[j];
        if (c == 0) {
            r[PLAN_REC_KIND] = (uint32_t)kind;
            r[PLAN_REC_COUNTS] = (uint32_t)n_small | ((uint32_t)n_normal << 16);
        }
    }
    __syncthreads();
    Quad* out = reinterpret_cast<Quad*>(ra.rec + (size_t)g0 * PLAN_REC_WORDS);           // d
    for (int e = t; e < ng * PLAN_REC_QUADS; e += PLAN_RECORD_THREADS) {
        const int g = e / PLAN_REC_QUADS, q = e - g * PLAN_REC_QUADS;
        out[e] = *reinterpret_cast<const Quad*>(s_rec + g * PLAN_REC_PITCH + 4 * q);
    }
}

// tetris_traj_plan_batch_dev.  A workgroup takes PLAN_BATCH_SAMPLES consecutive samples: a multiple of 8, so its run of either
// output starts on 16 bytes for every H and both element types.  The records are gathered with 16-byte loads, 28 consecutive
// lanes per sample — 448 contiguous bytes wherever the index points; a sample that names no entry becomes a record of zeros,
// which expands to zeros — into an LDS image [samples][112].  Then every thread builds 16 bytes of consecutive output elements
// from LDS, walking (sample, row, column) along without a division per element, and streams them out: a wave instruction
// stores 1 KB contiguous, d_delta first, then d_sums.  The mirror is the choice of the record's column.  Lanes of a group read
// at most ten distinct record words at a time (five columns of two samples: their banks differ); equal addresses broadcast.
// The tail of a last, short workgroup whose run is no multiple of 16 bytes leaves element by element.
struct PlanBatchShared {
    alignas(16) uint32_t rec[PLAN_BATCH_SAMPLES * PLAN_REC_WORDS];
    uint32_t mirror[PLAN_BATCH_SAMPLES];
};
template <bool SUMS>
__device__ __forceinline__ float plan_batch_cell(const uint32_t* r, bool mirror, int y, int c, float small_fill) {
    return SUMS ? plan_rec_sums(r, mirror, y, c, small_fill) : plan_rec_delta(r, mirror, y, c, small_fill);
}
template <typename T, bool SUMS>
__device__ __forceinline__ void plan_batch_store(const PlanBatchArgs& ba, const PlanBatchShared& sh, int first, int nb, void* plane_out) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int EPV = 16 / (int)sizeof(T);
    const int H = ba.H, HW = H * NCOL;
    const uint32_t total = (uint32_t)nb * (uint32_t)HW;
    T* out = (T*)plane_out + (size_t)first * HW;
    for (uint32_t e0 = (uint32_t)threadIdx.x * EPV; e0 < total; e0 += (uint32_t)PLAN_BATCH_THREADS * EPV) {
        int j = (int)(e0 / (uint32_t)HW);
        const int cell = (int)(e0 - (uint32_t)j * (uint32_t)HW);
        int y = cell / NCOL, c = cell - y * NCOL;
        T v[EPV];
        TE_UNROLL
        for (int q = 0; q < EPV; q++) {
            v[q] = plan_encode<T>(0.0f);
            if (e0 + (uint32_t)q < total) v[q] = plan_encode<T>(plan_batch_cell<SUMS>(sh.rec + j * PLAN_REC_WORDS, sh.mirror[j] != 0u, y, c, ba.small_fill));
            c++;
            if (c == NCOL) { c = 0; y++; }
            if (y == H) { y = 0; j++; }
        }
        if (e0 + EPV <= total) {
            u32x4 w;
            w.x = pd_pack(v, 0); w.y = pd_pack(v, 1); w.z = pd_pack(v, 2); w.w = pd_pack(v, 3);
            __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(out + e0));
        } else {
            TE_UNROLL
            for (int q = 0; q < EPV; q++)
                if (e0 + (uint32_t)q < total) out[e0 + q] = v[q];
        }
    }
}
template <typename T>
__global__ __launch_bounds__(PLAN_BATCH_THREADS) void k_traj_plan_batch(PlanBatchArgs ba) {
    __shared__ PlanBatchShared sh;
    const int t = (int)threadIdx.x, first = (int)blockIdx.x * PLAN_BATCH_SAMPLES, nb = imin(PLAN_BATCH_SAMPLES, ba.m - first);
    for (int e = t; e < nb * PLAN_REC_QUADS; e += PLAN_BATCH_THREADS) {
        const int j = e / PLAN_REC_QUADS, q = e - j * PLAN_REC_QUADS;
        const BatchEntry en = plan_batch_entry(ba, first + j);
        // (an entry that names no sample has at = 0: entry 0 is loaded and dropped word by word — a select between a loaded
        // aggregate and a constant one would go through scratch)
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 w = reinterpret_cast<const u32x4*>(ba.rec + (size_t)en.at * PLAN_REC_WORDS)[q];
        const uint32_t keep = en.valid ? ~0u : 0u;
        w.x &= keep; w.y &= keep; w.z &= keep; w.w &= keep;
        *reinterpret_cast<u32x4*>(sh.rec + j * PLAN_REC_WORDS + 4 * q) = w;
        if (q == 0) sh.mirror[j] = en.mirror ? 1u : 0u;
    }
    __syncthreads();
    if (ba.delta) plan_batch_store<T, false>(ba, sh, first, nb, ba.delta);
    if (ba.sums) plan_batch_store<T, true>(ba, sh, first, nb, ba.sums);
}

// ---- experience replay (tetris_replay.h)
// tetris_replay_add_dev in three launches, none of which waits for another workgroup: a lane per game counts its mask bytes
// (row t of the mask is read by consecutive lanes); ONE workgroup scans the N counts, SELECT_THREADS per trip with a carry, and
// applies the cursor rule; a lane per game copies its run.  The window is read as it lies — consecutive lanes read consecutive
// 48 S-byte records and row entries of a row t — and a lane writes a run of consecutive ring positions of its own.
constexpr int REPLAY_THREADS = 256;      // the replay kernels that are a lane per game, position, sorted slot or output
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_add_count(ReplayAddArgs aa) {
    const int g = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (g < aa.n) aa.offsets[g] = replay_add_count(aa, g) * (aa.augment ? 2u : 1u);
}
__global__ __launch_bounds__(SELECT_THREADS) void k_replay_add_scan(ReplayAddArgs aa) {
    __shared__ uint32_t s[SELECT_THREADS];
    uint32_t carry = 0u;
    for (int first = 0; first < aa.n; first += SELECT_THREADS) {
        const int g = first + (int)threadIdx.x;
        uint32_t sum;
        const uint32_t excl = select_block_scan<SELECT_THREADS>(g < aa.n ? aa.offsets[g] : 0u, s, sum);
        if (g < aa.n) aa.offsets[g] = carry + excl;
        carry += sum;
    }
    if (threadIdx.x == 0) aa.offsets[aa.n] = replay_cursor_rule(aa.rp.cursor, carry, (uint32_t)aa.rp.max_size);
}
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_add_scatter(ReplayAddArgs aa) {
    const int g = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (g < aa.n) replay_add_game(aa, g);
}

// tetris_replay_sample_dev around its two sorts: a lane per position / sorted slot / output
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_prio_keys(ReplaySampleArgs sa) {
    const uint32_t i = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (i < sa.max_size) replay_prio_key(sa, i);
}
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_sample_keys(ReplaySampleArgs sa) {
    const uint32_t s = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (s < sa.max_size) replay_sample_key(sa, s);
}
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_emit(ReplaySampleArgs sa) {
    const int j = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (j < sa.m || j == 0) {
        if (sa.m == 0) sa.count[0] = 0;
        else replay_emit(sa, j);
    }
}
__global__ __launch_bounds__(REPLAY_THREADS) void k_replay_update(ReplayUpdateArgs ua) {
    const int j = blockIdx.x * REPLAY_THREADS + threadIdx.x;
    if (j < ua.m) replay_update(ua, j);
}

// One pass of the stable LSD radix sort in three launches, none of which waits for another workgroup (no look-back, no grid
// barrier): the digit counts of every tile of SORT_TILE entries (LDS atomics), digit-major; a workgroup per digit scans its row
// of tile counts, SORT_SCAN_SPAN per trip with a carry, and leaves the digit's total; the scatter.  In the scatter wave w of a
// tile holds entries [512 w, 512 w + 512) in eight rounds of 64 consecutive ones.  A lane's rank among the entries of its digit
// in its wave is the wave's counter of the digit so far (LDS, one row of counters per wave) plus the lanes below it of the
// round with the same digit: eight ballots, one per bit of the digit, leave the mask of those lanes.  Then thread d turns the
// four waves' counters of digit d into their places in the tile's new order — (digits below d in the tile: a scan of the tile's
// counts) + (digit d in the waves before) — the tile is put into that order in LDS, and leaves from there: entry `at` of the
// new order goes to (digits below d: a scan of the totals) + (digit d in the tiles before) + (its place in d's run), so
// consecutive lanes write consecutive words of a run.  The order is tile, wave, round, lane = position in the input: the pass
// is stable.
static_assert(SORT_THREADS == SORT_RADIX && SORT_THREADS == 4 * 64, "four waves; a thread per digit");
__global__ __launch_bounds__(SORT_THREADS) void k_sort_histogram(SortArgs sa) {
    __shared__ uint32_t cnt[SORT_RADIX];
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t first = (uint32_t)blockIdx.x * SORT_TILE;
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; r++) {
        const uint32_t e = first + (uint32_t)r * SORT_THREADS + threadIdx.x;
        if (e < sa.total) atomicAdd(&cnt[sort_digit(sa.key_in[e], sa.pass)], 1u);
    }
    __syncthreads();
    sa.hist[(size_t)threadIdx.x * sa.ntiles + blockIdx.x] = cnt[threadIdx.x];
}
__global__ __launch_bounds__(SORT_SCAN_SPAN) void k_sort_scan(SortArgs sa) {      // (a tile per thread and trip)
    __shared__ uint32_t s[SORT_SCAN_SPAN];
    uint32_t* row = sa.hist + (size_t)blockIdx.x * sa.ntiles;
    uint32_t carry = 0u;
    for (int first = 0; first < sa.ntiles; first += SORT_SCAN_SPAN) {
        const int t = first + (int)threadIdx.x;
        uint32_t sum;
        const uint32_t excl = select_block_scan<SORT_SCAN_SPAN>(t < sa.ntiles ? row[t] : 0u, s, sum);
        if (t < sa.ntiles) row[t] = carry + excl;
        carry += sum;
    }
    if (threadIdx.x == 0) sa.totals[blockIdx.x] = carry;
}
__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(SortArgs sa) {
    __shared__ uint32_t wcnt[SORT_THREADS / 64][SORT_RADIX];
    __shared__ uint32_t s[SORT_THREADS], gbase[SORT_RADIX];
    __shared__ uint32_t lkey[SORT_TILE], lpos[SORT_TILE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#pragma unroll
    for (int w = 0; w < SORT_THREADS / 64; w++) wcnt[w][threadIdx.x] = 0u;
    uint32_t sum;
    const uint32_t below = select_block_scan<SORT_THREADS>(sa.totals[threadIdx.x], s, sum);      // (its barriers cover the zeroing)
    const uint32_t first = (uint32_t)blockIdx.x * SORT_TILE + (uint32_t)wave * (SORT_ITEMS * 64) + (uint32_t)lane;
    const uint64_t lower = (1ull << lane) - 1ull;
    uint32_t key[SORT_ITEMS], pos[SORT_ITEMS], rank[SORT_ITEMS];
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; r++) {
        const uint32_t e = first + (uint32_t)r * 64u;
        const bool live = e < sa.total;
        key[r] = live ? sa.key_in[e] : 0u;
        pos[r] = live ? sa.pos_in[e] : 0u;
        const uint32_t d = sort_digit(key[r], sa.pass);
        uint64_t same = __ballot(live);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const uint64_t set = __ballot(live && ((d >> bit) & 1u));
            same &= ((d >> bit) & 1u) ? set : ~set;
        }
        // (volatile: the lanes of a wave hand the counter on from round to round without a barrier; a wave's LDS accesses
        // complete in the order they are issued)
        volatile uint32_t* counter = &wcnt[wave][d];
        const uint32_t before = live ? *counter : 0u;
        rank[r] = before + (uint32_t)__builtin_popcountll(same & lower);
        __builtin_amdgcn_wave_barrier();                                        // every lane has read the counter
        if (live && (same & lower) == 0ull) *counter = before + (uint32_t)__builtin_popcountll(same);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // thread d: digit d's place in the tile (a scan of the tile's counts), the waves' shares of it, and where it goes
        const int d = threadIdx.x;
        uint32_t c[SORT_THREADS / 64], cd = 0u;
#pragma unroll
        for (int w = 0; w < SORT_THREADS / 64; w++) { c[w] = wcnt[w][d]; cd += c[w]; }
        const uint32_t local = select_block_scan<SORT_THREADS>(cd, s, sum);
        uint32_t at = local;
#pragma unroll
        for (int w = 0; w < SORT_THREADS / 64; w++) { wcnt[w][d] = at; at += c[w]; }
        gbase[d] = below + sa.hist[(size_t)d * sa.ntiles + blockIdx.x] - local;
    }
    __syncthreads();
    // the tile in its new order, in LDS: consecutive lanes then write consecutive entries of a digit's run
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; r++) {
        const uint32_t e = first + (uint32_t)r * 64u;
        if (e < sa.total) {
            const uint32_t at = wcnt[wave][sort_digit(key[r], sa.pass)] + rank[r];
            if (at < (uint32_t)SORT_TILE) { lkey[at] = key[r]; lpos[at] = pos[r]; }
        }
    }
    __syncthreads();
    const uint32_t tile_first = (uint32_t)blockIdx.x * SORT_TILE;
    const uint32_t live = sa.total - tile_first < (uint32_t)SORT_TILE ? sa.total - tile_first : (uint32_t)SORT_TILE;
#pragma unroll
    for (int r = 0; r < SORT_ITEMS; r++) {
        const uint32_t at = (uint32_t)r * SORT_THREADS + threadIdx.x;
        if (at < live) {
            const uint32_t k = lkey[at], dst = gbase[sort_digit(k, sa.pass)] + at;
            if (dst < sa.total) { sa.key_out[dst] = k; sa.pos_out[dst] = lpos[at]; }
        }
    }
}
