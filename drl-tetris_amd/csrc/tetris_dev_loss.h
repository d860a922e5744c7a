// Kernels of libtetris_hip.so, part 6: the trainers' loss heads and the planning agent's (bodies: tetris_loss.h).  Needs
// tetris_dev_vec.h and tetris_dev_act.h (ActShared, act_gather).

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

// The opposite direction of act_gather: the block's ng x 40 K gradient elements, 16 bytes per lane and store.  The elements of
// a sample's piece are sh.m[candidate][sample], all others zero.
template <int NT, int K, bool F16>
__device__ __forceinline__ void loss_scatter(void* grad, int g0, int ng, const ActShared& sh) {
    constexpr int EPV = F16 ? 8 : 4, PER = ACT_CANDIDATES * K;
    static_assert(PER % EPV == 0, "a 16-byte vector must not cross two samples");
    u32x4* dst = (u32x4*)((char*)grad + (size_t)g0 * PER * (F16 ? 2 : 4));
    const int nvec = ng * (PER / EPV);
#pragma unroll 4
    for (int v = threadIdx.x; v < nvec; v += NT) {
        const int e0 = v * EPV, s = e0 / PER, rem = e0 - s * PER;
        u32x4 q = {0u, 0u, 0u, 0u};
        if (K == 1) {
#pragma unroll
            for (int j = 0; j < EPV; j++) vec_put<F16>(q, j, sh.m[(rem + j) * ACT_LDS_STRIDE + s]);
        } else {
            int j = sh.piece[s] - rem % K;                    // the first element of the vector that belongs to the piece
            j = j < 0 ? j + K : j;
            if (j < EPV) vec_put<F16>(q, j, sh.m[((rem + j) / K) * ACT_LDS_STRIDE + s]);
            if (EPV > K && j + K < EPV) vec_put<F16>(q, j + K, sh.m[((rem + j + K) / K) * ACT_LDS_STRIDE + s]);
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
    const bool in_f16 = la.in_f16 != 0;      // (this kernel's two ladders stay written out: through vec_with_k_f16 its code moved)
    if (la.K == 7) {
        if (in_f16) act_gather<LOSS_THREADS, 7, true>(la.x, g0, ng, sh.act); else act_gather<LOSS_THREADS, 7, false>(la.x, g0, ng, sh.act);
    } else {
        if (in_f16) act_gather<LOSS_THREADS, 1, true>(la.x, g0, ng, sh.act); else act_gather<LOSS_THREADS, 1, false>(la.x, g0, ng, sh.act);
    }
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
    u32x4* run = (u32x4*)((char*)whole + (size_t)g0 * PER * (F16 ? 2 : 4));
#pragma unroll 2
    for (uint32_t v = threadIdx.x; v < nvec; v += PLAN_LOSS_THREADS) {
        u32x4 q = {0u, 0u, 0u, 0u};
        if (!PUT) q = run[v];
        const uint32_t e0 = v * EPV;
        uint32_t s = e0 / PER, rem = e0 - s * PER;
        uint32_t cell = rem / K, kk = rem - cell * K;
#pragma unroll
        for (int j = 0; j < (int)EPV; j++) {
            if ((int)kk == sh.piece[s]) {
                if (PUT) vec_put<F16>(q, j, sh.x[s * PLAN_LOSS_PITCH + cell]);
                else sh.x[s * PLAN_LOSS_PITCH + cell] = vec_element<F16>(q, j, act_f16_to_f32);
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
    vec_with_k_f16(la.K, la.in_f16 != 0, [](auto K, auto F16, auto&&... a) { plan_loss_stream<K(), F16(), false>(a...); }, la, g0, ng, sh);      // b
    for (int e = t; e < ng * PLAN_REC_QUADS; e += PLAN_LOSS_THREADS) {
        const int j = e / PLAN_REC_QUADS, q = e - j * PLAN_REC_QUADS;
        const BatchEntry en = batch_index_entry((uint32_t)la.index[g0 + j], la.total);
        // (an entry that names no sample has at = 0: entry 0 is loaded and dropped word by word, as in k_traj_plan_batch)
        u32x4 w = reinterpret_cast<const u32x4*>(la.rec + (size_t)en.at * PLAN_REC_WORDS)[q];
        const uint32_t keep = en.valid ? ~0u : 0u;
        w.x &= keep; w.y &= keep; w.z &= keep; w.w &= keep;
        *reinterpret_cast<u32x4*>(sh.rec + j * PLAN_REC_WORDS + 4 * q) = w;
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
    vec_with_k_f16(la.K, la.grad_f16 != 0, [](auto K, auto F16, auto&&... a) { plan_loss_stream<K(), F16(), true>(a...); }, la, g0, ng, sh);     // d
    for (int e = t; e < ng * la.V; e += PLAN_LOSS_THREADS) {
        const int s = e / la.V, kk = e - s * la.V;
        loss_store(la.grad_v, (size_t)g0 * la.V + e, kk == imin(sh.piece[s], la.V - 1) ? sh.gv[s] : 0.0f, la.grad_f16);
    }
}
