// Kernels of libtetris_hip.so, part 4: the planning and policy half of tetris_lib_agent.h: a planning agent's action lists, its
// afterstate deltas and its choice from phi, and the heuristic policy's evaluation and pick.  (The planning and policy STEP kernels
// are compiled for every player count and live in tetris_game_kernel.h.)  Needs tetris_dev_vec.h.

// tetris_action_lists_dev: the slabs k_actions wrote for games g0 .. g0 + m - 1 -> the caller's [N][L][K] lists, one wave per
// game (plan_compact_serial is the serial form of the same steps): prefix sum of the 40 slab counts in the reference's order,
// every raw list hashed into LDS, each lane tests its lists against all earlier ones (hash first), ballots give the output
// positions.  Nothing is written for a game that does not fit (count -1, F_LISTS).
__global__ __launch_bounds__(64) void k_plan_lists(const uint8_t* cnt, const uint8_t* slab_lens, const uint8_t* slab_keys, int KS, int g0,
                                                   int L, int K, int keep_null, int32_t* count, uint8_t* lens, uint8_t* keys,
                                                   uint32_t* status) {
    __shared__ int s_off[41];
    __shared__ uint32_t s_hash[PLAN_RAW_MAX];
    __shared__ uint16_t s_src[PLAN_RAW_MAX];           // slab entry of raw list m: (r * 10 + xi) * PLAN_LANE_LISTS + list
    __shared__ uint8_t s_len[PLAN_RAW_MAX];
    __shared__ uint8_t s_keep[PLAN_RAW_MAX];
    const int lane = threadIdx.x;
    const size_t t0 = (size_t)blockIdx.x * 40, g = (size_t)g0 + blockIdx.x;
    const uint8_t* gkeys = slab_keys + t0 * PLAN_LANE_LISTS * (size_t)KS;
    int c = lane < 40 ? cnt[t0 + plan_slab_lane(lane)] : 0;
    const bool over = c > PLAN_LANE_LISTS;
    if (over) c = 0;
    int incl = c;
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    if (lane < 40) s_off[lane] = incl - c;
    if (lane == 39) s_off[40] = incl;
    bool bad = __ballot(over) != 0;
    __syncthreads();
    const int M = s_off[40];
    bool my_bad = false, my_null = false;
    for (int m = lane; m < M; m += 64) {
        int lo = 0, hi = 40;                           // s_off[lo] <= m < s_off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= m) lo = mid; else hi = mid;
        }
        const int src = plan_slab_lane(lo) * PLAN_LANE_LISTS + (m - s_off[lo]);
        const int len = slab_lens[t0 * PLAN_LANE_LISTS + src];
        const uint8_t* k = gkeys + (size_t)src * KS;
        my_bad |= len > K;
        my_null |= plan_is_null(k, len);
        s_hash[m] = plan_list_hash(k, len);
        s_src[m] = (uint16_t)src;
        s_len[m] = (uint8_t)len;
    }
    bad |= __ballot(my_bad) != 0;
    const bool has_null = __ballot(my_null) != 0;
    __syncthreads();
    int n_sel = 0;
    for (int base = 0; base < M && !bad; base += 64) {     // (bad and M are uniform)
        const int m = base + lane;
        bool sel = false;
        if (m < M) {
            const int len = s_len[m];
            const uint32_t h = s_hash[m];
            const uint8_t* k = gkeys + (size_t)s_src[m] * KS;
            sel = keep_null || !plan_is_null(k, len);
            for (int e = 0; e < m && sel; e++)
                if (s_hash[e] == h && s_len[e] == len && plan_same_list(k, len, gkeys + (size_t)s_src[e] * KS, len)) sel = false;
            s_keep[m] = (uint8_t)sel;
        }
        n_sel += __popcll(__ballot(sel));
    }
    const int o0 = (!keep_null || has_null) ? 0 : 1;
    const int n_out = (o0 + n_sel) ? o0 + n_sel : 1;
    if (bad || n_out > L) {
        if (lane == 0) { count[g] = -1; plan_report_overflow(status); }
        return;
    }
    int o = o0;
    for (int base = 0; base < M; base += 64) {
        const int m = base + lane;
        const bool sel = m < M && s_keep[m];
        const unsigned long long bal = __ballot(sel);
        if (sel) plan_write_list(lens, keys, g, L, K, o + __popcll(bal & __lanemask_lt()), gkeys + (size_t)s_src[m] * KS, s_len[m]);
        o += __popcll(bal);
    }
    if (lane == 0) {
        if (o0 || !n_sel) plan_write_null(lens, keys, g, L, K);
        count[g] = n_out;
    }
}

// tetris_plan_deltas_dev: one workgroup per game, list k = thread k (L <= 256 = PD_BLOCK).  The output of a game is one contiguous
// run of H * 10 * L elements in either layout and is what the kernel costs (64 lists of a 20-row board: 51 KB of float32 against
// 2.5 KB of column words), so everything is arranged around its stores:
//   1. thread k gathers its list's ten column words (a stride of P * 10 * N words between threads: every word its own cache line,
//      shared with the 15 neighbouring games), applies the small rule on popcounts and leaves the words (zero unless the list is
//      normal) and the list's kind in LDS; the field before is the same for all threads (uniform loads);
//   2. the deltas: a thread builds 16 bytes of consecutive output elements from LDS and streams them out, so a wave instruction
//      stores 1 KB contiguous — lists-last: 4 (binary16: 8) lists of one cell from one 16-byte LDS read; list-major: consecutive
//      cells of one list.  Shapes whose inner extent is no multiple of that take one element per thread, still consecutive;
//   3. the sums: thread = cell, the integer count of set bits over the LDS rows, then plan_sums_value.
// Games are dealt to workgroups so that the 16 games sharing the cache lines of d_cols run on one XCD (workgroups go round-robin
// over the 8 XCDs, each with an L2 of its own): workgroup 8 m + x takes game ((m / 16) * 8 + x) * 16 + m % 16.  Only speed
// depends on that placement.
constexpr int PD_BLOCK = 256;
constexpr int PD_LS = PD_BLOCK + 4;     // words per LDS row: the ten rows start in ten different 16-byte slots

__device__ __forceinline__ uint32_t pd_pack(const float* v, int w) { return f2u(v[w]); }
__device__ __forceinline__ uint32_t pd_pack(const uint16_t* v, int w) { return (uint32_t)v[2 * w] | ((uint32_t)v[2 * w + 1] << 16); }

// the element of (list kind, column word, before bit b, row y): plan_delta_value over its four possible values, encoded once
// (passed by value: selecting between members of a struct in memory becomes a load from a selected address, i.e. scratch)
template <typename T>
__device__ __forceinline__ T pd_element(T v_fill, T v_zero, T v_one, T v_mone, int kind, uint32_t after, uint32_t b, int y) {
    const uint32_t a = (after >> y) & 1u;
    const T dv = a > b ? v_one : a < b ? v_mone : v_zero;
    return kind == PLAN_LIST_NORMAL ? dv : kind == PLAN_LIST_SMALL ? v_fill : v_zero;
}

template <typename T, bool LIST_MAJOR>
__global__ __launch_bounds__(PD_BLOCK) void k_plan_deltas(PlanDeltaArgs da) {
    constexpr int EPL = 16 / (int)sizeof(T);                  // elements of one 16-byte store
    __shared__ __attribute__((aligned(16))) uint32_t s_after[NCOL * PD_LS];
    __shared__ __attribute__((aligned(16))) uint8_t s_kind[PD_BLOCK];
    __shared__ uint32_t s_before[NCOL];
    const uint32_t m = blockIdx.x >> 3;
    const int i = (int)((((m >> 4) * 8u + (blockIdx.x & 7u)) << 4) + (m & 15u));
    if (i >= da.n) return;
    const int tid = (int)threadIdx.x, L = da.max_lists, H = da.H, HW = H * NCOL, P = da.geo.P;
    const int p = safe_player(da.player, i, P);
    const int count = plan_clamp_count(da.count[i], L);
    const uint32_t mask = plan_row_mask(H);
    const Ref br = board_ref(da.geo, p, (size_t)i);
    {
        uint32_t before[NCOL], after[NCOL];
        TE_UNROLL
        for (int c = 0; c < NCOL; c++) {
            before[c] = word_at(br, W_COL0 + c) & mask;
            after[c] = 0;
        }
        if (tid < count) {
            const uint32_t* src = da.cols + ((size_t)tid * P + p) * NCOL * (size_t)da.n + i;
            TE_UNROLL
            for (int c = 0; c < NCOL; c++) after[c] = src[(size_t)c * da.n] & mask;
        }
        const int kind = plan_list_kind(tid, count, plan_list_sum(after, before));
        TE_UNROLL
        for (int c = 0; c < NCOL; c++) s_after[c * PD_LS + tid] = kind == PLAN_LIST_NORMAL ? after[c] : 0u;
        s_kind[tid] = (uint8_t)kind;
        if (tid < NCOL) s_before[tid] = word_at(br, W_COL0 + tid) & mask;
        if (da.small && tid < L) da.small[(size_t)i * L + tid] = (uint8_t)(kind == PLAN_LIST_SMALL);
    }
    const int n_small = __syncthreads_count(s_kind[tid] == PLAN_LIST_SMALL);
    const int n_normal = __syncthreads_count(s_kind[tid] == PLAN_LIST_NORMAL);

    const float fill = da.small_fill;
    const T v_fill = plan_encode<T>(plan_delta_value(PLAN_LIST_SMALL, 0, fill));
    const T v_zero = plan_encode<T>(plan_delta_value(PLAN_LIST_NORMAL, 0, fill));
    const T v_one = plan_encode<T>(plan_delta_value(PLAN_LIST_NORMAL, 1, fill));
    const T v_mone = plan_encode<T>(plan_delta_value(PLAN_LIST_NORMAL, -1, fill));
    T* out = (T*)da.deltas + (size_t)i * HW * L;
    const int inner = LIST_MAJOR ? HW : L, outer_n = LIST_MAJOR ? L : HW;
    if (inner % EPL == 0) {
        // unit u = 16 bytes: (outer, in) = (u / LG, u % LG), stepped without a division
        const uint32_t LG = (uint32_t)(inner / EPL), units = (uint32_t)outer_n * LG;
        const uint32_t d_outer = PD_BLOCK / LG, d_in = PD_BLOCK % LG;
        uint32_t outer = (uint32_t)tid / LG, in = (uint32_t)tid % LG;
        for (uint32_t u = (uint32_t)tid; u < units; u += PD_BLOCK) {
            T v[EPL];
            if (!LIST_MAJOR) {
                const int y = (int)outer / NCOL, c = (int)outer - y * NCOL, k0 = (int)in * EPL;
                const uint32_t b = (s_before[c] >> y) & 1u;
                TE_UNROLL
                for (int q = 0; q < EPL / 4; q++) {
                    const u32x4 a4 = *reinterpret_cast<const u32x4*>(&s_after[c * PD_LS + k0 + 4 * q]);
                    const uint32_t k4 = *reinterpret_cast<const uint32_t*>(&s_kind[k0 + 4 * q]);
                    v[4 * q + 0] = pd_element(v_fill, v_zero, v_one, v_mone, (int)(k4 & 255u), a4.x, b, y);
                    v[4 * q + 1] = pd_element(v_fill, v_zero, v_one, v_mone, (int)((k4 >> 8) & 255u), a4.y, b, y);
                    v[4 * q + 2] = pd_element(v_fill, v_zero, v_one, v_mone, (int)((k4 >> 16) & 255u), a4.z, b, y);
                    v[4 * q + 3] = pd_element(v_fill, v_zero, v_one, v_mone, (int)(k4 >> 24), a4.w, b, y);
                }
            } else {
                const int k = (int)outer, kind = s_kind[k], cell0 = (int)in * EPL;
                TE_UNROLL
                for (int j = 0; j < EPL; j++) {
                    const int y = (cell0 + j) / NCOL, c = (cell0 + j) - y * NCOL;
                    v[j] = pd_element(v_fill, v_zero, v_one, v_mone, kind, s_after[c * PD_LS + k], (s_before[c] >> y) & 1u, y);
                }
            }
            u32x4 w;
            w.x = pd_pack(v, 0); w.y = pd_pack(v, 1); w.z = pd_pack(v, 2); w.w = pd_pack(v, 3);
            __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(out) + u);
            in += d_in; outer += d_outer;
            if (in >= LG) { in -= LG; outer++; }
        }
    } else {
        const uint32_t total = (uint32_t)HW * (uint32_t)L;
        for (uint32_t e = (uint32_t)tid; e < total; e += PD_BLOCK) {
            const int o = (int)(e / (uint32_t)inner), r = (int)(e - (uint32_t)o * (uint32_t)inner);
            const int k = LIST_MAJOR ? o : r, cell = LIST_MAJOR ? r : o;
            const int y = cell / NCOL, c = cell - y * NCOL;
            __builtin_nontemporal_store(pd_element(v_fill, v_zero, v_one, v_mone, s_kind[k], s_after[c * PD_LS + k], (s_before[c] >> y) & 1u, y), &out[e]);
        }
    }
    if (da.sums) {
        T* sums = (T*)da.sums + (size_t)i * HW;
        for (int t = tid; t < HW; t += PD_BLOCK) {
            const int y = t / NCOL, c = t - y * NCOL;
            uint32_t cnt = 0;
            for (int k = 0; k < L; k += 4) {                 // (the rows are zero from L on)
                const u32x4 a4 = *reinterpret_cast<const u32x4*>(&s_after[c * PD_LS + k]);
                cnt += ((a4.x >> y) & 1u) + ((a4.y >> y) & 1u) + ((a4.z >> y) & 1u) + ((a4.w >> y) & 1u);
            }
            const int b = (int)((s_before[c] >> y) & 1u);
            __builtin_nontemporal_store(plan_encode<T>(plan_sums_value((int)cnt - n_normal * b, n_small, fill)), &sums[t]);
        }
    }
}

// tetris_select_lists_dev: a workgroup of CHOOSE_THREADS threads takes G consecutive games (tetris_choose.h: the LDS image).
// What the call costs is reading phi (N x H x 10 x K elements of which one in K is used) and the acting players' column words
// (N x L x 10); nothing of size N x H x 10 x L exists.
//   A. the phi planes: consecutive threads take consecutive cells of one game (a stride of K elements in memory, so every cache
//      line of the games' phi is fetched once) and leave them in LDS, game-minor;
//   B. the column sums C_c for the small rule, thread = (game, column);
//   C. the scores: thread = (game g, slice s), lists k = s, s + S, ..: its ten column words are ten independent loads, coalesced
//      over the games of a slice (d_cols is game-minor); a normal list walks the set bits of after ^ before, one LDS read each;
//   D. one lane per game: total, q, choice, draw, entropy over at most 256 scores in LDS (choose_decide), the outputs that are one
//      element per game;
//   E. d_probs from LDS in memory order; d_sums and d_delta, thread = (game, column): the per-row counts over the normal lists as
//      bit-sliced counters over the column words (read a second time, from L2), staged through the LDS of the phi planes and
//      stored in memory order.
template <int G>
__device__ __forceinline__ void choose_store_planes(const PlanChooseArgs& ca, void* out, int g0, int ng, int HW, const float* s_plane) {
    constexpr int LS = G + 1;
    const size_t base = (size_t)g0 * HW;
    for (int e = (int)threadIdx.x; e < ng * HW; e += CHOOSE_THREADS) {
        const int g = e / HW, cell = e - g * HW;
        choose_store(out, base + e, s_plane[cell * LS + g], ca.out_f16);
    }
}

template <int G>
__global__ __launch_bounds__(CHOOSE_THREADS) void k_plan_choose(PlanChooseArgs ca) {
    extern __shared__ __attribute__((aligned(16))) uint32_t choose_lds[];
    constexpr int LS = G + 1, S = CHOOSE_THREADS / G;
    const int H = ca.a.H, HW = H * NCOL, L = ca.max_lists, P = ca.a.n_players;
    const size_t n = (size_t)ca.a.n;
    float* s_phi = reinterpret_cast<float*>(choose_lds);
    float* s_score = s_phi + HW * LS;
    float* s_col = s_score + L * LS;
    int* s_player = reinterpret_cast<int*>(s_col + NCOL * LS);
    int *s_piece = s_player + G, *s_count = s_piece + G, *s_choice = s_count + G, *s_small = s_choice + G, *s_normal = s_small + G;
    uint8_t* s_kind = reinterpret_cast<uint8_t*>(s_normal + G);
    const int t = (int)threadIdx.x, g0 = (int)blockIdx.x * G, ng = imin(G, ca.a.n - g0);
    const Geo geo = geo_of(ca.a);
    const uint32_t mask = plan_row_mask(H);
    if (t < G) {
        const bool live = t < ng;
        const int p = live ? safe_player(ca.player, g0 + t, P) : 0;
        s_player[t] = p;
        s_piece[t] = live ? act_piece_of(geo, (size_t)(g0 + t), p, ca.K) : 0;
        s_count[t] = live ? plan_clamp_count(ca.count[g0 + t], L) : 0;
    }
    __syncthreads();
    for (int e = t; e < ng * HW; e += CHOOSE_THREADS) {                                  // A
        const int g = e / HW, cell = e - g * HW;
        s_phi[cell * LS + g] = act_element(ca.phi, ((size_t)(g0 + g) * HW + cell) * ca.K + s_piece[g], ca.phi_f16);
    }
    __syncthreads();
    for (int u = t; u < NCOL * G; u += CHOOSE_THREADS) {                                 // B
        const int g = u % G, c = u / G;
        if (g < ng) s_col[c * LS + g] = choose_column_sum(s_phi + g, LS, H, c);
    }
    __syncthreads();
    {                                                                                   // C
        const int g = t % G, s = t / G, i = g0 + g;
        if (g < ng) {
            const int p = s_player[g], count = s_count[g];
            const Ref br = board_ref(geo, p, (size_t)i);
            uint32_t before[NCOL];
            TE_UNROLL
            for (int c = 0; c < NCOL; c++) before[c] = word_at(br, W_COL0 + c) & mask;
            const float plane_sum = choose_plane_sum(s_col + g, LS);
            for (int k = s; k < count; k += S) {
                const uint32_t* src = ca.cols + ((size_t)k * P + p) * NCOL * n + i;
                uint32_t after[NCOL];
                TE_UNROLL
                for (int c = 0; c < NCOL; c++) after[c] = src[(size_t)c * n] & mask;
                const int kind = plan_list_kind(k, count, plan_list_sum(after, before));
                s_score[k * LS + g] = choose_score(kind, after, before, s_phi + g, LS, ca.small_fill, plane_sum);
                s_kind[k * G + g] = (uint8_t)kind;
            }
        }
    }
    __syncthreads();
    if (t < ng) {                                                                       // D
        const int count = s_count[t];
        int n_small = 0;
        for (int k = 0; k < count; k++) n_small += s_kind[k * G + t] == PLAN_LIST_SMALL;
        s_small[t] = n_small;
        s_normal[t] = count - n_small;
        float prob, entropy;
        const int choice = choose_decide(ca, g0 + t, count, s_score + t, LS, prob, entropy);
        choose_write(ca, g0 + t, s_piece[t], choice, prob, entropy);
        s_choice[t] = choice;
    }
    __syncthreads();
    if (ca.probs) {                                                                     // E
        const size_t base = (size_t)g0 * L;
        for (int e = t; e < ng * L; e += CHOOSE_THREADS) {
            const int g = e / L, k = e - g * L;
            ca.probs[base + e] = k < s_count[g] ? s_score[k * LS + g] : 0.0f;
        }
    }
    if (ca.sums) {
        for (int u = t; u < NCOL * G; u += CHOOSE_THREADS) {
            const int g = u % G, c = u / G, i = g0 + g;
            if (g >= ng) continue;
            const int p = s_player[g], count = s_count[g], n_small = s_small[g], n_normal = s_normal[g];
            const uint32_t bw = word_at(board_ref(geo, p, (size_t)i), W_COL0 + c) & mask;
            const uint32_t* src = ca.cols + ((size_t)p * NCOL + c) * n + i;
            const size_t step = (size_t)P * NCOL * n;
            uint32_t plane[CHOOSE_COUNT_PLANES];
            TE_UNROLL
            for (int j = 0; j < CHOOSE_COUNT_PLANES; j++) plane[j] = 0u;
#pragma unroll 4
            for (int k = 0; k < count; k++) {
                const uint32_t word = src[(size_t)k * step] & mask;
                uint32_t carry = s_kind[k * G + g] == PLAN_LIST_NORMAL ? word : 0u;
                TE_UNROLL
                for (int j = 0; j < CHOOSE_COUNT_PLANES; j++) {
                    const uint32_t both = plane[j] & carry;
                    plane[j] ^= carry;
                    carry = both;
                }
            }
            for (int y = 0; y < H; y++) {
                uint32_t cnt = 0;
                TE_UNROLL
                for (int j = 0; j < CHOOSE_COUNT_PLANES; j++) cnt |= ((plane[j] >> y) & 1u) << j;
                s_phi[(y * NCOL + c) * LS + g] = plan_sums_value((int)cnt - n_normal * (int)((bw >> y) & 1u), n_small, ca.small_fill);
            }
        }
        __syncthreads();
        choose_store_planes<G>(ca, ca.sums, g0, ng, HW, s_phi);
        __syncthreads();
    }
    if (ca.delta) {
        for (int u = t; u < NCOL * G; u += CHOOSE_THREADS) {
            const int g = u % G, c = u / G, i = g0 + g;
            if (g >= ng) continue;
            const int p = s_player[g], count = s_count[g], choice = s_choice[g];
            const int kind = count > 0 ? (int)s_kind[choice * G + g] : (int)PLAN_LIST_PAST;
            const uint32_t bw = word_at(board_ref(geo, p, (size_t)i), W_COL0 + c) & mask;
            uint32_t aw = 0u;
            if (kind == PLAN_LIST_NORMAL) aw = ca.cols[(((size_t)choice * P + p) * NCOL + c) * n + i] & mask;
            for (int y = 0; y < H; y++)
                s_phi[(y * NCOL + c) * LS + g] = plan_delta_value(kind, kind == PLAN_LIST_NORMAL ? plan_cell_delta(aw, bw, y) : 0, ca.small_fill);
        }
        __syncthreads();
        choose_store_planes<G>(ca, ca.delta, g0, ng, HW, s_phi);
    }
}

// k_policy_eval: grid (ceil(N / 64), 40): a wave = 64 consecutive games of one candidate c = blockIdx.y, so that the state loads
// and the feature / score stores of a wave are coalesced rows (as k_plan_sim).  One wave per workgroup with its own LDS copy of
// the shape table.
template <bool FEAT>
__global__ __launch_bounds__(64) void k_policy_eval(PolicyArgs pa) {
    __shared__ uint32_t s_shapes[SHAPE_WORDS];
    s_shapes[threadIdx.x] = d_shape_table.s[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (i < pa.a.n) policy_eval_lane<FEAT>(pa, i, c, s_shapes);
}
// k_policy_pick: one lane per game, the maximum of its 40 scores
__global__ __launch_bounds__(256) void k_policy_pick(PolicyArgs pa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < pa.a.n) policy_pick_lane(pa, i);
}
