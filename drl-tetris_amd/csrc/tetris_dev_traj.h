// Kernels of libtetris_hip.so, part 9: trajectory windows, a window's states, sample sets and minibatches, and the planning agent's
// windows (bodies: tetris_traj.h, tetris_batch.h, tetris_plan_traj.h).  Needs tetris_dev_vec.h and tetris_dev_observe.h
// (obs_row_words, obs_row_halves) and tetris_dev_agent_plan.h (pd_pack).  select_block_scan also serves tetris_dev_replay.h.

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
