// Kernels of libtetris_hip.so, part 10: experience replay and its radix sort (bodies: tetris_replay.h).  Needs tetris_dev_traj.h
// (select_block_scan, SELECT_THREADS).

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
