// Kernels of libtetris_hip.so, part 3: what the core entry points of tetris_lib_core.h launch beside the step kernels
// (tetris_game_kernel.h) and the observations (tetris_dev_observe.h): split stages, drop enumeration, key lists, snapshots.
// The RNG table kernels are here too; the table management in tetris_lib_batch.h launches them.

template <int STAGE, bool TINT>
__global__ __launch_bounds__(256) void k_split(KArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_shapes_all[4][SHAPE_WORDS];      // per-wave copy, no block barrier (see k_game)
    uint32_t* s_shapes = s_shapes_all[threadIdx.x >> 6];
    s_shapes[threadIdx.x & 63] = d_shape_table.s[threadIdx.x & 63];
    __builtin_amdgcn_wave_barrier();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) split_body<STAGE, TINT>(a, i, s_shapes);
}

// ---- RNG tables: one lane per 16-bit seed, MT state strided [word][seed] (coalesced)
__global__ __launch_bounds__(256) void k_gen_seed(uint32_t* mt) {
    uint32_t seed = blockIdx.x * blockDim.x + threadIdx.x;
    if (seed >= 65536u) return;
    // randomizer.cpp:34-36,47-49: `short` seed converted to the engine's result type
    mt_seed(mt + seed, 65536, (uint32_t)(int32_t)(int16_t)(uint16_t)seed);
}

struct MapArg { uint8_t m[8]; };

__global__ __launch_bounds__(256) void k_gen_chunk(uint32_t* mt, float* w, uint8_t* out, uint64_t* start, int chunk,
                                                   MapArg map, int only_sz) {
    uint32_t seed = blockIdx.x * blockDim.x + threadIdx.x;
    if (seed >= 65536u) return;
    uint64_t word = 0;
    gen_chunk_for_seed(mt + seed, 65536, w + seed, 65536, out + (size_t)seed * CHUNK, &word, chunk, map.m, only_sz != 0);
    if (chunk == 0) start[seed] = word;
}

// BASELINE config 4.  One workgroup = one wave = ENUM_BOARDS (6) boards x 10 lanes; lane (board, xi) places the piece in column xi for
// the four rotations in turn.  Phase A: a board's ten lanes fetch its ten columns (ONE global load per word and board) and its piece
// word.  Phase B: they fill its BoardPre in LDS (tetris_kernels.h): band window (LDS atomics), depth strip (byte writes), prefix /
// suffix ANDs.  Phase C: four placements per lane from ~10 LDS reads each.  16 384 boards = 2 731 waves, all resident at once;
// the phases are ordered inside the wave (no workgroup barrier).
// PLANAR: rotation-minor planes — valid / land_y / cleared [n][10][4], after [10][n][10][4] (column plane c, game, column index,
// rotation) — so that a lane's four placements are one 4-byte / 16-byte store; else the layouts tetris_enumerate_drops documents
// ([n][4][10] and [n][4][10][10]).
template <int P, bool PLANAR>
__global__ __launch_bounds__(ENUM_BLOCK) void k_enumerate(Geo geo, int n, const int32_t* idx, const uint8_t* player, int H,
                                                          uint8_t* valid, int8_t* land_y, uint8_t* cleared, uint32_t* after) {
    __shared__ __attribute__((aligned(16))) uint32_t s_pre[ENUM_BOARDS][PRE_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t s_shapes[SHAPE_WORDS];
    const int tid = threadIdx.x, b = tid / 10, j = tid - b * 10;
    const int i = blockIdx.x * ENUM_BOARDS + b;                  // board of this lane
    const bool live = b < ENUM_BOARDS && i < n;
    uint32_t* pre = s_pre[b < ENUM_BOARDS ? b : 0];
    const uint32_t floor_bits = ~0u << H;
    if (tid < SHAPE_WORDS) s_shapes[tid] = d_shape_table.s[tid];
    uint32_t mine = 0;
    if (live) {
        const Ref br = board_ref(geo, safe_player(player, i, P), safe_slot(idx, i, (int)geo.n_games));
        mine = word_at(br, W_COL0 + j);
        pre[PRE_COL + j] = mine;
        if (j == 0) {
            pre[PRE_PIECE] = word_at(br, W_PIECE);
            pre[PRE_BAND] = 0xFFu; pre[PRE_BAND + 1] = 0xFFFF0000u;
        }
        if (j >= 1 && j < 5) pre[PRE_STRIP + (j - 1)] = 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (live) {
        int word;
        const uint32_t bits = pre_band_bits(mine, floor_bits, j, word);
        atomicOr(&pre[PRE_BAND + word], bits);
        ((uint8_t*)(pre + PRE_STRIP))[j + 2] = (uint8_t)pre_depth(mine, floor_bits);
        pre[PRE_PRE + j] = pre_and_below(pre + PRE_COL, j);
        pre[PRE_SUF + j] = pre_and_from(pre + PRE_COL, j);
        if (j == 0) { pre[PRE_PRE + NCOL] = pre_and_below(pre + PRE_COL, NCOL); pre[PRE_SUF + NCOL] = ~0u; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (!live) return;
    const ColumnCtx cc = enum_column(pre, j);
    if (PLANAR) {
        // rotation-minor planes: the lane's four placements are adjacent, so each result array takes ONE 4-byte store per lane and
        // each afterstate column ONE 16-byte store (13 stores per lane instead of 52; a wave's store = 1 KB contiguous)
        Placement pl[4];
        uint32_t v_ok = 0, v_y = 0, v_cl = 0;
        TE_UNROLL
        for (int r = 0; r < 4; r++) {
            pl[r] = enum_place(pre, cc, s_shapes, H, r);
            v_ok |= (uint32_t)pl[r].ok << (8 * r);
            v_y |= ((uint32_t)pl[r].y & 0xFFu) << (8 * r);
            v_cl |= (uint32_t)pl[r].cleared << (8 * r);
        }
        const size_t t4 = (size_t)i * 10 + j;                     // element (game i, column index j) of the [n][10][4] arrays
        reinterpret_cast<uint32_t*>(valid)[t4] = v_ok;
        reinterpret_cast<uint32_t*>(land_y)[t4] = v_y;
        reinterpret_cast<uint32_t*>(cleared)[t4] = v_cl;
        if (after) {
            u32x4* out = reinterpret_cast<u32x4*>(after);
            const size_t plane = (size_t)n * 10;
            for (int c = 0; c < NCOL; c++) {
                const uint32_t bc = pre[PRE_COL + c];
                u32x4 v;
                v.x = enum_after_col(bc, pl[0], c); v.y = enum_after_col(bc, pl[1], c);
                v.z = enum_after_col(bc, pl[2], c); v.w = enum_after_col(bc, pl[3], c);
                __builtin_nontemporal_store(v, &out[(size_t)c * plane + t4]);
            }
        }
    } else {
        uint32_t board[NCOL];                                   // the board's columns, read once for the four afterstates
        if (after)
            for (int c = 0; c < NCOL; c++) board[c] = pre[PRE_COL + c];
        TE_UNROLL
        for (int r = 0; r < 4; r++) {
            const Placement pl = enum_place(pre, cc, s_shapes, H, r);
            const size_t t = ((size_t)i * 4 + r) * 10 + j;
            valid[t] = (uint8_t)pl.ok;
            land_y[t] = (int8_t)pl.y;
            cleared[t] = (uint8_t)pl.cleared;
            if (after)
                for (int c = 0; c < NCOL; c++) after[t * NCOL + c] = enum_after_col(board[c], pl, c);      // 40 contiguous bytes per lane: left to the L2 to merge
        }
    }
}

template <int P>
__global__ __launch_bounds__(64) void k_actions(Geo geo, int n, const int32_t* idx, const uint8_t* player,
                                                int H, uint8_t* count, uint8_t* lens, uint8_t* keys, int max_lists, int max_keys,
                                                uint32_t* status) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (size_t)n * 40)
        actions_body<P>(geo, t, idx, player, H, d_shape_table.s, count, lens, keys, max_lists, max_keys, status);
}

__global__ __launch_bounds__(256) void k_snapshot(Geo geo, int n, const int32_t* idx, uint32_t* blob, int restore) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (size_t)n * (NGWORDS + geo.P * geo.nw)) snapshot_body(geo, t, idx, blob, restore);
}

__global__ __launch_bounds__(256) void k_set_dead(Geo geo, int n, const int32_t* idx, const uint8_t* dead /*[n][P]*/) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n * geo.P) set_dead_body(geo, t, idx, dead);
}
