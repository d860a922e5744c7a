// Kernels of libtetris_hip.so, part 1: observations.  The tile helpers that turn a board's ten column words into its byte plane
// in LDS and stream the tile out, the observation kernels of tetris_lib_core.h's entry points, and the step that leaves its
// observation behind.  First of the kernel headers of tetris_hip.hip because k_duo (tetris_dev_rollout.h) builds its
// observation with obs_build and obs_stream, and k_traj_batch (tetris_dev_traj.h) its tile with obs_row_words / obs_row_halves.
// Needs tetris_game_kernel.h (d_shape_table) and tetris_dev_vec.h.

template <int P, bool TINT>
__global__ __launch_bounds__(256) void k_observe(Geo geo, int n, const int32_t* idx, int H, tetris_record* rec, uint8_t* round_over,
                                                 int8_t* last_winner) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) observe_body<P, TINT>(geo, i, idx, H, d_shape_table.s, rec, round_over, last_winner);
}

// One board's ten column words -> its row of a workgroup's LDS tile, for even heights: the byte planes are built as words in
// registers — two rows = 20 cells = 5 words per loop trip, columns indexed statically — and go to LDS as dwords.  Shared by
// k_observe_packed (below) and k_traj_batch (tetris_dev_traj.h).  `col` is used up.
__device__ __forceinline__ void obs_row_words(uint32_t (&col)[NCOL], int H, uint32_t* row) {
    for (int yp = 0; yp < H / 2; yp++) {
        uint32_t lo[NCOL], hi[NCOL];                 // cells of rows 2 yp and 2 yp + 1
        for (int c = 0; c < NCOL; c++) { lo[c] = col[c] & 1u; hi[c] = (col[c] >> 1) & 1u; col[c] >>= 2; }
        row[5 * yp + 0] = lo[0] | (lo[1] << 8) | (lo[2] << 16) | (lo[3] << 24);
        row[5 * yp + 1] = lo[4] | (lo[5] << 8) | (lo[6] << 16) | (lo[7] << 24);
        row[5 * yp + 2] = lo[8] | (lo[9] << 8) | (hi[0] << 16) | (hi[1] << 24);
        row[5 * yp + 3] = hi[2] | (hi[3] << 8) | (hi[4] << 16) | (hi[5] << 24);
        row[5 * yp + 4] = hi[6] | (hi[7] << 8) | (hi[8] << 16) | (hi[9] << 24);
    }
}
// the same for odd heights, where a board's H * 10 bytes start on an even byte that need not be a word: one row = 5 halfwords
__device__ __forceinline__ void obs_row_halves(uint32_t (&col)[NCOL], int H, uint16_t* row) {
    for (int y = 0; y < H; y++) {
#pragma unroll
        for (int k = 0; k < NCOL / 2; k++) row[5 * y + k] = (uint16_t)((col[2 * k] & 1u) | ((col[2 * k + 1] & 1u) << 8));
#pragma unroll
        for (int c = 0; c < NCOL; c++) col[c] >>= 1;
    }
}

// Observation kernel: one lane reads its board's ten column words (coalesced SoA), expands them to H*10 bytes
// in LDS; after a barrier the workgroup streams its 256 boards' planes out as ONE contiguous run of dwords, so the
// uint8 rows leave the chip fully coalesced (a lane writing its own 200 bytes would not be).
template <int P>
__global__ __launch_bounds__(256) void k_observe_packed_bytes(Geo geo, int n, const int32_t* idx,
                                                        const uint8_t* player, int H, uint8_t* visual, uint8_t* vector,
                                                        uint8_t* piece) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_cells[];      // 256 * H * 10 bytes
    const int cells = H * NCOL;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int first = blockIdx.x * 256;
    const int nb = (n - first < 256) ? n - first : 256;
    for (int sl = 0; sl < P; sl++) {
        if (i < n) {
            const size_t slot = safe_slot(idx, i, (int)geo.n_games);
            const int me = safe_player(player, i, P);
            const int p = (sl == 0) ? me : (P - 1 - me);
            uint8_t vec[12];
            const int kind = observe_board(geo, slot, p, H, s_cells + (size_t)threadIdx.x * cells, vec);
            uint8_t* v = vector + ((size_t)sl * n + i) * 12;
            for (int k = 0; k < 12; k++) v[k] = vec[k];
            piece[(size_t)sl * n + i] = (uint8_t)kind;
        }
        __syncthreads();
        uint8_t* out = visual + ((size_t)sl * n + first) * cells;
        const size_t bytes = (size_t)nb * cells;
        if ((((uintptr_t)out | bytes) & 3u) == 0) {
            const uint32_t* src = (const uint32_t*)s_cells;
            uint32_t* dst = (uint32_t*)out;
            for (size_t k = threadIdx.x; k < bytes / 4; k += 256) dst[k] = src[k];
        } else {
            for (size_t k = threadIdx.x; k < bytes; k += 256) out[k] = s_cells[k];
        }
        __syncthreads();
    }
}

// Even heights (H * 10 cells = a whole number of words per board, the usual 20 / 22 rows): the byte planes are built as
// words in registers — two rows = 20 cells = 5 words per loop trip, columns indexed statically — and go to LDS as dwords
// instead of 200 byte writes per lane; the workgroup's tile then leaves as coalesced 16-byte stores.  The 12 vector bytes of a
// board leave as 3 dwords.
template <int P, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_observe_packed(Geo geo, int n, const int32_t* idx,
                                                          const uint8_t* player, int H, uint8_t* visual, uint8_t* vector,
                                                          uint8_t* piece) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_words[];      // BLOCK * nw words: the workgroup's slice of `visual` itself
    const int nw = H * NCOL / 4;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const int first = blockIdx.x * BLOCK;
    const int nb = (n - first < BLOCK) ? n - first : BLOCK;
    {
        const int sl = blockIdx.y;                       // one workgroup per (64 boards, slot): twice the waves in flight for P = 2
        if (i < n) {
            const size_t slot = safe_slot(idx, i, (int)geo.n_games);
            const int me = safe_player(player, i, P);
            const int p = (sl == 0) ? me : (P - 1 - me);
            const Ref br = board_ref(geo, p, slot);
            uint32_t col[NCOL];
            for (int c = 0; c < NCOL; c++) col[c] = word_at(br, W_COL0 + c);
            const uint32_t w = word_at(br, W_PIECE), m = word_at(br, W_MISC), dc = word_at(br, W_DROPCOMBO);
            obs_row_words(col, H, s_words + (size_t)threadIdx.x * nw);
            // state_processors.py:23-54 vector: x, y, incoming, combo time, combo count, one-hot next piece
            const ObsScalars s = obs_scalars(w, m, dc);
            uint32_t* v = (uint32_t*)(vector + ((size_t)sl * n + i) * 12);
            obs_vector_words(s, false, v[0], v[1], v[2]);
            piece[(size_t)sl * n + i] = (uint8_t)s.kind;
        }
        __syncthreads();
        // the tile is not padded (rows nw words apart: at most two lanes per LDS bank while it is written), so it IS the output
        // image: one 16-byte LDS read per 16-byte streaming store, no index arithmetic
        uint32_t* dst = (uint32_t*)(visual + ((size_t)sl * n + first) * (size_t)(H * NCOL));
        const uint32_t words = (uint32_t)nb * (uint32_t)nw;
        if ((((uintptr_t)dst) & 15u) == 0) {
            const uint32_t whole = words & ~3u;
            for (uint32_t g = 4u * threadIdx.x; g < whole; g += 4u * BLOCK)
                __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(s_words + g), reinterpret_cast<u32x4*>(dst + g));
            if (threadIdx.x < words - whole) dst[whole + threadIdx.x] = s_words[whole + threadIdx.x];
        } else
            for (uint32_t g = threadIdx.x; g < words; g += BLOCK) dst[g] = s_words[g];
    }
}

// ---- step + observation in one launch (tetris_step_rt_observe_dev) ------------------------------------------------------------
// One agent-loop iteration in ONE launch (worker.py:91-118: perform_action, then get_state + unpack for the next decision): the
// (r, t) step and, straight from the registers the step leaves behind, the packed observation k_observe_packed would rebuild
// from the stored state — no second launch, no second read of the state.  A wave's byte planes go through an LDS tile and leave
// as contiguous runs of 16-byte stores.  Even heights only (H * 10 cells = whole words per board).
// one board -> its row of the tile, its 12 vector bytes and its piece byte (slot sl, game i): as k_observe_packed
// (a macro, not a function: as an inlined function with the board passed by reference, by value or as seventeen scalars, the
// compiler left the step's column array in scratch memory — 128 B per lane and +1.5 us per launch)
#define TE_OBS_BUILD(a, row, sl, i, COL, qx, qy, qnext, qkind, qinc, qcombo, qrem)                                              \
    do {                                                                                                                        \
        uint32_t col_[NCOL];                                                                                                    \
        TE_UNROLL                                                                                                               \
        for (int c = 0; c < NCOL; c++) col_[c] = COL(c);                                                                        \
        for (int yp = 0; yp < (a).H / 2; yp++) {                                                                                \
            uint32_t lo[NCOL], hi[NCOL]; /* cells of rows 2 yp and 2 yp + 1 */                                                  \
            TE_UNROLL                                                                                                           \
            for (int c = 0; c < NCOL; c++) { lo[c] = col_[c] & 1u; hi[c] = (col_[c] >> 1) & 1u; col_[c] >>= 2; }                \
            (row)[5 * yp + 0] = lo[0] | (lo[1] << 8) | (lo[2] << 16) | (lo[3] << 24);                                           \
            (row)[5 * yp + 1] = lo[4] | (lo[5] << 8) | (lo[6] << 16) | (lo[7] << 24);                                           \
            (row)[5 * yp + 2] = lo[8] | (lo[9] << 8) | (hi[0] << 16) | (hi[1] << 24);                                           \
            (row)[5 * yp + 3] = hi[2] | (hi[3] << 8) | (hi[4] << 16) | (hi[5] << 24);                                           \
            (row)[5 * yp + 4] = hi[6] | (hi[7] << 8) | (hi[8] << 16) | (hi[9] << 24);                                           \
        }                                                                                                                       \
        /* state_processors.py:23-54 vector: x, y, incoming, combo time, combo count, one-hot next piece */                     \
        const uint32_t x_ = (uint32_t)(qx) & 0xFFu, y_ = (uint32_t)(qy) & 31u, next_ = (uint32_t)(qnext) & 7u;                  \
        uint32_t t_ = (((uint32_t)(qrem) & 0xFFFFu) + 50u) & 0xFFFFu; /* uint16 + 50 wraps like numpy (state_processors.py:38) */ \
        if (t_ > 25000u) t_ = 25000u;                                                                                           \
        uint32_t* v_ = (uint32_t*)((a).obs_vector + ((size_t)(sl) * (a).n + (i)) * 12);                                         \
        const uint64_t hot_ = next_ < 7u ? (1ull << (8 * next_)) : 0ull; /* bytes 5..11 */                                      \
        v_[0] = x_ | (y_ << 8) | (((uint32_t)(qinc) & 255u) << 16) | ((t_ / 100u) << 24);                                       \
        v_[1] = ((uint32_t)(qcombo) & 255u) | ((uint32_t)(hot_ & 0xFFFFFFu) << 8);                                              \
        v_[2] = (uint32_t)(hot_ >> 24);                                                                                         \
        (a).obs_piece[(size_t)(sl) * (a).n + (i)] = (uint8_t)((uint32_t)(qkind) & 7u);                                          \
    } while (0)
// the same as a function of scalars — the form that stays in registers inside k_duo (there the macro cost 784 B of scratch per lane)
__device__ __forceinline__ void obs_build(const KArgs& a, uint32_t* row, int sl, int i, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t c4,
                                          uint32_t c5, uint32_t c6, uint32_t c7, uint32_t c8, uint32_t c9, int qx, int qy, int qnext, int qkind,
                                          int inc_count, int combo_count, uint32_t combo_remaining) {
    const uint32_t cols[NCOL] = {c0, c1, c2, c3, c4, c5, c6, c7, c8, c9};
#define TE_OBS_COL(c) cols[c]
    TE_OBS_BUILD(a, row, sl, i, TE_OBS_COL, qx, qy, qnext, qkind, inc_count, combo_count, combo_remaining);
#undef TE_OBS_COL
}
// `nb` consecutive tile rows (boards first .. first + nb of slot sl) -> visual, by the 64 lanes of one wave.  The tile is NOT padded
// (row pitch = nw words), so it is the output image itself: one 16-byte LDS read per 16-byte store, no index arithmetic.  (The rows
// of a wave's lanes then start 50 / 55 / ... words apart: two lanes per LDS bank at most while the rows are written.)
__device__ __forceinline__ void obs_stream(const KArgs& a, const uint32_t* rows, int sl, int first, int nb, int lane) {
    const int nw = a.H * NCOL / 4;
    uint32_t* dst = (uint32_t*)(a.obs_visual + ((size_t)sl * a.n + first) * (size_t)(a.H * NCOL));
    const uint32_t words = (uint32_t)nb * (uint32_t)nw;
    if (((((uintptr_t)dst) | ((uintptr_t)rows)) & 15u) == 0) {
        const uint32_t whole = words & ~3u;
        for (uint32_t k = 4u * (uint32_t)lane; k < whole; k += 4u * 64u)
            __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(rows + k), reinterpret_cast<u32x4*>(dst + k));
        if ((uint32_t)lane < words - whole) dst[whole + lane] = rows[whole + lane];
    } else
        for (uint32_t k = (uint32_t)lane; k < words; k += 64u) dst[k] = rows[k];
}

// lane = game (k_step_observe): slot 0 = the deciding player's board, slot 1 = the opponent's, one slot after the other
template <int P>
__device__ __forceinline__ void observe_emit(const KArgs& a, const Game<P>& g, int first, int lane, bool active, uint32_t* tile) {
    const int pitch = a.H * NCOL / 4, i = first + lane;
    const int nb = (a.n - first < 64) ? a.n - first : 64;
    const int me = active ? safe_player(a.next_player, i, P) : 0;
    TE_UNROLL
    for (int sl = 0; sl < P; sl++) {
        if (active) {
            const bool sel = P > 1 && (sl == 0 ? me == 1 : me == 0);      // field-wise select of the second player's board
            const Player& q0 = g.pl[0];
            const Player& q1 = g.pl[P - 1];
            uint32_t* row = tile + (size_t)lane * pitch;
#define TE_OBS_COL(c) (sel ? q1.col[c] : q0.col[c])
            TE_OBS_BUILD(a, row, sl, i, TE_OBS_COL, sel ? q1.x : q0.x, sel ? q1.y : q0.y, sel ? q1.next : q0.next, sel ? q1.kind : q0.kind,
                         sel ? q1.inc_count : q0.inc_count, sel ? q1.combo_count : q0.combo_count, sel ? q1.combo_remaining : q0.combo_remaining);
#undef TE_OBS_COL
        }
        __syncthreads();
        obs_stream(a, tile, sl, first, nb, lane);
        __syncthreads();
    }
}

template <int P, int MODE>
__global__ __launch_bounds__(64) void k_step_observe(KArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_step_obs[];     // [SHAPE_WORDS] shape table, then the 64 x nw tile
    uint32_t* s_shapes = s_step_obs;
    uint32_t* tile = s_step_obs + SHAPE_WORDS;
    const int lane = threadIdx.x, first = blockIdx.x * 64, i = first + lane;
    const bool active = i < a.n;
    LaneCounters cnt = {0, 0, 0, 0};
    const uint32_t shape_word = d_shape_table.s[lane];
    Game<P> g;
    if (active) game_load<P, MODE, false>(a, i, g);
    s_shapes[lane] = shape_word;
    __builtin_amdgcn_wave_barrier();
    if (active) game_run<P, MODE, false>(a, i, s_shapes, g, cnt);
    observe_emit<P>(a, g, first, lane, active, tile);
}
