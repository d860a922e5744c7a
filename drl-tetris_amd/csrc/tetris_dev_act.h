// Kernels of libtetris_hip.so, part 5: acting on a network's evaluation (bodies: tetris_act.h); tetris_dev_loss.h gathers with it too.
// Needs tetris_dev_vec.h.  From here on every kernel has one named block size, used by its launch bounds and by its launch.

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

// The block's elements, 16 bytes per lane and load.  Element e of the block belongs to game e / (40 K), candidate (e mod 40 K) / K
// and piece e mod K; 40 K is a multiple of the 4 or 8 elements of a vector, so a vector lies inside one game and (K = 7) holds
// at most two elements of the game's piece: only those are converted and stored.
template <int NT, int K, bool F16>
__device__ __forceinline__ void act_gather(const void* eval, int g0, int ng, ActShared& sh) {
    constexpr int EPV = F16 ? 8 : 4, PER_GAME = ACT_CANDIDATES * K;
    static_assert(PER_GAME % EPV == 0, "a 16-byte vector must not cross two games");
    const u32x4* src = (const u32x4*)((const char*)eval + (size_t)g0 * PER_GAME * (F16 ? 2 : 4));
    const int nvec = ng * (PER_GAME / EPV);
#pragma unroll 4
    for (int v = threadIdx.x; v < nvec; v += NT) {
        const u32x4 q = src[v];
        const int e0 = v * EPV, game = e0 / PER_GAME, rem = e0 - game * PER_GAME;
        if (K == 1) {
#pragma unroll
            for (int j = 0; j < EPV; j++) sh.x[(rem + j) * ACT_LDS_STRIDE + game] = vec_element<F16>(q, j, act_f16_to_f32);
        } else {
            int j = sh.piece[game] - rem % K;                 // the first element of the vector that belongs to the piece
            j = j < 0 ? j + K : j;
            if (j < EPV) sh.x[((rem + j) / K) * ACT_LDS_STRIDE + game] = vec_element<F16>(q, j, act_f16_to_f32);
            if (EPV > K && j + K < EPV) sh.x[((rem + j + K) / K) * ACT_LDS_STRIDE + game] = vec_element<F16>(q, j + K, act_f16_to_f32);
        }
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
    vec_with_k_f16(aa.K, aa.eval_f16 != 0, [](auto K, auto F16, auto&&... a) { act_gather<NT, K(), F16()>(a...); }, aa.action_eval, g0, ng, sh);
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
