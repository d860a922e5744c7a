// libtetris_hip.so — kernels and C ABI of the MI355X batched Tetris environment (gfx950 only).
//
// One lane = one game (all its players), state SoA in HBM (tetris_layout.h), step logic in
// tetris_engine.h.  Launch geometry: 256-thread workgroups (one wave per SIMD of a CU); 64k games
// = 256 workgroups = one per CU, so the kernel is latency/issue bound, not occupancy bound.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <new>
#include <chrono>
#include <string>
#include <vector>

#include "tetris_kernels.h"

using namespace te;

// ============================================================================ device side

#include "tetris_game_kernel.h"

// Chained launches of the built-in rollout (one env-step per launch).  A game's step E depends on nothing but the same game's
// step E - 1, yet launches on one stream are separated by a full barrier: launch E waits for the SLOWEST wave of launch E - 1
// plus the kernel boundary (~1.4 us of a ~5.7 us launch period, profiles/).  Here consecutive launches rotate over CHAIN_STREAMS (3)
// streams, so launch E is dispatched while E - 1 and E - 2 still run, and the dependence is enforced per WAVE (one workgroup = one
// wave = 64 games): wave w of launch E polls an epoch word until wave w of launch E - 1 has published E - 1.  Every state
// load / store is agent-scope (`sc1`: written through, read past the per-XCD L2), the storing wave drains its stores
// (`s_waitcnt vmcnt(0)`) before it publishes — the measured-valid hand-off of MI355X_MICROARCH.md.  Spins are bounded: a wave
// that gives up marks its epoch word (CHAIN_ABANDONED), raises F_CHAIN and leaves its games untouched; so does the same wave of
// every later launch, and the host finishes those games un-chained once the streams have drained (chain_recover).
constexpr int CHAIN_LANES = 64;      // games per wave of k_chain
constexpr int CHAIN_STREAMS = 3;     // streams the chained launches rotate over = launches in flight.  3 x 1024 waves of 64k single-player
                                     // boards fit in the 15 x 256 wave slots chain_fits counts; GPU-paced 4.02 us per launch against 4.14 with 2
                                     // (with the epoch words still packed 32 to a line it had been 4.9-5.06 against 4.71-4.80)
// XCD-AFFINE form (k_chain_affine; direct dispatch only, tetris_aql.h).  The write-through hand-off above crosses the fabric twice per
// step because block b of consecutive launches never meets its own XCD again (a queue deals its blocks round-robin over the eight XCDs
// from a start of its own: profiles/r03/handoff_experiments.txt).  Here the GAMES follow the XCD instead: the workgroup that finds
// itself on XCD x takes the game block (b & ~7) | x, so a block is stepped on the same XCD in every launch and its state and epoch
// word can stay in that XCD's L2 — plain stores, `sc1` loads (past the CU's L1, served by the L2).  One L2 is coherent for all CUs
// of its XCD; nothing else is relied on.  That the eight workgroups of a group of eight really sit on eight different XCDs is
// CHECKED, by every workgroup for itself: the queue's start XCD is measured when the queue is made (a.xcd_base), and a
// workgroup that is not on XCD (xcd_base + b) mod 8 touches nothing, raises F_PLACE and leaves — its games then look abandoned to the
// next launch, whose waves give up, and the host finishes the call un-chained (chain_recover) and switches the affine form off.
// What makes this FASTER only with direct dispatch: the packets between a queue's first and last carry no cache maintenance
// (a kernel boundary's L2 write-back + invalidate, three times per 12 us, cost more than the fabric: +0.1 us per launch through
// streams); the queue's last packet releases, so memory is current when the call returns.
// FUSED says which launches a kernel serves.  false: one env-step per launch, the case that is timed (k_chain, k_chain_affine) —
// rollout_step once, straight-line.  With game_run's loop over a.steps around the step the compiler hoists the loop's constants
// and the next step's policy draw into a preheader BEHIND the state loads, where every instruction is on the wave's dependent
// chain, and keeps a second copy of Philox in the body; a one-step launch uses none of it.  true: any other step count (k_chain_fused,
// k_chain_fused_affine: S > 1, and S = 0 of the counter calibration), game_run with its loop.
template <int P, bool AFFINE, bool FUSED>
__device__ __forceinline__ void chain_body(const KArgs& a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_shapes[SHAPE_WORDS];
    const int lane = threadIdx.x;
    if (a.steps < 0) { chain_census(a, lane == 0); return; }
    constexpr int CMEM = AFFINE ? MEM_AFFINE : MEM_AGENT;
    int wave = blockIdx.x;
    uint32_t xcc = 0;
    // AFFINE: block 0 reports where this queue starts dealing (F_XCC0 + queue: the host's expectation for the next call) on its way
    // out, so that the store's trip to host memory never holds up the step (a wave waits for ALL its outstanding vector memory
    // accesses at the first poll)
    const auto report_xcc = [&]() { if (AFFINE && blockIdx.x == 0 && lane == 0) st_flag(a.status + F_XCC0 + (a.xcd_slot & 3u), 0x100u | xcc); };
    if (AFFINE) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 0xFu;
        if (xcc != ((a.xcd_base + blockIdx.x) & 7u)) {          // not where the host expects this block to run: hands off
            if (lane == 0) st_flag(a.status + F_PLACE, 1u);
            report_xcc();
            return;
        }
        wave = (int)((blockIdx.x & ~7u) | xcc);
        if (wave * CHAIN_LANES >= a.n) { report_xcc(); return; }   // (padding of the last group of eight: no games, no epoch word)
    }
    const int i = wave * CHAIN_LANES + lane;
    const bool active = lane < CHAIN_LANES && i < a.n;
    LaneCounters cnt = {0, 0, 0, 0};
    const uint32_t shape_word = d_shape_table.s[lane];     // (issued at the top; it has long arrived when the LDS table is written)
    Game<P> g;
    // Work that does not depend on the predecessor happens before the poll: the policy draw of this step (kernel arguments only:
    // its 40 dependent multiplies run while the wave waits), and the row stride of the state arrays (pinned into an SGPR here;
    // the compiler would load it after the poll, with a wait for the scalar load in front of the first state load).  The LDS
    // shape table is written after the state loads are issued: written before the poll it would need a wait for its global load
    // in front of the first poll.
    // (Issuing the first poll of the epoch word BEFORE the draw — most waves find their predecessor done at that poll — measured
    // +0.06 us per launch, GPU-paced: profiles/r02/chain_ab_gpu_paced.txt.)
    if (active) policy_draw(a, (uint32_t)i, a.first_step, g.draw0, g.draw1);
    const uint32_t d0 = g.draw0, d1 = g.draw1;
    int stride = a.n_stride;
    asm volatile("" : "+s"(stride));
    // The single-step kernels also multiply out, here, the byte offsets of the state rows the step touches (tetris_engine.h: RowTable)
    // and pin them into SGPRs: the loads behind the poll and the stores behind the step then find their offsets ready.  Left to itself
    // the compiler multiplies them out where they are used, twice, between the loads and among the stores: on the chain.
    RowTable<NWORDS> rows = {};
    RowTable<NGWORDS> grows = {};
    if (!FUSED) {
        TE_UNROLL
        for (int w = 0; w < NWORDS; w++)
            if (P > 1 || (w < NWORDS_HOT && w != W_INCOMING && w != W_HOLE_DRAWS)) {      // (one player: no queue, these are never touched)
                uint32_t bytes = (uint32_t)(w * P) * (uint32_t)stride * 4u;
                asm volatile("" : "+s"(bytes));
                rows.bytes[w] = bytes;
            }
        TE_UNROLL
        for (int w = 0; w < NGWORDS; w++) {            // (G_LINES, G_SENT: the rare counter atomics)
            uint32_t bytes = (uint32_t)w * (uint32_t)stride * 4u;
            asm volatile("" : "+s"(bytes));
            grows.bytes[w] = bytes;
        }
    }
    const uint32_t seen = chain_poll(a, (uint32_t)wave);
    if (seen == a.epoch - 1u) {                 // (a uniform branch: the state loads follow the poll's exit)
        Geo geo = geo_of(a);
        geo.stride = (size_t)stride;
        if (active) {
            if (FUSED) load_game<P>(geo, (size_t)i, g, false, P > 1, true, CMEM);
            else load_game_rows<P>(geo, (size_t)i, rows, grows, g, false, P > 1, true, CMEM);
            g.draw0 = d0; g.draw1 = d1;
        }
        s_shapes[lane] = shape_word;
        __builtin_amdgcn_wave_barrier();
        if (FUSED) {
            if (active) game_run<P, M_ROLLOUT, false, CMEM>(a, i, s_shapes, g, cnt);
        } else if (active) {
            const Ctx cx = make_ctx(a, s_shapes, false, P > 1);
            rollout_step<P>(cx, a, (size_t)i, a.first_step, g, cnt);
            store_game_rows<P>(geo, (size_t)i, rows, grows, g, false, P > 1, true, CMEM);
            report_status(a, g.status);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every store (and counter atomic) of this wave has been acknowledged
        if (lane == 0) {
            // AFFINE: a plain store, the line stays in this XCD's L2 where the next launch's wave polls it; otherwise written through
            // (`sc1`).  Neither waits for its acknowledgement: the wave ends here.
            if (AFFINE) st_xcd(a.chain + (size_t)wave * CHAIN_STRIDE, a.epoch);
            else st_agent(a.chain + (size_t)wave * CHAIN_STRIDE, a.epoch);
        }
    } else if (!(seen & CHAIN_ABANDONED)) {     // (with the bit set an earlier launch's wave gave up and recorded it)
        chain_give_up(a, (uint32_t)wave, lane == 0);          // the games stay as launch E - 1 (or an earlier one) left them
    }
    report_xcc();
}
template <int P>
__global__ __launch_bounds__(64) void k_chain(KArgs a) { chain_body<P, false, false>(a); }
template <int P>
__global__ __launch_bounds__(64) void k_chain_affine(KArgs a) { chain_body<P, true, false>(a); }
template <int P>
__global__ __launch_bounds__(64) void k_chain_fused(KArgs a) { chain_body<P, false, true>(a); }
template <int P>
__global__ __launch_bounds__(64) void k_chain_fused_affine(KArgs a) { chain_body<P, true, true>(a); }
template __global__ void k_chain_affine<1>(KArgs);
template __global__ void k_chain_fused_affine<1>(KArgs);
// the XCD every workgroup of a launch lands on (calibration of the affine form: aql::make_queues)
extern "C" __global__ void tetris_k_xcc_probe(uint32_t* out) {
    if (threadIdx.x == 0) {
        uint32_t xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        out[blockIdx.x] = xcc & 0xFu;
    }
}

// Measurement / test aid: keeps a stream busy until the HOST sets `*go` (a word in pinned host memory; NULL: no such word) or
// `ticks` of the 100 MHz real-time clock have passed, whichever comes first.  TETRIS_PREQUEUE=1 parks the chain streams behind it
// while the host enqueues, so that every launch of the call is queued before the first one starts — the GPU-paced launch period
// without any host pacing; tetris_debug_stall uses it to hold a stream or the device's wave slots (tests of the give-up path).
__global__ void k_blocker(const uint32_t* go, unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) {
        if (go && __hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) break;
        __builtin_amdgcn_s_sleep(32);
    }
}

// Measurement aid (tetris_debug_clock_khz): shader clock of the moment, from the ratio of the shader cycle counter to the constant
// 100 MHz real-time counter over ~`ticks` of the latter, by one wave
__global__ void k_clock_probe(unsigned long long ticks, unsigned long long* out) {
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) { __builtin_amdgcn_s_sleep(4); r1 = __builtin_amdgcn_s_memrealtime(); }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}

// Sums the per-game cumulative rollout counters (G_STEPS, G_EPISODE, G_LINES, G_SENT): run once before and once
// after a rollout, outside its timed region, instead of any cross-lane reduction inside the step
// kernel (4096 same-address atomics per launch cost ~28 us; a shuffle + LDS + read-modify-write tail
// still ~1.2 us of a 8 us launch).
__global__ __launch_bounds__(256) void k_totals(Geo geo, unsigned long long* out /*[4]*/) {
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (int)geo.n_games; i += gridDim.x * blockDim.x) {
        unsigned long long t[4];
        totals_of_game(geo, i, t);
        v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
    }
    for (int k = 0; k < 4; k++) {
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
        if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd(&out[k], v[k]);
    }
}

// The per-game words as they stand, totals[k][i] (tetris_rollout_game_totals_dev; kept by a rollout call that reports counters), and
// what the games counted since such a copy: (now - before) mod 2^32 per game, summed in 64 bits.  The words are cumulative modulo
// 2^32, so the difference of two k_totals sums is off by 2^32 for every word that wrapped in between; this one is exact as long as
// no single game counts 2^32 between the two readings.
__global__ __launch_bounds__(256) void k_policy_totals(Geo geo, uint32_t* totals /*[4][N]*/) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int)geo.n_games) policy_game_totals_lane(geo, i, totals);
}
__global__ __launch_bounds__(256) void k_totals_since(Geo geo, const uint32_t* before /*[4][N]*/, unsigned long long* out /*[4]*/) {
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (int)geo.n_games; i += gridDim.x * blockDim.x) {
        unsigned long long t[4];
        totals_of_game(geo, i, t);
        for (int k = 0; k < 4; k++) v[k] += (uint32_t)((uint32_t)t[k] - before[(size_t)k * geo.n_games + i]);
    }
    for (int k = 0; k < 4; k++) {
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
        if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd(&out[k], v[k]);
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
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
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

// "Duo" mapping for two-player games (BASELINE config 3): the two players of a game sit in lanes l and l ^ 32 of ONE wave,
// so 64k games are 2 waves per SIMD instead of 1 and the second player's clear/spawn, timers and state traffic overlap with
// the first's.  The in-step order dependence between the players is the split-mode stage protocol (tetris_engine.h) with
// the exchange words moved by __shfl_xor(.., 32): A = key interpreter + loop 1 (player 1 speculatively, with a register
// backup for the rollback when player 0 died), B0 / B1 = delayCheck of player 0, then player 1, C = winner logic.
// CHAIN (rollout only, 64-thread workgroups): chained launches as in k_chain — a wave's 32 games wait for the epoch word the same
// wave of the previous launch published, and all state traffic is agent-scope.
// OBS (tetris_step_rt_observe_dev): after the step every lane turns its own board into the packed observation — slot 0 if its
// player is the one the game's next decision is for, slot 1 otherwise; rows 0..31 / 32..63 of the wave's LDS tile.
// AFFINE (with CHAIN; k_duo_affine, direct dispatch only): the XCD-affine hand-over of k_chain_affine — a wave's 32 games follow the XCD.
template <int MODE, bool CHAIN, bool OBS, bool AFFINE>
__device__ __forceinline__ void duo_body(const KArgs& a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_shapes_all[4][SHAPE_WORDS];      // per-wave copy, no block barrier (see k_game)
    extern __shared__ __attribute__((aligned(16))) uint32_t s_duo_tile[];               // OBS: 4 waves x 64 rows x nw words
    uint32_t* s_shapes = s_shapes_all[threadIdx.x >> 6];
    const uint32_t shape_word = d_shape_table.s[threadIdx.x & 63];
    const int lane = threadIdx.x & 63, side = lane >> 5;
    int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    constexpr bool ROLL = MODE == M_ROLLOUT, AUTO = MODE == M_STEP_RT_AUTO;
    constexpr int MEM = CHAIN ? (AFFINE ? MEM_AFFINE : MEM_AGENT) : MEM_STREAM;
    if (CHAIN && a.steps < 0) { chain_census(a, lane == 0); return; }
    uint32_t xcc = 0;
    const auto report_xcc = [&]() { if (AFFINE && blockIdx.x == 0 && lane == 0) st_flag(a.status + F_XCC0 + (a.xcd_slot & 3u), 0x100u | xcc); };
    if (AFFINE) {                        // (64-thread workgroups: one wave each; see chain_body, also for report_xcc)
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 0xFu;
        if (xcc != ((a.xcd_base + blockIdx.x) & 7u)) {
            if (lane == 0) st_flag(a.status + F_PLACE, 1u);
            report_xcc();
            return;
        }
        wave = (int)((blockIdx.x & ~7u) | xcc);
        if (wave * 32 >= a.n) { report_xcc(); return; }
    }
    const int gi = wave * 32 + (lane & 31);
    const bool active = gi < a.n;
    Geo geo = geo_of(a);
    geo.P = 2;                           // compile-time stride factor for the hot loads
    const Ref gr = game_ref(geo, (size_t)gi);
    // one UNIFORM row base for both half-waves (it becomes a buffer resource): the player's offset goes into the lane offset
    const Ref br = {geo.state, (uint32_t)((size_t)side * geo.stride + (size_t)gi) * 4u, 2 * geo.stride};
    Game<1> g;
    Player& q = g.pl[0];
    uint32_t pd0 = 0, pd1 = 0;
    if (CHAIN) {
        if (active) policy_draw(a, (uint32_t)gi, a.first_step, pd0, pd1);        // while the wave waits for its predecessor
        if (!chain_wait(a, (uint32_t)wave, lane == 0)) { report_xcc(); return; }
    }
    if (active) {
        load_game_words<1>(gr, g, ROLL, MEM);
        load_player(br.s, br.o, br.ws, q, false, true, MEM);
        if (CHAIN) { g.draw0 = pd0; g.draw1 = pd1; }
        else if (ROLL) policy_draw(a, (uint32_t)gi, a.first_step, g.draw0, g.draw1);   // under the loads (see game_load)
        else { g.draw0 = a.rot[gi]; g.draw1 = (uint32_t)a.trans[gi] | ((a.player ? (uint32_t)a.player[gi] : 0u) << 8); }
    }
    s_shapes[lane] = shape_word;
    __builtin_amdgcn_wave_barrier();
    Ctx cx = make_ctx(a, s_shapes, false);
    uint32_t my_lines = 0, my_sent = 0;
    int done = 0, out_reward = 0, out_dead = 0;
    // ONE env-step per launch (launch_game sends fused rollouts to k_game<2>): as a loop over a.steps this kernel needed 199
    // registers per lane instead of ~130 — everything stayed live around the loop's back edge.
    {
        int r = 0, t = 0, acting = 0;
        ResetPrefetch rpf;
        rpf.ok = 0; rpf.seed16 = 0; rpf.word = 0;
        uint32_t sent_start = 0;
        uint32_t wa = 0;
        uint32_t undo_pose = 0, undo_group = 0, undo_draws = 0, undo_cleared = 0;
        bool undo_ran = false;
        Player pre;                                                    // un-chained kernels only: player 1's board before its speculative pass
        if (active) {
            if (ROLL) {
                r = (int)(g.draw0 & 3u); t = (int)(g.draw1 % 10u); acting = (int)(a.first_step % 2ull);
            } else {
                r = (int)(g.draw0 & 3u); t = (int)(g.draw1 & 0xFFu); acting = (int)(g.draw1 >> 8);
            }
            if (ROLL || AUTO) prefetch_reset(cx, episode_seed(a.game_offset + (uint32_t)gi, g.episode + 1), rpf);
            prefetch_next(cx, q, g.seed16, g.status);
            sent_start = q.lines_sent;
            // stage A
            if (!g.round_over && !q.dead && acting == side) play_rt(cx, q, r, t);
            // Player 1's loop-1 pass is speculative (the reference skips it when player 0 died in loop 1, PythonHandle.cpp:153-156,
            // which this lane learns from the shuffle below).  What the pass changes when it clears no row and the new piece
            // fits — nearly always — is the piece (kind, rotation, position, next), the draw counter, now and then the piece
            // group, and 200 ms of combo time: an undo record of three registers.  (A full copy of the board in registers cost
            // ~80 of them in every lane of every step; loading the state again and replaying the keys on EVERY rollback made the
            // slowest wave of most launches ~2 us longer.)  The chained kernel — which has to stay within 128 registers for two
            // launches of 64k games to fit on the device — falls back to that reload where the record does not do; a wave that
            // takes it (1-2 % of them per launch) delays only its own chain.  The un-chained kernels keep the copy in registers
            // instead (they have room): there a launch ends with its SLOWEST wave, and one reload per launch cost every launch
            // 1.4 us (10.0 against 8.6 us, same box: profiles/r03/ab_r02.txt).
            if (!CHAIN && side == 1) pre = q;
            undo_pose = pose_pack(q);
            undo_group = q.pgroup; undo_draws = q.piece_draws;
            undo_cleared = q.lines_cleared; undo_ran = !g.round_over && !q.dead;
            wa = split_settle(cx, g);
        }
        const uint32_t opp_a = __shfl_xor(wa, 32);
        uint32_t wb0 = 0, wb1 = 0;
        if (active) {
            if (side == 1 && (opp_a & XW_DIED)) {
                if (!CHAIN) {
                    q = pre;
                } else if (undo_ran && q.lines_cleared == undo_cleared && !q.dead) {
                    undo_simple_settle(q, undo_pose, undo_group, undo_draws);
                } else if (undo_ran) {
                    // rows were cleared or the new piece did not fit (rare together with a rollback): nothing has been stored by
                    // this launch yet, so the state before this step is still in memory — load it again and replay the keys
                    load_player(br.s, br.o, br.ws, q, false, true, MEM);
                    prefetch_next(cx, q, g.seed16, g.status);
                    if (!g.round_over && !q.dead && acting == side) play_rt(cx, q, r, t);
                    sent_start = q.lines_sent;
                }
                wa = 0;
            }
            if (side == 0) {                                           // stage B0
                const int in = (!(wa & XW_DIED) && (opp_a & XW_RAN) && !(opp_a & XW_DIED)) ? xw_sent(opp_a) : 0;
                wb0 = split_tick(cx, g, a.ms, in);
            }
        }
        const uint32_t x0 = __shfl_xor(wb0, 32);
        if (active && side == 1) {                                     // stage B1
            const int in1 = ((opp_a & XW_RAN) && !(opp_a & XW_DIED)) ? xw_sent(opp_a) : 0;
            if (!g.round_over && in1 > 0) q.incoming = q.incoming + (float)in1 / 1.0f;
            wb1 = split_tick(cx, g, a.ms, (x0 & XW_DIED) ? 0 : xw_sent(x0));
        }
        const uint32_t x1 = __shfl_xor(wb1, 32);
        if (active) {                                                  // stage C
            const uint32_t opp_b = side == 0 ? x1 : x0;
            const int in = (side == 0 && !(opp_b & XW_DIED)) ? xw_sent(opp_b) : 0;
            g.flags = (uint32_t)side;
            done = split_finish(g, in, (opp_b & XW_DEAD_NOW) != 0, (opp_b & XW_ERR) != 0);
            out_reward = q.reward; out_dead = q.dead;                  // what the step reports: the state BEFORE an auto-reset
            if (ROLL) {
                g.steps++;
                if (!q.dead) my_lines += (unsigned)q.reward;
                my_sent += (q.lines_sent - sent_start) & 0xFFFFu;
            }
            if ((ROLL || AUTO) && done) {
                g.episode++;
                reset_split(cx, g, episode_seed(a.game_offset + (uint32_t)gi, g.episode));
            }
        }
    }
    const uint32_t opp_lines = __shfl_xor(my_lines, 32), opp_sent = __shfl_xor(my_sent, 32);
    if (active) {
        store_player(br.s, br.o, br.ws, q, false, true, MEM);
        if (!ROLL) {
            if (a.lines) a.lines[(size_t)side * a.n + gi] = (uint8_t)out_reward;
            if (a.dead) a.dead[(size_t)side * a.n + gi] = (uint8_t)out_dead;
        }
        const uint32_t st = g.status | __shfl_xor(g.status, 32);
        if (side == 0) {
            if (!ROLL && a.done) a.done[gi] = (uint8_t)done;
            g.flags = 0;
            g.add_lines = my_lines + opp_lines;
            g.add_sent = my_sent + opp_sent;
            store_game_words<1>(gr, g, ROLL, MEM);
            report_status(a, st);
        }
    }
    if (CHAIN) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every store (and counter atomic) of this wave has been acknowledged
        if (lane == 0) {                // (as in chain_body: no wait for the acknowledgement)
            if (AFFINE) st_xcd(a.chain + (size_t)wave * CHAIN_STRIDE, a.epoch);
            else st_agent(a.chain + (size_t)wave * CHAIN_STRIDE, a.epoch);
        }
        report_xcc();
    }
    if (OBS) {
        const int pitch = a.H * NCOL / 4, first = wave * 32;
        uint32_t* tile = s_duo_tile + ((size_t)(threadIdx.x >> 6) * 64 * pitch + 3) / 4 * 4;       // (16-byte aligned per wave)
        if (active) {
            const int sl = side == safe_player(a.next_player, gi, 2) ? 0 : 1;
            obs_build(a, tile + (size_t)(sl * 32 + (lane & 31)) * pitch, sl, gi, q.col[0], q.col[1], q.col[2], q.col[3], q.col[4], q.col[5], q.col[6],
                      q.col[7], q.col[8], q.col[9], q.x, q.y, q.next, q.kind, q.inc_count, q.combo_count, q.combo_remaining);
        }
        __syncthreads();
        const int nb = (a.n - first < 32) ? a.n - first : 32;
        if (nb > 0) {
            obs_stream(a, tile, 0, first, nb, lane);
            obs_stream(a, tile + (size_t)32 * pitch, 1, first, nb, lane);
        }
    }
}
template <int MODE, bool CHAIN = false, bool OBS = false>
__global__ __launch_bounds__(CHAIN ? 64 : 256) void k_duo(KArgs a) { duo_body<MODE, CHAIN, OBS, false>(a); }
__global__ __launch_bounds__(64) void k_duo_affine(KArgs a) { duo_body<M_ROLLOUT, true, false, true>(a); }

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

template <int P, bool TINT>
__global__ __launch_bounds__(256) void k_observe(Geo geo, int n, const int32_t* idx, int H, tetris_record* rec, uint8_t* round_over,
                                                 int8_t* last_winner) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) observe_body<P, TINT>(geo, i, idx, H, d_shape_table.s, rec, round_over, last_winner);
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
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        if ((((uintptr_t)dst) & 15u) == 0) {
            const uint32_t whole = words & ~3u;
            for (uint32_t g = 4u * threadIdx.x; g < whole; g += 4u * BLOCK)
                __builtin_nontemporal_store(*reinterpret_cast<const u32x4*>(s_words + g), reinterpret_cast<u32x4*>(dst + g));
            if (threadIdx.x < words - whole) dst[whole + threadIdx.x] = s_words[whole + threadIdx.x];
        } else
            for (uint32_t g = threadIdx.x; g < words; g += BLOCK) dst[g] = s_words[g];
    }
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
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
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

template <int P>
__global__ __launch_bounds__(64) void k_actions(Geo geo, int n, const int32_t* idx, const uint8_t* player,
                                                int H, uint8_t* count, uint8_t* lens, uint8_t* keys, int max_lists, int max_keys,
                                                uint32_t* status) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (size_t)n * 40)
        actions_body<P>(geo, t, idx, player, H, d_shape_table.s, count, lens, keys, max_lists, max_keys, status);
}

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
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
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

__global__ __launch_bounds__(256) void k_snapshot(Geo geo, int n, const int32_t* idx, uint32_t* blob, int restore) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (size_t)n * (NGWORDS + geo.P * geo.nw)) snapshot_body(geo, t, idx, blob, restore);
}

__global__ __launch_bounds__(256) void k_set_dead(Geo geo, int n, const int32_t* idx, const uint8_t* dead /*[n][P]*/) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n * geo.P) set_dead_body(geo, t, idx, dead);
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

// ============================================================================ host side
// (headers of this translation unit only, in dependency order: they launch the kernels above)

#include "tetris_lib_batch.h"
#include "tetris_lib_rollout.h"
#include "tetris_lib_core.h"
#include "tetris_lib_agent.h"
