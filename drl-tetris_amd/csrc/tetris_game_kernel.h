// What both translation units compile: the per-translation-unit shape table and the step kernels that exist for every player
// count: the general step kernel (all players of a game in one lane), the planning kernels and the policy step kernels.
// tetris_hip.hip instantiates them for one and two players (and holds every other kernel, in its tetris_dev_*.h headers, and the
// C ABI); tetris_hip_multi.hip for three and four: 36 more instantiations of k_game alone, compiled in parallel with the first
// file because they double its compile time.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "tetris_kernels.h"
#include "tetris_plan.h"
#include "tetris_policy.h"
#include "tetris_host.h"          // (with_shape; and every other tetris_*.h the first translation unit's kernels wrap)

using namespace te;

static __device__ const ShapeTable d_shape_table = make_shape_table();

template <int P, int MODE, bool TINT>
__global__ __launch_bounds__(256) void k_game(KArgs a) {
    // Shape table in LDS, one private 128-byte copy per wave: no workgroup barrier, so a wave starts computing as soon as
    // the state words it needs first have arrived instead of waiting for all loads of all four waves.  The table load is
    // issued before the state loads (loads return in order), and ds_write -> ds_read order within a wave is by lgkmcnt.
    __shared__ __attribute__((aligned(16))) uint32_t s_shapes_all[4][SHAPE_WORDS];
    uint32_t* s_shapes = s_shapes_all[threadIdx.x >> 6];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = lane_active(a, i);
    LaneCounters cnt = {0, 0, 0, 0};                   // (per-lane sums feed the CPU test harness only)
    const uint32_t shape_word = d_shape_table.s[threadIdx.x & 63];
    Game<P> g;
    if (active) game_load<P, MODE, TINT>(a, i, g);
    s_shapes[threadIdx.x & 63] = shape_word;
    __builtin_amdgcn_wave_barrier();
    if (active) game_run<P, MODE, TINT>(a, i, s_shapes, g, cnt);
}

// The planning kernels (tetris_plan.h), one wave per workgroup with its own LDS copy of the shape table.
// k_plan_sim: grid (ceil(N / 64), max_lists): wave = 64 consecutive games of one list index k, so that a wave whose k is past
// every count in it leaves at once and the state loads and the column stores of a wave are coalesced rows.
template <int P, bool TINT>
__global__ __launch_bounds__(64) void k_plan_sim(PlanArgs pa, int fin) {
    __shared__ uint32_t s_shapes[SHAPE_WORDS];
    s_shapes[threadIdx.x] = d_shape_table.s[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y;
    if (i < pa.a.n) plan_sim_lane<P, TINT>(pa, i, k, fin != 0, s_shapes, true);
}
// k_plan_step: one lane per game
template <int P, bool TINT, bool AUTO>
__global__ __launch_bounds__(64) void k_plan_step(PlanArgs pa) {
    __shared__ uint32_t s_shapes[SHAPE_WORDS];
    s_shapes[threadIdx.x] = d_shape_table.s[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < pa.a.n) plan_step_lane<P, TINT, AUTO>(pa, i, s_shapes, true);
}
template <int P, bool TINT>
static void launch_plan(int which, dim3 grid, hipStream_t st, const PlanArgs& pa, int fin) {
    if (which == 0) hipLaunchKernelGGL((k_plan_sim<P, TINT>), grid, dim3(64), 0, st, pa, fin);
    else if (which == 1) hipLaunchKernelGGL((k_plan_step<P, TINT, false>), grid, dim3(64), 0, st, pa);
    else hipLaunchKernelGGL((k_plan_step<P, TINT, true>), grid, dim3(64), 0, st, pa);
}

// The step kernels of the heuristic policy (tetris_policy.h), one lane per game, one wave per workgroup.  ROLL: the rollout's
// step(s) with counters; FROM_SCORES: the choice is read from the scores k_policy_eval left (spread mapping), otherwise the
// lane evaluates its own 40 candidates (fused launches).
template <int P, bool TINT, bool ROLL, bool AUTO, bool FROM_SCORES>
__global__ __launch_bounds__(64) void k_policy_step(PolicyArgs pa) {
    __shared__ uint32_t s_shapes[SHAPE_WORDS];
    s_shapes[threadIdx.x] = d_shape_table.s[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < pa.a.n) policy_step_lane<P, TINT, ROLL, AUTO, FROM_SCORES>(pa, i, s_shapes, true);
}
// which: 0 step, 1 step with auto-reset, 2 one rollout step from the scores, 3 fused rollout steps (lane mapping)
template <int P, bool TINT>
static void launch_policy_step(int which, dim3 grid, hipStream_t st, const PolicyArgs& pa) {
    if (which == 0) hipLaunchKernelGGL((k_policy_step<P, TINT, false, false, true>), grid, dim3(64), 0, st, pa);
    else if (which == 1) hipLaunchKernelGGL((k_policy_step<P, TINT, false, true, true>), grid, dim3(64), 0, st, pa);
    else if (which == 2) hipLaunchKernelGGL((k_policy_step<P, TINT, true, true, true>), grid, dim3(64), 0, st, pa);
    else hipLaunchKernelGGL((k_policy_step<P, TINT, true, true, false>), grid, dim3(64), 0, st, pa);
}

// launches k_game<P, mode, tint> for P = 3, 4 (tetris_hip_multi.hip)
__attribute__((visibility("hidden"))) int tetris_launch_game_multi(int n_players, int tint, int mode, dim3 grid, dim3 block, hipStream_t stream, const te::KArgs& a);
// launches the planning kernels for P = 3, 4 (tetris_hip_multi.hip); which: 0 simulate, 1 step, 2 step with auto-reset
__attribute__((visibility("hidden"))) int tetris_launch_plan_multi(int n_players, int tint, int which, dim3 grid, hipStream_t stream, const te::PlanArgs& pa, int fin);
// launches the policy step kernels for P = 3, 4 (tetris_hip_multi.hip); which: as launch_policy_step
__attribute__((visibility("hidden"))) int tetris_launch_policy_multi(int n_players, int tint, int which, dim3 grid, hipStream_t stream, const te::PolicyArgs& pa);
