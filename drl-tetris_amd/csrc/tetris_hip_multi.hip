// libtetris_hip.so, second translation unit: the step kernel for three and four players per game (tetris_game_kernel.h) and,
// beside it, the planning kernels (k_plan_sim, k_plan_step; tetris_plan.h) and the policy step kernels (k_policy_step;
// tetris_policy.h) for three and four players.  Nothing else lives here; the two files are compiled in parallel
// (__graft_entry__.build_hip).
#include "tetris_game_kernel.h"

template <int P, bool TINT>
static int launch_mode(int mode, dim3 grid, dim3 block, hipStream_t st, const KArgs& a) {
    switch (mode) {
#define TE_CASE(M) case M: hipLaunchKernelGGL((k_game<P, M, TINT>), grid, block, 0, st, a); return 0
        TE_CASE(M_INIT); TE_CASE(M_RESET); TE_CASE(M_MAKE); TE_CASE(M_FINISH); TE_CASE(M_STEP_KEYS); TE_CASE(M_STEP_RT);
        TE_CASE(M_ROLLOUT); TE_CASE(M_STEP_RT_AUTO); TE_CASE(M_RESET_SCHED);
#undef TE_CASE
        default: return -1;
    }
}

__attribute__((visibility("hidden"))) int tetris_launch_game_multi(int n_players, int tint, int mode, dim3 grid, dim3 block, hipStream_t st, const KArgs& a) {
    int rc = -1;
    with_shape<3, 4>(n_players, tint != 0, [&](auto P, auto TINT) { rc = launch_mode<P(), TINT()>(mode, grid, block, st, a); });
    return rc;
}

__attribute__((visibility("hidden"))) int tetris_launch_plan_multi(int n_players, int tint, int which, dim3 grid, hipStream_t st, const PlanArgs& pa, int fin) {
    return with_shape<3, 4>(n_players, tint != 0, [&](auto P, auto TINT) { launch_plan<P(), TINT()>(which, grid, st, pa, fin); }) ? 0 : -1;
}

__attribute__((visibility("hidden"))) int tetris_launch_policy_multi(int n_players, int tint, int which, dim3 grid, hipStream_t st, const PolicyArgs& pa) {
    return with_shape<3, 4>(n_players, tint != 0, [&](auto P, auto TINT) { launch_policy_step<P(), TINT()>(which, grid, st, pa); }) ? 0 : -1;
}
