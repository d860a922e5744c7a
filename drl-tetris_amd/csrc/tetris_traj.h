// Kernel bodies of the trajectory windows (include/tetris_hip.h: tetris_traj_record_dev, tetris_traj_advantages_dev): the
// worker-side arithmetic between perform_action and the data packet (drl_tetris/worker.py:103-112) — store_experience's row of
// a per-env trajectory, and sventon_trajectory.process_trajectory's adv_and_targets (agents/datatypes/trajectory.py:56-86,
// 111-141) as that call uses it: the TD errors on v(s | piece), the target on mean v.
//
// `__host__ __device__` like tetris_act.h: tetris_hip.hip wraps these in gfx950 kernels (k_traj_record, k_traj_advantages,
// tetris_dev_traj.h), tests/cpu_harness/harness_lib_agent.h in plain host loops.
//
// The backward recurrence is one game's state in six registers (TrajScan) and one function per row (traj_scan_row) that takes
// the row's four inputs as values: the kernel feeds it from a workgroup's LDS tiles, the host from the window itself.  Every
// operation is a float32 operation in the order the header writes down; the builds use -ffp-contract=off and the correctly
// rounded division, so host and device give the same bits.
#pragma once
#include "tetris_kernels.h"

namespace te {

constexpr int TRAJ_BLOCK = 64;      // games per workgroup: one lane of the scanning wave each
constexpr int TRAJ_TILE = 16;       // rows per LDS tile

struct TrajRecordArgs {
    int n, n_players;
    const uint8_t* rot;             // [N] the outputs of the acting call
    const uint8_t* trans;
    const uint8_t* piece;
    const uint8_t* player;          // [N] or NULL (player 0; clamped)
    const float* eval;              // [N]
    const float* value;             // [2][N] or NULL (zeros)
    const uint8_t* done;            // [N] the step's outputs
    const uint8_t* dead;            // [P][N]
    uint8_t* action;                // row `row` of the window: [N][4]
    float* prob;                    // [N]
    float* value0;                  // [N] of value[0]
    float* value1;                  // [N] of value[1]
    float* reward;                  // [N]
    uint8_t* done_out;              // [N]
};

struct TrajAdvArgs {
    int n, rows;
    size_t plane;                   // floats between value[0] and value[1]: capacity * N
    const float* value;             // [2][T][N]
    const float* reward;            // [T][N]
    const uint8_t* done;            // [T][N]
    const float* boot;              // [N] or NULL
    float gamma, lambda_adv, lambda_value;
    float* adv;                     // [rows][N]
    float* target;                  // [rows][N]
    uint8_t* closed;                // [rows][N] or NULL
};

// tetris_environment.reward_fcn without extra_rewards (tetris_environment.py:135-144) for the acting player p
TE_HD float traj_reward(const uint8_t* dead, int i, int n, int n_players, int p, bool done) {
    if (!done) return 0.0f;
    const int me = dead[(size_t)p * n + i] != 0 ? 1 : 0;
    const int you = n_players > 1 ? (dead[(size_t)(1 - p) * n + i] != 0 ? 1 : 0) : 0;
    return (me && you) ? -1.0f : (float)(you - me);
}

// row `row` of game i
TE_HD void traj_record_game(const TrajRecordArgs& ra, int i) {
    const int p = safe_player(ra.player, i, ra.n_players);
    uint8_t* a = ra.action + (size_t)i * 4;
    a[0] = ra.rot[i]; a[1] = ra.trans[i]; a[2] = ra.piece[i]; a[3] = (uint8_t)p;
    ra.prob[i] = ra.eval[i];
    ra.value0[i] = ra.value ? ra.value[i] : 0.0f;
    ra.value1[i] = ra.value ? ra.value[(size_t)ra.n + i] : 0.0f;
    const uint8_t d = ra.done[i];
    ra.done_out[i] = d;
    ra.reward[i] = traj_reward(ra.dead, i, ra.n, ra.n_players, p, d != 0);
}

// one game's state of the backward walk
struct TrajScan {
    float A1, A2, W1, W2, vnext;
    uint32_t seen;
};

TE_HD void traj_scan_begin(TrajScan& s, float boot) {
    s.A1 = s.A2 = s.W1 = s.W2 = 0.0f;
    s.vnext = boot;
    s.seen = 0u;
}

// one row, in the header's order of operations (trajectory.py:116-126, 138)
TE_HD void traj_scan_row(TrajScan& s, const TrajAdvArgs& aa, float reward, float v0, float v1, bool done, float& adv, float& target) {
    if (done) { s.A1 = s.A2 = s.W1 = s.W2 = 0.0f; s.seen = 1u; }
    const float td = (reward + (aa.gamma * s.vnext) * (done ? 0.0f : 1.0f)) - v0;
    s.A1 = s.A1 * (aa.gamma * aa.lambda_adv) + td;
    s.W1 = s.W1 * aa.lambda_adv + 1.0f;
    s.A2 = s.A2 * (aa.gamma * aa.lambda_value) + td;
    s.W2 = s.W2 * aa.lambda_value + 1.0f;
    adv = ((s.A1 + v0) - v1) / s.W1;
    target = v1 + ((s.A2 + v0) - v1) / s.W2;
    s.vnext = v0;
}

// Serial form of game i (CPU harness; the kernel feeds the same function from LDS)
TE_HD void traj_advantages_game(const TrajAdvArgs& aa, int i) {
    TrajScan s;
    traj_scan_begin(s, aa.boot ? aa.boot[i] : 0.0f);
    for (int t = aa.rows - 1; t >= 0; t--) {
        const size_t at = (size_t)t * aa.n + i;
        float adv, target;
        traj_scan_row(s, aa, aa.reward[at], aa.value[at], aa.value[aa.plane + at], aa.done[at] != 0, adv, target);
        aa.adv[at] = adv;
        aa.target[at] = target;
        if (aa.closed) aa.closed[at] = (uint8_t)s.seen;
    }
}

}  // namespace te
