// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// The CPU test harness with the planning, heuristic-policy, deltas and acting entry points (harness_act.cpp, included whole)
// plus tetris_traj_record_dev and tetris_traj_advantages_dev of include/tetris_hip.h as plain host loops over the same bodies
// (drl-tetris_amd/csrc/tetris_traj.h: traj_record_game, traj_advantages_game).  "Device" pointers are host pointers here.
// __graft_entry__.build_harness compiles this file into libtetris_cpu_harness.so.
#include "harness_act.cpp"

#include "../../drl-tetris_amd/csrc/tetris_traj.h"

// the argument checks of the product (tetris_hip.hip: traj_record_args, traj_adv_args), then the kernel arguments
static int traj_record_args(tetris_batch* b, const tetris_traj* traj, int row, const tetris_act_eval* e, const uint8_t* d_done,
                            const uint8_t* d_dead, TrajRecordArgs& ra) {
    if (!traj || !e) return fail(TETRIS_E_ARG, "the window or the argument struct is NULL");
    if (b->split) return fail(TETRIS_E_ARG, "tetris_traj_record_dev is not available on split batches");
    if (b->P > 2) return fail(TETRIS_E_ARG, "the reward is defined for one or two players (tetris_environment.py:135-144)");
    if (!traj->d_action || !traj->d_prob || !traj->d_value || !traj->d_reward || !traj->d_done) return fail(TETRIS_E_ARG, "an array of the window is NULL");
    if (row < 0 || row >= traj->capacity) return fail(TETRIS_E_ARG, "row outside the window");
    if (!e->d_rot || !e->d_trans || !e->d_piece || !e->d_eval) return fail(TETRIS_E_ARG, "rot/trans/piece/eval of the acting call are NULL");
    if (!d_done || !d_dead) return fail(TETRIS_E_ARG, "done/dead are NULL");
    const size_t n = (size_t)b->N, at = (size_t)row * n;
    ra.n = b->N; ra.n_players = b->P;
    ra.rot = e->d_rot; ra.trans = e->d_trans; ra.piece = e->d_piece; ra.player = e->d_player;
    ra.eval = e->d_eval; ra.value = e->d_value;
    ra.done = d_done; ra.dead = d_dead;
    ra.action = traj->d_action + at * 4; ra.prob = traj->d_prob + at;
    ra.value0 = traj->d_value + at; ra.value1 = traj->d_value + (size_t)traj->capacity * n + at;
    ra.reward = traj->d_reward + at; ra.done_out = traj->d_done + at;
    return TETRIS_OK;
}

static int traj_adv_args(tetris_batch* b, const tetris_traj* traj, int rows, float gamma, float lambda_adv, float lambda_value,
                         const float* d_boot, float* d_adv, float* d_target, uint8_t* d_closed, TrajAdvArgs& aa) {
    if (!traj) return fail(TETRIS_E_ARG, "the window is NULL");
    if (!traj->d_value || !traj->d_reward || !traj->d_done) return fail(TETRIS_E_ARG, "value/reward/done of the window are NULL");
    if (!d_adv || !d_target) return fail(TETRIS_E_ARG, "adv/target are NULL");
    if (rows < 1 || rows > traj->capacity) return fail(TETRIS_E_ARG, "rows outside [1, capacity]");
    aa.n = b->N; aa.rows = rows;
    aa.plane = (size_t)traj->capacity * (size_t)b->N;
    aa.value = traj->d_value; aa.reward = traj->d_reward; aa.done = traj->d_done; aa.boot = d_boot;
    aa.gamma = gamma; aa.lambda_adv = lambda_adv; aa.lambda_value = lambda_value;
    aa.adv = d_adv; aa.target = d_target; aa.closed = d_closed;
    return TETRIS_OK;
}

extern "C" {

int tetris_traj_record_dev(tetris_batch* b, const tetris_traj* traj, int row, const tetris_act_eval* e, const uint8_t* d_done,
                           const uint8_t* d_dead) {
    TrajRecordArgs ra;
    int rc = traj_record_args(b, traj, row, e, d_done, d_dead, ra); if (rc) return rc;
    for (int i = 0; i < b->N; i++) traj_record_game(ra, i);
    return TETRIS_OK;
}

int tetris_traj_advantages_dev(tetris_batch* b, const tetris_traj* traj, int rows, float gamma, float lambda_adv,
                               float lambda_value, const float* d_boot, float* d_adv, float* d_target, uint8_t* d_closed) {
    TrajAdvArgs aa;
    int rc = traj_adv_args(b, traj, rows, gamma, lambda_adv, lambda_value, d_boot, d_adv, d_target, d_closed, aa); if (rc) return rc;
    for (int i = 0; i < b->N; i++) traj_advantages_game(aa, i);
    return TETRIS_OK;
}

}  // extern "C"
