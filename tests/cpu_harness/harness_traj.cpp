// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// The CPU test harness with the planning, heuristic-policy, deltas and acting entry points (harness_act.cpp, included whole)
// plus tetris_traj_record_dev and tetris_traj_advantages_dev of include/tetris_hip.h as plain host loops over the same bodies
// (drl-tetris_amd/csrc/tetris_traj.h: traj_record_game, traj_advantages_game).  "Device" pointers are host pointers here.
// __graft_entry__.build_harness compiles this file into libtetris_cpu_harness.so.  The checks and traj_record_args / traj_adv_args are
// the product's (tetris_host.h).
#include "harness_act.cpp"

extern "C" {

int tetris_traj_record_dev(tetris_batch* b, const tetris_traj* traj, int row, const tetris_act_eval* e, const uint8_t* d_done,
                           const uint8_t* d_dead) {
    TrajRecordArgs ra;
    int rc = traj_record_args(shape_of(b), traj, row, e, d_done, d_dead, ra); if (rc) return rc;
    for (int i = 0; i < b->N; i++) traj_record_game(ra, i);
    return TETRIS_OK;
}

int tetris_traj_advantages_dev(tetris_batch* b, const tetris_traj* traj, int rows, float gamma, float lambda_adv,
                               float lambda_value, const float* d_boot, float* d_adv, float* d_target, uint8_t* d_closed) {
    TrajAdvArgs aa;
    int rc = traj_adv_args(shape_of(b), traj, rows, gamma, lambda_adv, lambda_value, d_boot, d_adv, d_target, d_closed, aa); if (rc) return rc;
    for (int i = 0; i < b->N; i++) traj_advantages_game(aa, i);
    return TETRIS_OK;
}

}  // extern "C"
