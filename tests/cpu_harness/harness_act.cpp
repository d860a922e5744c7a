// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// The CPU test harness with the planning, heuristic-policy and deltas entry points (harness_deltas.cpp, included whole) plus
// tetris_select_eval_dev, tetris_step_eval_dev and tetris_step_eval_observe_dev of include/tetris_hip.h as plain host loops over
// the same body (drl-tetris_amd/csrc/tetris_act.h: act_select_game).  "Device" pointers are host pointers here.
// __graft_entry__.build_harness compiles this file into libtetris_cpu_harness.so.  The checks and act_args are the product's
// (tetris_host.h).
#include "harness_deltas.cpp"

extern "C" {

int tetris_select_eval_dev(tetris_batch* b, const tetris_act_eval* e) {
    ActArgs aa;
    int rc = act_args(shape_of(b), e, "tetris_select_eval_dev", aa);
    if (rc || (rc = finish_call(b))) return rc;
    aa.a = base_args(b, b->N, nullptr);
    aa.a.steps = 1;
    for (int i = 0; i < b->N; i++) act_select_game(aa, i);
    return TETRIS_OK;
}

int tetris_step_eval_dev(tetris_batch* b, const tetris_act_eval* e, int ms, int flags, uint8_t* done, uint8_t* lines, uint8_t* dead) {
    int rc = step_eval_check(flags);
    if (rc || (rc = tetris_select_eval_dev(b, e))) return rc;
    return tetris_step_rt_dev_ex(b, e->d_rot, e->d_trans, e->d_player, ms, done, lines, dead, flags);
}

int tetris_step_eval_observe_dev(tetris_batch* b, const tetris_act_eval* e, int ms, int flags, uint8_t* done, uint8_t* lines, uint8_t* dead,
                                 const uint8_t* next_player, uint8_t* visual, uint8_t* vector, uint8_t* obs_piece) {
    int rc = step_eval_observe_check(shape_of(b), flags, visual, vector, obs_piece);
    if (rc || (rc = tetris_select_eval_dev(b, e))) return rc;
    return tetris_step_rt_observe_dev(b, e->d_rot, e->d_trans, e->d_player, ms, done, lines, dead, flags, next_player, visual, vector, obs_piece);
}

}  // extern "C"
