// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// The CPU test harness with the planning, heuristic-policy and deltas entry points (harness_deltas.cpp, included whole) plus
// tetris_select_eval_dev, tetris_step_eval_dev and tetris_step_eval_observe_dev of include/tetris_hip.h as plain host loops over
// the same body (drl-tetris_amd/csrc/tetris_act.h: act_select_game).  "Device" pointers are host pointers here.
// __graft_entry__.build_harness compiles this file into libtetris_cpu_harness.so.
#include "harness_deltas.cpp"

#include "../../drl-tetris_amd/csrc/tetris_act.h"

// the argument checks of the product (tetris_hip.hip: act_args), then the kernel arguments
static int act_args(tetris_batch* b, const tetris_act_eval* e, const char* what, ActArgs& aa) {
    if (!e) return fail(TETRIS_E_ARG, "the argument struct is NULL");
    if (b->split) return fail(TETRIS_E_ARG, (std::string(what) + " is not available on split batches").c_str());
    if (!e->d_action_eval || !e->d_rot || !e->d_trans) return fail(TETRIS_E_ARG, "action_eval/rot/trans are NULL");
    if (e->n_pieces != 1 && e->n_pieces != 7) return fail(TETRIS_E_ARG, "n_pieces must be 1 or 7");
    if (e->d_state_eval && e->n_values != 1 && e->n_values != 7 && e->n_values != 8) return fail(TETRIS_E_ARG, "n_values must be 1, 7 or 8");
    if (e->d_value && !e->d_state_eval) return fail(TETRIS_E_ARG, "value needs state_eval");
    if (e->mode < TETRIS_ACT_ARGMAX || e->mode > TETRIS_ACT_EPSILON) return fail(TETRIS_E_ARG, "unknown mode");
    if (e->flags & ~(TETRIS_ACT_F16 | TETRIS_ACT_VALUE_F16)) return fail(TETRIS_E_ARG, "unknown flag");
    if (e->mode == TETRIS_ACT_RANK && !e->table) return fail(TETRIS_E_ARG, "the RANK mode needs a table");
    if (e->d_entropy && e->mode != TETRIS_ACT_PI) return fail(TETRIS_E_ARG, "entropy is an output of the PI mode");
    if (((uintptr_t)e->d_action_eval) & 15u) return fail(TETRIS_E_ARG, "action_eval must be 16-byte aligned");
    memset(&aa, 0, sizeof aa);
    aa.a = base_args(b, b->N, nullptr);
    aa.a.steps = 1;
    aa.player = e->d_player;
    aa.action_eval = e->d_action_eval; aa.state_eval = e->d_state_eval;
    aa.K = e->n_pieces; aa.V = e->d_state_eval ? e->n_values : 1;
    aa.eval_f16 = (e->flags & TETRIS_ACT_F16) ? 1 : 0; aa.value_f16 = (e->flags & TETRIS_ACT_VALUE_F16) ? 1 : 0;
    aa.mode = e->mode;
    aa.seed = e->sample_seed; aa.draw_lo = (uint32_t)e->draw; aa.draw_hi = (uint32_t)(e->draw >> 32);
    aa.epsilon = e->epsilon;
    if (e->mode == TETRIS_ACT_RANK) memcpy(aa.table, e->table, sizeof aa.table);
    aa.rot = e->d_rot; aa.trans = e->d_trans; aa.piece = e->d_piece;
    aa.eval = e->d_eval; aa.value = e->d_value; aa.entropy = e->d_entropy;
    return TETRIS_OK;
}

extern "C" {

int tetris_select_eval_dev(tetris_batch* b, const tetris_act_eval* e) {
    ActArgs aa;
    int rc = act_args(b, e, "tetris_select_eval_dev", aa); if (rc) return rc;
    if ((rc = finish_call(b))) return rc;
    for (int i = 0; i < b->N; i++) act_select_game(aa, i);
    return TETRIS_OK;
}

int tetris_step_eval_dev(tetris_batch* b, const tetris_act_eval* e, int ms, int flags, uint8_t* done, uint8_t* lines, uint8_t* dead) {
    if (flags & ~TETRIS_STEP_AUTO_RESET) return fail(TETRIS_E_ARG, "unknown flag");
    int rc = tetris_select_eval_dev(b, e); if (rc) return rc;
    return tetris_step_rt_dev_ex(b, e->d_rot, e->d_trans, e->d_player, ms, done, lines, dead, flags);
}

int tetris_step_eval_observe_dev(tetris_batch* b, const tetris_act_eval* e, int ms, int flags, uint8_t* done, uint8_t* lines, uint8_t* dead,
                                 const uint8_t* next_player, uint8_t* visual, uint8_t* vector, uint8_t* obs_piece) {
    if (!visual || !vector || !obs_piece) return fail(TETRIS_E_ARG, "visual/vector/piece are NULL");
    if (flags & ~TETRIS_STEP_AUTO_RESET) return fail(TETRIS_E_ARG, "unknown flag");
    if (b->P > 2) return fail(TETRIS_E_ARG, "the packed observation is defined for one or two players (own / opponent's board: state_unpack.py:88-137)");
    int rc = tetris_select_eval_dev(b, e); if (rc) return rc;
    return tetris_step_rt_observe_dev(b, e->d_rot, e->d_trans, e->d_player, ms, done, lines, dead, flags, next_player, visual, vector, obs_piece);
}

}  // extern "C"
