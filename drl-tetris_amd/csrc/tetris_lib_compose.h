// The entry points that are nothing but a fixed sequence of calls to other entry points, or to helpers both sides have (check_batch,
// shape_of, create_impl, rollout_counters_begin / _end, the checks of tetris_host.h).  No HIP in here: tetris_hip.hip and
// tests/cpu_harness/harness.cpp both include it, last, so the CPU suite runs these lines as they ship.

// The work of a loss head behind its argument rules.  The product has launch_loss(tetris_batch*, LossArgs&) (tetris_lib_agent.h:
// the gfx950 kernels), which as a plain function is preferred to this template and leaves it uninstantiated: the library holds no
// CPU path.  A build whose host side defines none — the CPU harness, whose "device" memory is host memory — gets the serial form of
// the same bodies (tetris_host.h: loss_run_serial).
template <class B>
static int launch_loss(B*, LossArgs& la) { return loss_run_serial(la); }
// (the k-step target estimator likewise: launch_kstep of tetris_lib_agent.h, or kstep_run_serial; and the gather of a step list:
// launch_traj_batch of tetris_lib_agent.h, or traj_batch_run_serial)
template <class B>
static int launch_kstep(B*, KstepArgs& a) { return kstep_run_serial(a); }
template <class B>
static int launch_traj_batch(B* b, const TrajBatchArgs& ba) { return traj_batch_run_serial(b->P, ba); }
// (and the output heads: launch_head of tetris_lib_agent.h, or head_run_serial)
template <class B>
static int launch_head(B*, const HeadArgs& h) { return head_run_serial(h); }
// (and the network inputs: launch_input of tetris_lib_agent.h, or input_run_serial)
template <class B>
static int launch_input(B*, const InputArgs& ia) { return input_run_serial(ia); }
// (and the keyboard convolution: launch_kbd of tetris_lib_agent.h, or kbd_run_serial)
template <class B>
static int launch_kbd(B*, const KbdArgs& a) { return kbd_run_serial(a); }
// (and the residual layer: launch_res of tetris_lib_agent.h, or res_run_serial)
template <class B>
static int launch_res(B*, const ResArgs& a) { return res_run_serial(a); }

extern "C" {

const char* tetris_last_error(void) { return last_error(); }
int tetris_record_size(void) { return (int)sizeof(tetris_record); }
int tetris_layout_words(void) { return NWORDS; }
int tetris_snapshot_words(const tetris_batch* b) { return b ? NGWORDS + b->P * b->nw : 0; }

int tetris_create(tetris_batch** out, int n_games, int n_players, int height, int width, const uint8_t piece_map[7],
                  int device, const int16_t* seeds) {
    return create_impl(out, n_games, n_players, height, width, piece_map, device, seeds, 0, 0);
}

int tetris_create_ex(tetris_batch** out, int n_games, int n_players, int height, int width, const uint8_t piece_map[7], int device,
                     const int16_t* seeds, int flags) {
    return create_impl(out, n_games, n_players, height, width, piece_map, device, seeds, 0, 0, flags);
}

int tetris_create_split(tetris_batch** out, int n_games, int side, int height, int width, const uint8_t piece_map[7], int device,
                        const int16_t* seeds) {
    return create_impl(out, n_games, 1, height, width, piece_map, device, seeds, 1, side);
}

int tetris_step_rt_dev(tetris_batch* b, const uint8_t* d_rot, const uint8_t* d_trans, const uint8_t* d_player, int ms,
                       uint8_t* d_done, uint8_t* d_lines, uint8_t* d_dead) {
    return tetris_step_rt_dev_ex(b, d_rot, d_trans, d_player, ms, d_done, d_lines, d_dead, 0);
}

int tetris_enumerate_drops_dev(tetris_batch* b, const int32_t* d_idx, int n, const uint8_t* d_player, uint8_t* d_valid,
                               int8_t* d_land_y, uint8_t* d_cleared, uint32_t* d_after) {
    return tetris_enumerate_drops_dev_ex(b, d_idx, n, d_player, d_valid, d_land_y, d_cleared, d_after, 0);
}

int tetris_step_eval_dev(tetris_batch* b, const tetris_act_eval* e, int ms, int flags, uint8_t* d_done, uint8_t* d_lines,
                         uint8_t* d_dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = step_eval_check(flags))) return rc;
    // two launches: the step fused behind the selection in one kernel took 1.6-2.2 times as long
    if ((rc = tetris_select_eval_dev(b, e))) return rc;
    return tetris_step_rt_dev_ex(b, e->d_rot, e->d_trans, e->d_player, ms, d_done, d_lines, d_dead, flags);
}

int tetris_step_eval_observe_dev(tetris_batch* b, const tetris_act_eval* e, int ms, int flags, uint8_t* d_done, uint8_t* d_lines,
                                 uint8_t* d_dead, const uint8_t* d_next_player, uint8_t* d_visual, uint8_t* d_vector,
                                 uint8_t* d_obs_piece) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = step_eval_observe_check(shape_of(b), flags, d_visual, d_vector, d_obs_piece))) return rc;
    if ((rc = tetris_select_eval_dev(b, e))) return rc;
    return tetris_step_rt_observe_dev(b, e->d_rot, e->d_trans, e->d_player, ms, d_done, d_lines, d_dead, flags, d_next_player,
                                      d_visual, d_vector, d_obs_piece);
}

int tetris_step_lists_eval_dev(tetris_batch* b, const tetris_plan_eval* e, const uint8_t* d_lens, const uint8_t* d_keys, int max_keys,
                               int ms, int flags, uint8_t* d_done, uint8_t* d_lines, uint8_t* d_dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = step_lists_eval_check(shape_of(b), e, d_lens, d_keys, max_keys, flags))) return rc;
    if ((rc = tetris_select_lists_dev(b, e))) return rc;
    return tetris_step_lists_dev(b, e->d_player, e->d_choice, e->d_count, d_lens, d_keys, e->max_lists, max_keys, ms, flags, d_done,
                                 d_lines, d_dead);
}

int tetris_ppo_loss_dev(tetris_batch* b, const tetris_ppo_loss* l) {
    int rc = check_batch(b);
    if (rc) return rc;
    LossArgs la;
    if ((rc = ppo_loss_args(l, la))) return rc;
    return launch_loss(b, la);
}

int tetris_dqn_loss_dev(tetris_batch* b, const tetris_dqn_loss* l) {
    int rc = check_batch(b);
    if (rc) return rc;
    LossArgs la;
    if ((rc = dqn_loss_args(l, la))) return rc;
    return launch_loss(b, la);
}

int tetris_plan_loss_dev(tetris_batch* b, const tetris_traj_plan* plan, const tetris_plan_loss* l) {
    int rc = check_batch(b);
    if (rc) return rc;
    LossArgs la;
    if ((rc = plan_loss_args(shape_of(b), plan, l, la))) return rc;
    return launch_loss(b, la);
}

int tetris_replay_gather_steps_dev(tetris_batch* b, const tetris_replay* rp, const int32_t* d_index, int M, uint64_t step_mask,
                                   const tetris_traj_batch* out) {
    int rc = check_batch(b);
    if (rc) return rc;
    TrajBatchArgs ba;
    if ((rc = replay_gather_steps_args(shape_of(b), rp, d_index, M, step_mask, out, ba))) return rc;
    return launch_traj_batch(b, ba);
}

int tetris_kstep_target_dev(tetris_batch* b, const tetris_kstep_target* t) {
    int rc = check_batch(b);
    if (rc) return rc;
    KstepArgs a;
    if ((rc = kstep_target_args(t, a))) return rc;
    return launch_kstep(b, a);
}

int tetris_q_head_dev(tetris_batch* b, const tetris_q_head* q) {
    int rc = check_batch(b);
    if (rc) return rc;
    HeadArgs h;
    if ((rc = q_head_args(q, 0, h))) return rc;
    return launch_head(b, h);
}

int tetris_q_head_grad_dev(tetris_batch* b, const tetris_q_head* q) {
    int rc = check_batch(b);
    if (rc) return rc;
    HeadArgs h;
    if ((rc = q_head_args(q, 1, h))) return rc;
    return launch_head(b, h);
}

int tetris_policy_head_dev(tetris_batch* b, const tetris_policy_head* p) {
    int rc = check_batch(b);
    if (rc) return rc;
    HeadArgs h;
    if ((rc = policy_head_args(p, 0, h))) return rc;
    return launch_head(b, h);
}

int tetris_policy_head_grad_dev(tetris_batch* b, const tetris_policy_head* p) {
    int rc = check_batch(b);
    if (rc) return rc;
    HeadArgs h;
    if ((rc = policy_head_args(p, 1, h))) return rc;
    return launch_head(b, h);
}

int tetris_net_input_dev(tetris_batch* b, const tetris_net_input* in) {
    int rc = check_batch(b);
    if (rc) return rc;
    InputArgs ia;
    if ((rc = input_args(shape_of(b), in, ia))) return rc;
    return launch_input(b, ia);
}

int tetris_kbd_conv_dev(tetris_batch* b, const tetris_kbd_conv* k) {
    int rc = check_batch(b);
    if (rc) return rc;
    KbdArgs a;
    if ((rc = kbd_args(k, KBD_FWD, a))) return rc;
    return launch_kbd(b, a);
}

int tetris_kbd_conv_grad_x_dev(tetris_batch* b, const tetris_kbd_conv* k) {
    int rc = check_batch(b);
    if (rc) return rc;
    KbdArgs a;
    if ((rc = kbd_args(k, KBD_GRAD_X, a))) return rc;
    return launch_kbd(b, a);
}

int tetris_kbd_conv_grad_w_dev(tetris_batch* b, const tetris_kbd_conv* k) {
    int rc = check_batch(b);
    if (rc) return rc;
    KbdArgs a;
    if ((rc = kbd_args(k, KBD_GRAD_W, a))) return rc;
    return launch_kbd(b, a);
}

int tetris_res_layer_dev(tetris_batch* b, const tetris_res_layer* r) {
    int rc = check_batch(b);
    if (rc) return rc;
    ResArgs a;
    if ((rc = res_args(r, RES_FWD, a))) return rc;
    return launch_res(b, a);
}

int tetris_res_layer_grad_x_dev(tetris_batch* b, const tetris_res_layer* r) {
    int rc = check_batch(b);
    if (rc) return rc;
    ResArgs a;
    if ((rc = res_args(r, RES_GRAD_X, a))) return rc;
    return launch_res(b, a);
}

int tetris_res_layer_grad_w_dev(tetris_batch* b, const tetris_res_layer* r) {
    int rc = check_batch(b);
    if (rc) return rc;
    ResArgs a;
    if ((rc = res_args(r, RES_GRAD_W, a))) return rc;
    return launch_res(b, a);
}

int tetris_rollout_random(tetris_batch* b, int launches, int steps_per_launch, uint32_t policy_seed, uint64_t first_step,
                          int ms, uint64_t counters[4], float* elapsed_ms) {
    int rc;
    if (counters && (rc = rollout_counters_begin(b))) return rc;
    if ((rc = tetris_rollout_launch(b, launches, steps_per_launch, policy_seed, first_step, ms, elapsed_ms))) return rc;
    if (counters && (rc = rollout_counters_end(b, counters))) return rc;
    return TETRIS_OK;
}

}  // extern "C"
