// Host side of libtetris_hip.so, part 4: the agent-side entry points: planning, heuristic policy, acting on an evaluation, trajectory
// windows, window batches, the planning agent's windows, experience replay, loss heads, output heads, network inputs.  Needs tetris_lib_batch.h and tetris_lib_rollout.h (margin, counters).

// ---------------------------------------------------------------- planning: action lists, simulated afterstates, list steps
// Games per k_actions + k_plan_lists pair: bounds the slab scratch (40 x 16 slab entries of max_keys + 1 bytes per game: 128 MB
// at 4 096 games and 48 keys); a batch of more games enqueues one pair per chunk, ordered by the stream.
static const int PLAN_CHUNK = 4096;

// which: 0 simulate, 1 step, 2 step with auto-reset
static int launch_plan_kernel(tetris_batch* b, int which, dim3 grid, const PlanArgs& pa, int fin) {
    const bool here = with_shape<1, 2>(b->P, b->tint != 0, [&](auto P, auto TINT) { launch_plan<P(), TINT()>(which, grid, b->stream, pa, fin); });
    if (!here && tetris_launch_plan_multi(b->P, b->tint, which, grid, b->stream, pa, fin)) return fail(TETRIS_E_ARG, "no planning kernel for this player count");
    return launched();
}

extern "C" {

int tetris_action_lists_dev(tetris_batch* b, const uint8_t* d_player, int max_lists, int max_keys, int flags, int32_t* d_count,
                            uint8_t* d_lens, uint8_t* d_keys) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = action_lists_check(shape_of(b), d_count, d_lens, d_keys, max_lists, max_keys, flags))) return rc;
    const int chunk = b->N < PLAN_CHUNK ? b->N : PLAN_CHUNK;
    const int KS = max_keys + 1;                 // one key more than the caller takes: a list that does not fit shows as one
    const size_t lanes = (size_t)chunk * 40;
    const size_t need = lanes + lanes * PLAN_LANE_LISTS + lanes * PLAN_LANE_LISTS * KS;
    if (!b->iota.d) {
        std::vector<int32_t> iota((size_t)b->N);
        for (int i = 0; i < b->N; i++) iota[i] = i;
        if ((rc = b->iota.ensure((size_t)b->N, b->stream))) return rc;
        HIP_TRY(hipMemcpy(b->iota.d, iota.data(), (size_t)b->N * 4, hipMemcpyHostToDevice));
    }
    if ((rc = b->plan_status.ensure(NFLAGS, b->stream)) || (rc = b->plan_slabs.ensure(need, b->stream))) return rc;
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    uint8_t* s_cnt = b->plan_slabs.d;
    uint8_t* s_len = s_cnt + lanes;
    uint8_t* s_key = s_len + lanes * PLAN_LANE_LISTS;
    const Geo geo = geo_of_batch(b);
    for (int g0 = 0; g0 < b->N; g0 += chunk) {
        const int m = b->N - g0 < chunk ? b->N - g0 : chunk;
        const int32_t* d_idx = b->iota.d + g0;
        const uint8_t* pl = d_player ? d_player + g0 : nullptr;
        const dim3 grid(blocks_for((size_t)m * 40, 64)), block(64);
        with_value<1, 4>(b->P, [&](auto P) {
            hipLaunchKernelGGL(k_actions<P()>, grid, block, 0, b->stream, geo, m, d_idx, pl, b->H, s_cnt, s_len, s_key, PLAN_LANE_LISTS, KS, b->plan_status.d);
        });
        if ((rc = launched())) return rc;
        if ((rc = launch(b, k_plan_lists, dim3((unsigned)m), block, 0, s_cnt, s_len, s_key, KS, g0, max_lists, max_keys,
                         (flags & TETRIS_LISTS_KEEP_NULL) ? 1 : 0, d_count, d_lens, d_keys, b->flags))) return rc;
    }
    return TETRIS_OK;
}

int tetris_simulate_lists_dev(tetris_batch* b, const uint8_t* d_player, const int32_t* d_count, const uint8_t* d_lens, const uint8_t* d_keys,
                              int max_lists, int max_keys, int ms, int flags, uint32_t* d_cols, uint8_t* d_done, uint8_t* d_lines,
                              uint8_t* d_dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = simulate_lists_check(shape_of(b), d_count, d_lens, d_keys, max_lists, max_keys, flags, d_cols))) return rc;
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    PlanArgs pa = plan_args(base_args(b, b->N, nullptr), d_player, d_count, d_lens, d_keys, max_lists, max_keys, ms);
    pa.cols = d_cols;
    const int fin = (flags & TETRIS_SIM_FINALIZE) ? 1 : 0;
    if (fin) { pa.a.done = d_done; pa.a.lines = d_lines; pa.a.dead = d_dead; }
    return launch_plan_kernel(b, 0, dim3(blocks_for(b->N, 64), (unsigned)max_lists), pa, fin);
}

int tetris_step_lists_dev(tetris_batch* b, const uint8_t* d_player, const int32_t* d_choice, const int32_t* d_count, const uint8_t* d_lens,
                          const uint8_t* d_keys, int max_lists, int max_keys, int ms, int flags, uint8_t* d_done, uint8_t* d_lines,
                          uint8_t* d_dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = step_lists_check(shape_of(b), d_choice, d_count, d_lens, d_keys, max_lists, max_keys, flags))) return rc;
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    PlanArgs pa = plan_args(base_args(b, b->N, nullptr), d_player, d_count, d_lens, d_keys, max_lists, max_keys, ms);
    pa.choice = d_choice;
    pa.a.done = d_done; pa.a.lines = d_lines; pa.a.dead = d_dead;
    return launch_plan_kernel(b, (flags & TETRIS_STEP_AUTO_RESET) ? 2 : 1, dim3(blocks_for(b->N, 64)), pa, 0);
}

int tetris_plan_deltas_dev(tetris_batch* b, const uint8_t* d_player, const int32_t* d_count, const uint32_t* d_cols, int max_lists,
                           float small_fill, int flags, void* d_deltas, void* d_sums, uint8_t* d_small) {
    int rc = check_batch(b);
    if (rc) return rc;
    static_assert(PD_BLOCK == PLAN_DELTAS_MAX_LISTS, "list k = thread k");
    PlanDeltaArgs da;
    if ((rc = plan_deltas_args(shape_of(b), geo_of_batch(b), d_player, d_count, d_cols, max_lists, small_fill, flags, d_deltas, d_sums, d_small, da))) return rc;
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;
    const dim3 grid(blocks_for(b->N, 128) * 128u), block(PD_BLOCK);     // whole groups of 8 XCDs x 16 games
    with_flag((flags & TETRIS_DELTAS_F16) != 0, [&](auto F16) {
        with_flag((flags & TETRIS_DELTAS_LIST_MAJOR) != 0, [&](auto MAJOR) {
            hipLaunchKernelGGL((k_plan_deltas<std::conditional_t<F16(), uint16_t, float>, MAJOR()>), grid, block, 0, b->stream, da);
        });
    });
    return launched();
}

}  // extern "C"

// ---------------------------------------------------------------- heuristic policy: features, choice, step, rollout (tetris_policy.h)

static PolicyArgs policy_args(tetris_batch* b, const uint8_t* d_player, const int16_t* d_weights, int per_game, int ms) {
    return policy_args(base_args(b, b->N, nullptr), d_player, d_weights, per_game, ms, b->policy_scores.d);
}

static int policy_scores_buffer(tetris_batch* b) { return b->policy_scores.ensure((size_t)POLICY_CANDIDATES * b->N, b->stream); }

static dim3 policy_eval_grid(const tetris_batch* b) { return dim3(blocks_for(b->N, 64), (unsigned)POLICY_CANDIDATES); }

// the 40 scores of every game -> b->policy_scores
static int launch_policy_scores(tetris_batch* b, const PolicyArgs& pa) {
    return launch(b, k_policy_eval<false>, policy_eval_grid(b), dim3(64), 0, pa);
}

// which: as launch_policy_step (tetris_game_kernel.h)
static int launch_policy_step_kernel(tetris_batch* b, int which, const PolicyArgs& pa) {
    const dim3 grid(blocks_for(b->N, 64));
    const bool here = with_shape<1, 2>(b->P, b->tint != 0, [&](auto P, auto TINT) { launch_policy_step<P(), TINT()>(which, grid, b->stream, pa); });
    if (!here && tetris_launch_policy_multi(b->P, b->tint, which, grid, b->stream, pa)) return fail(TETRIS_E_ARG, "no policy kernel for this player count");
    return launched();
}

extern "C" {

int tetris_rt_features_dev(tetris_batch* b, const uint8_t* d_player, int16_t* d_features) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = policy_check(shape_of(b), "tetris_rt_features_dev", !d_features, "features is NULL"))) return rc;
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    PolicyArgs pa = policy_args(b, d_player, nullptr, 0, 0);
    pa.features = d_features;
    return launch(b, k_policy_eval<true>, policy_eval_grid(b), dim3(64), 0, pa);
}

int tetris_policy_rt_dev(tetris_batch* b, const uint8_t* d_player, const int16_t* d_weights, int per_game, uint8_t* d_rot,
                         uint8_t* d_trans, int32_t* d_score) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = policy_check(shape_of(b), "tetris_policy_rt_dev", !d_weights || !d_rot || !d_trans, "weights/rot/trans are NULL"))) return rc;
    if ((rc = policy_scores_buffer(b))) return rc;
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    PolicyArgs pa = policy_args(b, d_player, d_weights, per_game, 0);
    pa.rot = d_rot; pa.trans = d_trans; pa.score = d_score;
    if ((rc = launch_policy_scores(b, pa))) return rc;
    return launch(b, k_policy_pick, dim3(blocks_for(b->N)), dim3(256), 0, pa);
}

int tetris_step_policy_dev(tetris_batch* b, const uint8_t* d_player, const int16_t* d_weights, int per_game, int ms, int flags,
                           uint8_t* d_done, uint8_t* d_lines, uint8_t* d_dead, uint8_t* d_rot, uint8_t* d_trans) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = policy_check(shape_of(b), "tetris_step_policy_dev", !d_weights, "weights is NULL", flags))) return rc;
    if ((rc = policy_scores_buffer(b))) return rc;
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    PolicyArgs pa = policy_args(b, d_player, d_weights, per_game, ms);
    pa.a.done = d_done; pa.a.lines = d_lines; pa.a.dead = d_dead;
    pa.rot = d_rot; pa.trans = d_trans;
    if ((rc = launch_policy_scores(b, pa))) return rc;
    return launch_policy_step_kernel(b, (flags & TETRIS_STEP_AUTO_RESET) ? 1 : 0, pa);
}

int tetris_rollout_game_totals_dev(tetris_batch* b, uint32_t* d_totals) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = policy_check(shape_of(b), "tetris_rollout_game_totals_dev", !d_totals, "totals is NULL"))) return rc;
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    return launch(b, k_policy_totals, dim3(blocks_for(b->N)), dim3(256), 0, geo_of_batch(b), d_totals);
}

// The launches of tetris_rollout_policy, un-chained on the batch's stream.  One step per launch: the spread mapping (the scores of
// all 40 N candidates, then one lane per game that chooses and steps); more: one launch whose lanes evaluate their own candidates.
static int rollout_policy_launches(tetris_batch* b, int launches, int steps_per_launch, const int16_t* d_weights, int per_game,
                                   uint64_t first_step, int ms, float* elapsed_ms) {
    const int group = rollout_group(steps_per_launch);
    MarginGuard margin_guard(b, rollout_margin(steps_per_launch, group));
    int rc = TETRIS_OK;
    HIP_TRY(hipEventRecord(b->ev0, b->stream));
    for (int l = 0; l < launches; l++) {
        if ((rc = gate_launch(b, group))) return rc;
        PolicyArgs pa = policy_args(b, nullptr, d_weights, per_game, ms);
        pa.a.steps = steps_per_launch;
        pa.a.first_step = first_step + (uint64_t)l * (uint64_t)steps_per_launch;
        if (steps_per_launch == 1) {
            pa.fixed_player = (int)(pa.a.first_step % (uint64_t)b->P);      // the evaluation kernel's acting player: step mod P
            if ((rc = launch_policy_scores(b, pa))) return rc;
            if ((rc = launch_policy_step_kernel(b, 2, pa))) return rc;
        } else if ((rc = launch_policy_step_kernel(b, 3, pa))) return rc;
    }
    HIP_TRY(hipEventRecord(b->ev1, b->stream));
    HIP_TRY(poll_event(b->ev1, 200000));
    if ((rc = finish_call(b, true))) return rc;   // the end event is behind everything this call enqueued
    if (elapsed_ms) HIP_TRY(hipEventElapsedTime(elapsed_ms, b->ev0, b->ev1));
    return TETRIS_OK;
}

int tetris_rollout_policy(tetris_batch* b, int launches, int steps_per_launch, const int16_t* d_weights, int per_game,
                          uint64_t first_step, int ms, uint64_t counters[4], float* elapsed_ms) {
    int rc = check_batch(b);
    if (rc) return rc;
    if ((rc = rollout_policy_check(shape_of(b), d_weights, launches, steps_per_launch))) return rc;
    if ((rc = policy_scores_buffer(b))) return rc;
    if (counters && (rc = rollout_counters_begin(b))) return rc;
    if ((rc = rollout_policy_launches(b, launches, steps_per_launch, d_weights, per_game, first_step, ms, elapsed_ms))) return rc;
    if (counters && (rc = rollout_counters_end(b, counters))) return rc;      // (what this call did, whatever the words held: as tetris_rollout_random)
    return TETRIS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- acting on a network's evaluation (tetris_act.h)
extern "C" {

int tetris_select_eval_dev(tetris_batch* b, const tetris_act_eval* e) {
    int rc = check_batch(b);
    if (rc) return rc;
    ActArgs aa;
    if ((rc = act_args(shape_of(b), e, "tetris_select_eval_dev", aa))) return rc;
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    aa.a = base_args(b, b->N, nullptr);          // (behind the gate: it may have extended the RNG tables)
    aa.a.steps = 1;
    return launch(b, k_act_select, dim3(blocks_for(b->N, ACT_BLOCK)), dim3(ACT_THREADS), 0, aa);
}

// ---------------------------------------------------------------- choosing a planning agent's list from phi (tetris_choose.h)
int tetris_select_lists_dev(tetris_batch* b, const tetris_plan_eval* e) {
    int rc = check_batch(b);
    if (rc) return rc;
    PlanChooseArgs ca;
    if ((rc = plan_choose_args(shape_of(b), e, "tetris_select_lists_dev", ca))) return rc;
    if ((rc = enqueue(b, Enqueue::STEPS))) return rc;
    ca.a = base_args(b, b->N, nullptr);          // (behind the gate: it may have extended the RNG tables)
    ca.a.steps = 1;
    const int G = choose_games_per_block(b->H, ca.max_lists);
    const size_t lds = choose_lds_bytes(G, b->H, ca.max_lists);
    const dim3 grid(blocks_for(b->N, G)), block(CHOOSE_THREADS);
    with_flag(G == 32, [&](auto WIDE) { hipLaunchKernelGGL((k_plan_choose<WIDE() ? 32 : 16>), grid, block, lds, b->stream, ca); });
    return launched();
}

// ---------------------------------------------------------------- trajectory windows (tetris_traj.h)
int tetris_traj_record_dev(tetris_batch* b, const tetris_traj* traj, int row, const tetris_act_eval* e, const uint8_t* d_done,
                           const uint8_t* d_dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    TrajRecordArgs ra;
    if ((rc = traj_record_args(shape_of(b), traj, row, e, d_done, d_dead, ra))) return rc;
    if ((rc = enqueue(b, Enqueue::CALLER))) return rc;          // the caller's evaluation and step outputs -> the caller's window
    return launch(b, k_traj_record, dim3(blocks_for(b->N, TRAJ_LANE_THREADS)), dim3(TRAJ_LANE_THREADS), 0, ra);
}

int tetris_traj_advantages_dev(tetris_batch* b, const tetris_traj* traj, int rows, float gamma, float lambda_adv,
                               float lambda_value, const float* d_boot, float* d_adv, float* d_target, uint8_t* d_closed) {
    int rc = check_batch(b);
    if (rc) return rc;
    TrajAdvArgs aa;
    if ((rc = traj_adv_args(shape_of(b), traj, rows, gamma, lambda_adv, lambda_value, d_boot, d_adv, d_target, d_closed, aa))) return rc;
    if ((rc = enqueue(b, Enqueue::CALLER))) return rc;          // the caller's window -> the caller's advantages and targets
    return launch(b, k_traj_advantages, dim3(blocks_for(b->N, TRAJ_BLOCK)), dim3(TRAJ_THREADS), 0, aa);
}

// ---------------------------------------------------------------- a window's states and sample sets (tetris_batch.h)
int tetris_traj_observe_dev(tetris_batch* b, const tetris_traj_obs* obs, int row, const uint8_t* d_player) {
    int rc = check_batch(b);
    if (rc) return rc;
    TrajObserveArgs oa;
    if ((rc = traj_observe_args(shape_of(b), geo_of_batch(b), obs, row, d_player, oa))) return rc;
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;
    return launch(b, k_traj_observe, dim3(blocks_for(b->N, TRAJ_LANE_THREADS), (unsigned)b->P), dim3(TRAJ_LANE_THREADS), 0, oa);
}

int tetris_traj_select_dev(tetris_batch* b, const uint8_t* d_mask, int rows, int flags, int32_t* d_index, long long cap,
                           int32_t* d_count) {
    int rc = check_batch(b);
    if (rc) return rc;
    TrajSelectArgs sa;
    if ((rc = traj_select_args(shape_of(b), d_mask, rows, flags, d_index, cap, d_count, sa))) return rc;
    if ((rc = b->select_blocks.ensure((size_t)sa.nblocks + 1, b->stream))) return rc;
    sa.blocks = b->select_blocks.d;
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;
    const dim3 grid((unsigned)sa.nblocks), block(SELECT_THREADS);
    if ((rc = launch(b, k_select_count, grid, block, 0, sa)) || (rc = launch(b, k_select_scan, dim3(1), block, 0, sa))) return rc;
    return launch(b, k_select_scatter, grid, block, 0, sa);
}

// the gather of a minibatch: tetris_traj_batch_dev from a window, tetris_replay_gather_dev from the replay's ring
static int launch_traj_batch(tetris_batch* b, const TrajBatchArgs& ba) {
    if (ba.m == 0) return TETRIS_OK;
    const int rc = enqueue(b, Enqueue::STATE);
    if (rc) return rc;
    const size_t lds = ba.visual ? (size_t)BATCH_BLOCK * b->H * NCOL : 0;          // at most 19 840 bytes (31 rows)
    return launch(b, k_traj_batch, dim3(blocks_for(ba.m, BATCH_BLOCK), (unsigned)b->P), dim3(BATCH_BLOCK), lds, ba);
}

int tetris_traj_batch_dev(tetris_batch* b, const tetris_traj* traj, const tetris_traj_obs* obs, const float* d_adv_in,
                          const float* d_target_in, const int32_t* d_index, int M, const tetris_traj_batch* out) {
    int rc = check_batch(b);
    if (rc) return rc;
    TrajBatchArgs ba;
    if ((rc = traj_batch_args(shape_of(b), traj, obs, d_adv_in, d_target_in, d_index, M, out, ba))) return rc;
    return launch_traj_batch(b, ba);
}

// ---------------------------------------------------------------- the planning agent's windows (tetris_plan_traj.h)
int tetris_traj_record_plan_dev(tetris_batch* b, const tetris_traj* traj, const tetris_traj_plan* plan, const tetris_traj_obs* obs,
                                int row, const tetris_plan_eval* e, const uint8_t* d_done, const uint8_t* d_dead) {
    int rc = check_batch(b);
    if (rc) return rc;
    PlanRecordArgs ra;
    if ((rc = traj_record_plan_args(shape_of(b), traj, plan, obs, row, e, d_done, d_dead, ra))) return rc;
    if ((rc = enqueue(b, Enqueue::CALLER))) return rc;          // the caller's choice, columns and records -> the caller's windows
    const size_t lds = ra.rec ? plan_record_lds_bytes(ra.max_lists) : plan_record_lds_bytes(0);
    return launch(b, k_traj_record_plan, dim3(blocks_for(b->N, PLAN_RECORD_GAMES)), dim3(PLAN_RECORD_THREADS), lds, ra);
}

int tetris_traj_plan_batch_dev(tetris_batch* b, const tetris_traj_plan* plan, const int32_t* d_index, int M, float small_fill, int flags,
                               void* d_delta, void* d_sums) {
    int rc = check_batch(b);
    if (rc) return rc;
    PlanBatchArgs ba;
    if ((rc = traj_plan_batch_args(shape_of(b), plan, d_index, M, small_fill, flags, d_delta, d_sums, ba))) return rc;
    if (M == 0) return TETRIS_OK;
    if ((rc = enqueue(b, Enqueue::CALLER))) return rc;          // the caller's records -> the caller's planes
    const dim3 grid(blocks_for(M, PLAN_BATCH_SAMPLES)), block(PLAN_BATCH_THREADS);
    with_flag(ba.f16 != 0, [&](auto F16) { hipLaunchKernelGGL((k_traj_plan_batch<std::conditional_t<F16(), uint16_t, float>>), grid, block, 0, b->stream, ba); });
    return launched();
}

// ---------------------------------------------------------------- experience replay (tetris_replay.h)
// four passes from (key, pos) back into (key, pos), through (okey, opos)
static int launch_sort(tetris_batch* b, SortArgs so, uint32_t* key, uint32_t* pos, uint32_t* okey, uint32_t* opos) {
    const dim3 tiles((unsigned)so.ntiles), block(SORT_THREADS);
    int rc = TETRIS_OK;
    for (int pass = 0; pass < 4 && !rc; pass++) {
        sort_pass(so, pass, key, pos, okey, opos);
        if ((rc = launch(b, k_sort_histogram, tiles, block, 0, so))) break;
        if ((rc = launch(b, k_sort_scan, dim3(SORT_RADIX), dim3(SORT_SCAN_SPAN), 0, so))) break;
        rc = launch(b, k_sort_scatter, tiles, block, 0, so);
    }
    return rc;
}

int tetris_replay_add_dev(tetris_batch* b, const tetris_replay* rp, const tetris_traj* traj, const tetris_traj_obs* obs,
                          const float* d_adv_in, const float* d_target_in, const float* d_prio_in, const uint8_t* d_mask, int rows,
                          int flags) {
    int rc = check_batch(b);
    if (rc) return rc;
    ReplayAddArgs aa;
    if ((rc = replay_add_args(shape_of(b), rp, traj, obs, d_adv_in, d_target_in, d_prio_in, d_mask, rows, flags, aa))) return rc;
    if ((rc = b->replay_offsets.ensure((size_t)b->N + 1, b->stream))) return rc;
    aa.offsets = b->replay_offsets.d;
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;
    const dim3 grid(blocks_for(b->N, REPLAY_THREADS)), block(REPLAY_THREADS);
    if ((rc = launch(b, k_replay_add_count, grid, block, 0, aa)) ||
        (rc = launch(b, k_replay_add_scan, dim3(1), dim3(SELECT_THREADS), 0, aa))) return rc;
    return launch(b, k_replay_add_scatter, grid, block, 0, aa);
}

int tetris_replay_sample_dev(tetris_batch* b, const tetris_replay* rp, int M, float alpha, float beta, uint32_t seed, uint64_t draw,
                             int32_t* d_index, float* d_weight, int32_t* d_count, int32_t* d_rank, float* d_key) {
    int rc = check_batch(b);
    if (rc) return rc;
    ReplaySampleArgs sa;
    if ((rc = replay_sample_args(shape_of(b), rp, M, alpha, beta, seed, draw, d_index, d_weight, d_count, d_rank, d_key, sa))) return rc;
    if ((rc = b->replay_sort.ensure(replay_scratch_words(sa.max_size), b->stream))) return rc;
    const SortArgs so = replay_sample_scratch(sa, b->replay_sort.d);
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;
    const dim3 all(blocks_for(sa.max_size, REPLAY_THREADS)), block(REPLAY_THREADS);
    if ((rc = launch(b, k_replay_prio_keys, all, block, 0, sa)) || (rc = launch_sort(b, so, sa.key_a, sa.pos_a, sa.key_b, sa.pos_b)) ||
        (rc = launch(b, k_replay_sample_keys, all, block, 0, sa)) || (rc = launch_sort(b, so, sa.key_b, sa.pos_b, sa.key_a, sa.pos_a))) return rc;
    return launch(b, k_replay_emit, dim3(std::max(1u, blocks_for(M, REPLAY_THREADS))), block, 0, sa);
}

int tetris_replay_update_prios_dev(tetris_batch* b, const tetris_replay* rp, const int32_t* d_index, const float* d_prio_new, int M) {
    int rc = check_batch(b);
    if (rc) return rc;
    ReplayUpdateArgs ua;
    if ((rc = replay_update_args(shape_of(b), rp, d_index, d_prio_new, M, ua))) return rc;
    if (M == 0) return TETRIS_OK;
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;
    return launch(b, k_replay_update, dim3(blocks_for(M, REPLAY_THREADS)), dim3(REPLAY_THREADS), 0, ua);
}

int tetris_replay_gather_dev(tetris_batch* b, const tetris_replay* rp, const int32_t* d_index, int M, int steps,
                             const tetris_traj_batch* out) {
    int rc = check_batch(b);
    if (rc) return rc;
    TrajBatchArgs ba;
    if ((rc = replay_gather_args(shape_of(b), rp, d_index, M, steps, out, ba))) return rc;
    return launch_traj_batch(b, ba);
}

}  // extern "C"

// ---------------------------------------------------------------- k-step target estimator (tetris_kstep.h)
// What tetris_kstep_target_dev (tetris_lib_compose.h) runs after the argument rules: in Q mode the values of the M n rows — into
// d_values, or into the batch's scratch where the caller wants none —, then the samples
static int launch_kstep(tetris_batch* b, KstepArgs& a) {
    if (a.M == 0) return TETRIS_OK;
    int rc;
    if (a.mode == KSTEP_Q) {
        if (!a.values && (rc = b->kstep_values.ensure((size_t)a.M * a.n, b->stream))) return rc;
        a.vals = a.values ? a.values : b->kstep_values.d;
    }
    if ((rc = enqueue(b, Enqueue::STATE))) return rc;                // (the batch's scratch)
    if (a.mode == KSTEP_Q && (rc = launch(b, k_kstep_values, dim3((unsigned)kstep_value_blocks(a)), dim3(KSTEP_VALUE_THREADS), 0, a))) return rc;
    return launch(b, k_kstep_estimate, dim3(blocks_for(a.M, KSTEP_THREADS)), dim3(KSTEP_THREADS), 0, a);
}

// ---------------------------------------------------------------- output heads (tetris_head.h)
// What the four head entry points (tetris_lib_compose.h) run after the argument rules: one launch, a workgroup per HEAD_BLOCK samples
static int launch_head(tetris_batch* b, const HeadArgs& h) {
    int rc = enqueue(b, Enqueue::CALLER);
    if (rc) return rc;
    const dim3 grid((unsigned)head_blocks(h.M)), block(HEAD_THREADS);
    if (h.head == HEAD_Q) return h.grad ? launch(b, k_q_head_grad, grid, block, 0, h) : launch(b, k_q_head, grid, block, 0, h);
    return h.grad ? launch(b, k_policy_head_grad, grid, block, 0, h) : launch(b, k_policy_head, grid, block, 0, h);
}

// ---------------------------------------------------------------- keyboard convolution (tetris_kbd.h)
// What the three keyboard-convolution entry points (tetris_lib_compose.h) run after the argument rules, two launches each: the
// forward and grad_x repack w into the batch's scratch and then run the product; grad_w writes a partial per chunk of
// KBD_W_SAMPLES samples there and then adds them up
static int launch_kbd(tetris_batch* b, const KbdArgs& in) {
    KbdArgs a = in;
    const size_t packed = (size_t)a.Hp * KBD_D * KBD_OP * a.C, per = packed + KBD_OP;      // elements of the repacked w; floats of a partial with its bias row
    a.chunks = kbd_w_chunks(a.M);
    const size_t words = a.op == KBD_GRAD_W ? (size_t)a.chunks * per : a.f16 ? packed / 2 : packed;
    int rc = b->kbd_scratch.ensure(words, b->stream);
    if (rc || (rc = enqueue(b, Enqueue::STATE))) return rc;          // (the batch's scratch)
    a.packed = b->kbd_scratch.d; a.partial = reinterpret_cast<float*>(b->kbd_scratch.d);
    const dim3 block(KBD_THREADS);
    with_flag(a.f16 != 0, [&](auto F16) {
        if (a.op == KBD_FWD) {
            hipLaunchKernelGGL((k_kbd_pack<F16(), true>), dim3(blocks_for(packed, KBD_THREADS)), block, 0, b->stream, a, (void*)b->kbd_scratch.d);
            hipLaunchKernelGGL((k_kbd_fwd<F16(), KBD_BLOCK>), dim3((unsigned)kbd_blocks(a.M)), dim3(KBD_FWD_THREADS), 0, b->stream, a);
        } else if (a.op == KBD_GRAD_X) {
            hipLaunchKernelGGL((k_kbd_pack<F16(), false>), dim3(blocks_for(packed, KBD_THREADS)), block, 0, b->stream, a, (void*)b->kbd_scratch.d);
            hipLaunchKernelGGL((k_kbd_grad_x<F16(), KBD_BLOCK>), dim3((unsigned)kbd_blocks(a.M)), block, 0, b->stream, a);
        } else {
            const dim3 grid((unsigned)a.chunks, (unsigned)a.Hp, (unsigned)((a.C + KBD_W_CHANNELS - 1) / KBD_W_CHANNELS));
            hipLaunchKernelGGL((k_kbd_grad_w<F16()>), grid, block, 0, b->stream, a);
            hipLaunchKernelGGL(k_kbd_grad_w_reduce, dim3(blocks_for(per, KBD_THREADS)), block, 0, b->stream, a);
        }
    });
    return launched();
}

// ---------------------------------------------------------------- residual layer (tetris_res.h)
// What the three residual-layer entry points (tetris_lib_compose.h) run after the argument rules, two launches each: the forward
// and grad_x repack w into the batch's scratch and then run the product; grad_w writes a partial per chunk of RES_W_SAMPLES samples
// there and then adds them up
static int launch_res(tetris_batch* b, const ResArgs& in) {
    ResArgs a = in;
    if (a.op == RES_FWD) { a.N = a.Cz; a.K = a.Ci; } else { a.N = a.Ci; a.K = a.Cz; }
    a.NP = res_pad32(a.N); a.KP = res_pad32(a.K);
    a.chunks = res_w_chunks(a.M);
    const size_t packed = (size_t)RES_TAPS * a.NP * a.KP, per = (size_t)RES_TAPS * a.Ci * a.Co + (size_t)a.Co;      // elements of the repacked w; floats of a partial with its bias row
    const size_t words = a.op == RES_GRAD_W ? (size_t)a.chunks * per : a.f16 ? packed / 2 : packed;
    int rc = b->res_scratch.ensure(words, b->stream);
    if (rc || (rc = enqueue(b, Enqueue::STATE))) return rc;          // (the batch's scratch)
    a.packed = b->res_scratch.d; a.partial = reinterpret_cast<float*>(b->res_scratch.d);
    const dim3 block(RES_THREADS), conv_grid((unsigned)((size_t)a.M * res_bands(a.Hp)), (unsigned)((a.NP + RES_NB - 1) / RES_NB));
    with_flag(a.f16 != 0, [&](auto F16) {
        if (a.op == RES_FWD) {
            hipLaunchKernelGGL((k_res_pack<F16(), true>), dim3(blocks_for(packed, RES_THREADS)), block, 0, b->stream, a, (void*)b->res_scratch.d);
            hipLaunchKernelGGL((k_res_conv<F16(), true>), conv_grid, block, 0, b->stream, a);
        } else if (a.op == RES_GRAD_X) {
            hipLaunchKernelGGL((k_res_pack<F16(), false>), dim3(blocks_for(packed, RES_THREADS)), block, 0, b->stream, a, (void*)b->res_scratch.d);
            hipLaunchKernelGGL((k_res_conv<F16(), false>), conv_grid, block, 0, b->stream, a);
        } else {
            const dim3 grid((unsigned)a.chunks, (unsigned)((a.Ci + RES_W_CHANNELS - 1) / RES_W_CHANNELS), (unsigned)(a.Co / RES_W_CHANNELS));
            hipLaunchKernelGGL((k_res_grad_w<F16()>), grid, block, 0, b->stream, a);
            hipLaunchKernelGGL(k_res_grad_w_reduce, dim3(blocks_for(per, RES_THREADS)), block, 0, b->stream, a);
        }
    });
    return launched();
}

// ---------------------------------------------------------------- network inputs (tetris_input.h)
// What tetris_net_input_dev (tetris_lib_compose.h) runs after the argument rules: one launch, a workgroup per INPUT_BLOCK samples
// of a slot
static int launch_input(tetris_batch* b, const InputArgs& ia) {
    if (ia.ba.m == 0) return TETRIS_OK;
    const int rc = enqueue(b, Enqueue::CALLER);          // the caller's records -> the caller's planes
    if (rc) return rc;
    const dim3 grid((unsigned)input_blocks(ia.ba.m), (unsigned)b->P), block(INPUT_THREADS);
    // (an image of at most 32 rows — every height but 31 with the pad — fits 32-bit column words; one channel is the same memory in both layouts)
    with_flag(ia.f16 != 0, [&](auto F16) {
        with_flag(ia.last != 0 && ia.C > 1, [&](auto LAST) {
            with_flag(ia.Hp > 32, [&](auto WIDE) {
                hipLaunchKernelGGL((k_net_input<std::conditional_t<F16(), uint16_t, float>, LAST(), std::conditional_t<WIDE(), uint64_t, uint32_t>>),
                                   grid, block, 0, b->stream, ia);
            });
        });
    });
    return launched();
}

// ---------------------------------------------------------------- loss heads (tetris_loss.h)
// What tetris_ppo_loss_dev, tetris_dqn_loss_dev and tetris_plan_loss_dev (tetris_lib_compose.h) run after the argument rules, at most
// three launches: the count of D / Dnz where a mask, weights or a window's index list are given, the head, the statistics
static int launch_loss(tetris_batch* b, LossArgs& la) {
    if (la.M == 0) {
        HIP_TRY(hipMemsetAsync(la.stats, 0, LOSS_STATS * sizeof(float), b->stream));
        return TETRIS_OK;
    }
    int rc = b->loss_scratch.ensure(loss_scratch_words(la), b->stream);
    if (rc || (rc = enqueue(b, Enqueue::STATE))) return rc;          // (the batch's scratch)
    la.partial = reinterpret_cast<float*>(b->loss_scratch.d + 4);
    if (loss_counts(la)) {
        if ((rc = launch(b, k_loss_count, dim3(1), dim3(LOSS_COUNT_THREADS), 0, la, b->loss_scratch.d))) return rc;
        la.count = b->loss_scratch.d;
    }
    const int blocks = loss_blocks_of(la);
    if (la.head == LOSS_PLAN) rc = launch(b, k_plan_loss_head, dim3((unsigned)blocks), dim3(PLAN_LOSS_THREADS), 0, la);
    else rc = launch(b, k_loss_head, dim3((unsigned)blocks), dim3(LOSS_THREADS), 0, la);
    if (rc) return rc;
    return launch(b, k_loss_reduce, dim3(1), dim3(LOSS_REDUCE_LANES), 0, la, blocks);
}
