// Host side of the CPU harness, part 4 (as tetris_lib_agent.h, section by section): the agent-side entry points as plain host loops over
// the same bodies; their checks and argument structs' fills are the product's (tetris_host.h).  Needs harness_lib_batch.h and
// harness_lib_rollout.h (margin, counters).  "Device" pointers are host pointers here.

// ---------------------------------------------------------------- planning: action lists, simulated afterstates, list steps, deltas (tetris_plan.h)
static void sim_all(tetris_batch* b, const PlanArgs& pa, int fin) {
    for (int k = 0; k < pa.max_lists; k++)
        for (int i = 0; i < b->N; i++)
            with_shape<1, 4>(b->P, b->tint != 0, [&](auto P, auto TINT) { plan_sim_lane<P(), TINT()>(pa, i, k, fin != 0, SHAPES.s, false); });
}

template <bool AUTO>
static void step_all(tetris_batch* b, const PlanArgs& pa) {
    for (int i = 0; i < b->N; i++)
        with_shape<1, 4>(b->P, b->tint != 0, [&](auto P, auto TINT) { plan_step_lane<P(), TINT(), AUTO>(pa, i, SHAPES.s, false); });
}

extern "C" {

int tetris_action_lists_dev(tetris_batch* b, const uint8_t* player, int max_lists, int max_keys, int flags, int32_t* count,
                            uint8_t* lens, uint8_t* keys) {
    int rc = action_lists_check(shape_of(b), count, lens, keys, max_lists, max_keys, flags);
    if (rc || (rc = finish_call(b))) return rc;          // (the product polls its flag words here instead)
    const int KS = max_keys + 1;
    const size_t lanes = (size_t)b->N * 40;
    std::vector<uint8_t> hc(lanes), hl(lanes * PLAN_LANE_LISTS), hk(lanes * PLAN_LANE_LISTS * KS);
    uint32_t scratch_status[NFLAGS] = {0};
    for (size_t t = 0; t < lanes; t++)
        with_value<1, 4>(b->P, [&](auto P) {
            actions_body<P()>(geo_of_batch(b), t, nullptr, player, b->H, SHAPES.s, hc.data(), hl.data(), hk.data(), PLAN_LANE_LISTS, KS, scratch_status);
        });
    for (int i = 0; i < b->N; i++)
        plan_compact_serial(hc.data(), hl.data(), hk.data(), KS, (size_t)i * 40, (size_t)i, max_lists, max_keys,
                            (flags & TETRIS_LISTS_KEEP_NULL) != 0, count, lens, keys, b->flags);
    return TETRIS_OK;
}

int tetris_simulate_lists_dev(tetris_batch* b, const uint8_t* player, const int32_t* count, const uint8_t* lens, const uint8_t* keys,
                              int max_lists, int max_keys, int ms, int flags, uint32_t* cols, uint8_t* done, uint8_t* lines,
                              uint8_t* dead) {
    int rc = simulate_lists_check(shape_of(b), count, lens, keys, max_lists, max_keys, flags, cols);
    if (rc || (rc = finish_call(b))) return rc;
    PlanArgs pa = plan_args(base_args(b, b->N, nullptr), player, count, lens, keys, max_lists, max_keys, ms);
    pa.cols = cols;
    const int fin = (flags & TETRIS_SIM_FINALIZE) ? 1 : 0;
    if (fin) { pa.a.done = done; pa.a.lines = lines; pa.a.dead = dead; }
    sim_all(b, pa, fin);
    return TETRIS_OK;
}

int tetris_step_lists_dev(tetris_batch* b, const uint8_t* player, const int32_t* choice, const int32_t* count, const uint8_t* lens,
                          const uint8_t* keys, int max_lists, int max_keys, int ms, int flags, uint8_t* done, uint8_t* lines,
                          uint8_t* dead) {
    int rc = step_lists_check(shape_of(b), choice, count, lens, keys, max_lists, max_keys, flags);
    if (rc || (rc = finish_call(b))) return rc;
    PlanArgs pa = plan_args(base_args(b, b->N, nullptr), player, count, lens, keys, max_lists, max_keys, ms);
    pa.choice = choice;
    pa.a.done = done; pa.a.lines = lines; pa.a.dead = dead;
    if (flags & TETRIS_STEP_AUTO_RESET) step_all<true>(b, pa); else step_all<false>(b, pa);
    return TETRIS_OK;
}

int tetris_plan_deltas_dev(tetris_batch* b, const uint8_t* player, const int32_t* count, const uint32_t* cols, int max_lists,
                           float small_fill, int flags, void* deltas, void* sums, uint8_t* small) {
    PlanDeltaArgs da;
    int rc = plan_deltas_args(shape_of(b), geo_of_batch(b), player, count, cols, max_lists, small_fill, flags, deltas, sums, small, da);
    if (rc || (rc = finish_call(b))) return rc;
    const bool major = (flags & TETRIS_DELTAS_LIST_MAJOR) != 0;
    for (int i = 0; i < b->N; i++) {
        if (flags & TETRIS_DELTAS_F16) plan_deltas_game<uint16_t>(da, i, major);
        else plan_deltas_game<float>(da, i, major);
    }
    return TETRIS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- heuristic policy: features, choice, step, rollout (tetris_policy.h)
// Both mappings of the product run here as they do there: one step per call goes through the [40][N] score array (spread
// mapping), fused rollout launches through the lane that evaluates its own candidates.
// (the [40][N] scores live in a vector of the call)
static PolicyArgs policy_args(tetris_batch* b, const uint8_t* player, const int16_t* weights, int per_game, int ms, std::vector<int32_t>& scores) {
    scores.assign((size_t)POLICY_CANDIDATES * b->N, 0);
    return policy_args(base_args(b, b->N, nullptr), player, weights, per_game, ms, scores.data());
}

template <bool FEAT>
static void policy_eval_all(tetris_batch* b, const PolicyArgs& pa) {
    for (int c = 0; c < POLICY_CANDIDATES; c++)
        for (int i = 0; i < b->N; i++) policy_eval_lane<FEAT>(pa, i, c, SHAPES.s);
}

template <bool ROLL, bool AUTO, bool FROM_SCORES>
static void policy_step_all(tetris_batch* b, const PolicyArgs& pa) {
    for (int i = 0; i < b->N; i++)
        with_shape<1, 4>(b->P, b->tint != 0, [&](auto P, auto TINT) { policy_step_lane<P(), TINT(), ROLL, AUTO, FROM_SCORES>(pa, i, SHAPES.s, false); });
}

// which: 0 step, 1 step with auto-reset, 2 one rollout step from the scores, 3 fused rollout steps (as launch_policy_step)
static void policy_step_which(tetris_batch* b, int which, const PolicyArgs& pa) {
    if (which == 0) policy_step_all<false, false, true>(b, pa);
    else if (which == 1) policy_step_all<false, true, true>(b, pa);
    else if (which == 2) policy_step_all<true, true, true>(b, pa);
    else policy_step_all<true, true, false>(b, pa);
}

extern "C" {

int tetris_rt_features_dev(tetris_batch* b, const uint8_t* player, int16_t* features) {
    int rc = policy_check(shape_of(b), "tetris_rt_features_dev", !features, "features is NULL");
    if (rc || (rc = finish_call(b))) return rc;
    std::vector<int32_t> scores;
    PolicyArgs pa = policy_args(b, player, nullptr, 0, 0, scores);
    pa.features = features;
    policy_eval_all<true>(b, pa);
    return TETRIS_OK;
}

int tetris_policy_rt_dev(tetris_batch* b, const uint8_t* player, const int16_t* weights, int per_game, uint8_t* rot, uint8_t* trans,
                         int32_t* score) {
    int rc = policy_check(shape_of(b), "tetris_policy_rt_dev", !weights || !rot || !trans, "weights/rot/trans are NULL");
    if (rc || (rc = finish_call(b))) return rc;
    std::vector<int32_t> scores;
    PolicyArgs pa = policy_args(b, player, weights, per_game, 0, scores);
    pa.rot = rot; pa.trans = trans; pa.score = score;
    policy_eval_all<false>(b, pa);
    for (int i = 0; i < b->N; i++) policy_pick_lane(pa, i);
    return TETRIS_OK;
}

int tetris_step_policy_dev(tetris_batch* b, const uint8_t* player, const int16_t* weights, int per_game, int ms, int flags,
                           uint8_t* done, uint8_t* lines, uint8_t* dead, uint8_t* rot, uint8_t* trans) {
    int rc = policy_check(shape_of(b), "tetris_step_policy_dev", !weights, "weights is NULL", flags);
    if (rc || (rc = finish_call(b))) return rc;
    std::vector<int32_t> scores;
    PolicyArgs pa = policy_args(b, player, weights, per_game, ms, scores);
    pa.a.done = done; pa.a.lines = lines; pa.a.dead = dead;
    pa.rot = rot; pa.trans = trans;
    policy_eval_all<false>(b, pa);
    policy_step_which(b, (flags & TETRIS_STEP_AUTO_RESET) ? 1 : 0, pa);
    return TETRIS_OK;
}

int tetris_rollout_game_totals_dev(tetris_batch* b, uint32_t* totals) {
    int rc = policy_check(shape_of(b), "tetris_rollout_game_totals_dev", !totals, "totals is NULL");
    if (rc || (rc = finish_call(b))) return rc;
    for (int i = 0; i < b->N; i++) policy_game_totals_lane(geo_of_batch(b), i, totals);
    return TETRIS_OK;
}

int tetris_rollout_policy(tetris_batch* b, int launches, int steps_per_launch, const int16_t* weights, int per_game, uint64_t first_step,
                          int ms, uint64_t counters[4], float* elapsed_ms) {
    int rc = rollout_policy_check(shape_of(b), weights, launches, steps_per_launch);
    if (rc) return rc;
    if (counters && (rc = rollout_counters_begin(b))) return rc;
    // the harness looks at the flag words after every launch, so the margin only has to cover one launch
    MarginGuard margin_guard(b, (uint32_t)(2 * steps_per_launch + 16));
    rc = finish_call(b);
    std::vector<int32_t> scores;
    for (int l = 0; l < launches && !rc; l++) {
        PolicyArgs pa = policy_args(b, nullptr, weights, per_game, ms, scores);
        pa.a.steps = steps_per_launch;
        pa.a.first_step = first_step + (uint64_t)l * (uint64_t)steps_per_launch;
        if (steps_per_launch == 1) {
            pa.fixed_player = (int)(pa.a.first_step % (uint64_t)b->P);
            policy_eval_all<false>(b, pa);
            policy_step_which(b, 2, pa);
        } else policy_step_which(b, 3, pa);
        rc = finish_call(b);
    }
    if (elapsed_ms) *elapsed_ms = 0.0f;
    if (rc) return rc;
    if (counters && (rc = rollout_counters_end(b, counters))) return rc;
    return TETRIS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- acting on a network's evaluation (tetris_act.h)
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

// ---------------------------------------------------------------- choosing a planning agent's list from phi (tetris_choose.h)
int tetris_select_lists_dev(tetris_batch* b, const tetris_plan_eval* e) {
    PlanChooseArgs ca;
    int rc = plan_choose_args(shape_of(b), e, "tetris_select_lists_dev", ca);
    if (rc || (rc = finish_call(b))) return rc;
    ca.a = base_args(b, b->N, nullptr);
    ca.a.steps = 1;
    for (int i = 0; i < b->N; i++) plan_choose_game(ca, i);
    return TETRIS_OK;
}

// ---------------------------------------------------------------- trajectory windows (tetris_traj.h)
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

// ---------------------------------------------------------------- a window's states and sample sets (tetris_batch.h)
int tetris_traj_observe_dev(tetris_batch* b, const tetris_traj_obs* obs, int row, const uint8_t* d_player) {
    TrajObserveArgs oa;
    int rc = traj_observe_args(shape_of(b), geo_of_batch(b), obs, row, d_player, oa);
    if (rc) return rc;
    for (int sl = 0; sl < b->P; sl++)
        for (int i = 0; i < b->N; i++) traj_observe_slot(oa, i, sl);
    return TETRIS_OK;
}

int tetris_traj_select_dev(tetris_batch* b, const uint8_t* d_mask, int rows, int flags, int32_t* d_index, long long cap,
                           int32_t* d_count) {
    TrajSelectArgs sa;
    int rc = traj_select_args(shape_of(b), d_mask, rows, flags, d_index, cap, d_count, sa); if (rc) return rc;
    long long k = 0;
    for (uint32_t base = 0; base < sa.total; base += 16u) k += __builtin_popcount(select_bits(sa, base));
    long long pos = 0;
    for (uint32_t base = 0; base < sa.total; base += 16u) {
        const uint32_t bits = select_bits(sa, base);
        select_emit(sa, base, bits, pos, k);
        pos += __builtin_popcount(bits);
    }
    for (long long p = sa.augment ? 2 * k : k; p < sa.cap; p++) sa.index[p] = -1;
    *sa.count = (int32_t)(sa.augment ? 2 * k : k);
    return TETRIS_OK;
}

int tetris_traj_batch_dev(tetris_batch* b, const tetris_traj* traj, const tetris_traj_obs* obs, const float* d_adv_in,
                          const float* d_target_in, const int32_t* d_index, int M, const tetris_traj_batch* out) {
    TrajBatchArgs ba;
    int rc = traj_batch_args(shape_of(b), traj, obs, d_adv_in, d_target_in, d_index, M, out, ba); if (rc) return rc;
    for (int sl = 0; sl < b->P; sl++)
        for (int j = 0; j < M; j++) batch_sample_slot(ba, j, sl);
    return TETRIS_OK;
}

// ---------------------------------------------------------------- the planning agent's windows (tetris_plan_traj.h)
int tetris_traj_record_plan_dev(tetris_batch* b, const tetris_traj* traj, const tetris_traj_plan* plan, const tetris_traj_obs* obs,
                                int row, const tetris_plan_eval* e, const uint8_t* d_done, const uint8_t* d_dead) {
    PlanRecordArgs ra;
    int rc = traj_record_plan_args(shape_of(b), traj, plan, obs, row, e, d_done, d_dead, ra); if (rc) return rc;
    for (int i = 0; i < b->N; i++) plan_record_game(ra, i);
    return TETRIS_OK;
}

int tetris_traj_plan_batch_dev(tetris_batch* b, const tetris_traj_plan* plan, const int32_t* d_index, int M, float small_fill, int flags,
                               void* d_delta, void* d_sums) {
    PlanBatchArgs ba;
    int rc = traj_plan_batch_args(shape_of(b), plan, d_index, M, small_fill, flags, d_delta, d_sums, ba); if (rc) return rc;
    for (int j = 0; j < M; j++) plan_batch_sample(ba, j);
    return TETRIS_OK;
}

// ---------------------------------------------------------------- experience replay (tetris_replay.h)
// The sort runs as the product's three launches per pass do, tile by tile — histogram, scan, scatter — with a serial form of the rank
// inside a tile (sort_tile_histogram, sort_scan_digit, sort_tile_scatter); the wave ballots themselves run on the GPU only.
static void harness_sort(SortArgs so, uint32_t* key, uint32_t* pos, uint32_t* okey, uint32_t* opos) {
    for (int pass = 0; pass < 4; pass++) {
        sort_pass(so, pass, key, pos, okey, opos);
        for (int t = 0; t < so.ntiles; t++) sort_tile_histogram(so, t);
        for (int d = 0; d < SORT_RADIX; d++) sort_scan_digit(so, d);
        for (int t = 0; t < so.ntiles; t++) sort_tile_scatter(so, t);
    }
}

int tetris_replay_add_dev(tetris_batch* b, const tetris_replay* rp, const tetris_traj* traj, const tetris_traj_obs* obs,
                          const float* d_adv_in, const float* d_target_in, const float* d_prio_in, const uint8_t* d_mask, int rows,
                          int flags) {
    ReplayAddArgs aa;
    int rc = replay_add_args(shape_of(b), rp, traj, obs, d_adv_in, d_target_in, d_prio_in, d_mask, rows, flags, aa); if (rc) return rc;
    std::vector<uint32_t> offsets((size_t)b->N + 1);
    aa.offsets = offsets.data();
    uint32_t k = 0u;
    for (int g = 0; g < b->N; g++) {
        const uint32_t c = replay_add_count(aa, g) * (aa.augment ? 2u : 1u);
        offsets[g] = k;
        k += c;
    }
    offsets[b->N] = replay_cursor_rule(aa.rp.cursor, k, (uint32_t)aa.rp.max_size);
    for (int g = 0; g < b->N; g++) replay_add_game(aa, g);
    return TETRIS_OK;
}

int tetris_replay_sample_dev(tetris_batch* b, const tetris_replay* rp, int M, float alpha, float beta, uint32_t seed, uint64_t draw,
                             int32_t* d_index, float* d_weight, int32_t* d_count, int32_t* d_rank, float* d_key) {
    ReplaySampleArgs sa;
    int rc = replay_sample_args(shape_of(b), rp, M, alpha, beta, seed, draw, d_index, d_weight, d_count, d_rank, d_key, sa); if (rc) return rc;
    std::vector<uint32_t> scratch(replay_scratch_words(sa.max_size));
    const SortArgs so = replay_sample_scratch(sa, scratch.data());
    for (uint32_t i = 0; i < sa.max_size; i++) replay_prio_key(sa, i);
    harness_sort(so, sa.key_a, sa.pos_a, sa.key_b, sa.pos_b);
    for (uint32_t s = 0; s < sa.max_size; s++) replay_sample_key(sa, s);
    harness_sort(so, sa.key_b, sa.pos_b, sa.key_a, sa.pos_a);
    if (M == 0) sa.count[0] = 0;
    for (int j = 0; j < M; j++) replay_emit(sa, j);
    return TETRIS_OK;
}

int tetris_replay_update_prios_dev(tetris_batch* b, const tetris_replay* rp, const int32_t* d_index, const float* d_prio_new, int M) {
    ReplayUpdateArgs ua;
    int rc = replay_update_args(shape_of(b), rp, d_index, d_prio_new, M, ua); if (rc) return rc;
    for (int j = 0; j < M; j++) replay_update(ua, j);
    return TETRIS_OK;
}

int tetris_replay_gather_dev(tetris_batch* b, const tetris_replay* rp, const int32_t* d_index, int M, int steps,
                             const tetris_traj_batch* out) {
    TrajBatchArgs ba;
    int rc = replay_gather_args(shape_of(b), rp, d_index, M, steps, out, ba); if (rc) return rc;
    for (int sl = 0; sl < b->P; sl++)
        for (int j = 0; j < ba.m; j++) batch_sample_slot(ba, j, sl);
    return TETRIS_OK;
}

}  // extern "C"
