// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// The CPU test harness with the planning entry points (harness_plan.cpp, included whole) plus the heuristic-policy entry points
// of include/tetris_hip.h (tetris_rt_features_dev, tetris_policy_rt_dev, tetris_step_policy_dev, tetris_rollout_policy,
// tetris_rollout_game_totals_dev) as plain host loops over the same kernel bodies (drl-tetris_amd/csrc/tetris_policy.h).
// "Device" pointers are host pointers here.  __graft_entry__.build_harness compiles this file into libtetris_cpu_harness.so.
//
// Both mappings of the product run here as they do there: one step per call goes through the [40][N] score array (spread
// mapping), fused rollout launches through the lane that evaluates its own candidates.
// The calls' checks and policy_args are the product's (tetris_host.h).
#include "harness_plan.cpp"

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
    const std::vector<uint32_t> before = game_words(b);
    // the harness looks at the flag words after every launch, so the margin only has to cover one launch
    const uint32_t saved = b->margin;
    b->margin = (uint32_t)(2 * steps_per_launch + 16);
    if (b->margin < saved) b->margin = saved;
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
    b->margin = saved;
    if (elapsed_ms) *elapsed_ms = 0.0f;
    if (rc) return rc;
    if (counters) add_counted_since(b, before, counters);
    return TETRIS_OK;
}

}  // extern "C"
