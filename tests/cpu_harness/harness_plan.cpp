// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// The CPU test harness (harness.cpp, included whole) plus the planning entry points of include/tetris_hip.h
// (tetris_action_lists_dev, tetris_simulate_lists_dev, tetris_step_lists_dev) as plain host loops over the same kernel
// bodies (drl-tetris_amd/csrc/tetris_plan.h).  "Device" pointers are host pointers here.  __graft_entry__.build_harness
// compiles this file into libtetris_cpu_harness.so.
//
// tetris_take_errors of harness.cpp is renamed on the way in and wrapped below, so that it also reports TETRIS_ERR_LISTS.
#define tetris_take_errors harness_take_errors_base
#include "harness.cpp"
#undef tetris_take_errors

#include "../../drl-tetris_amd/csrc/tetris_plan.h"

static PlanArgs plan_args(tetris_batch* b, const uint8_t* player, const int32_t* count, const uint8_t* lens, const uint8_t* keys,
                          int max_lists, int max_keys, int ms) {
    PlanArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.a = base_args(b, b->N, nullptr);
    pa.a.ms = ms;
    pa.player = player; pa.count = count; pa.lens = lens; pa.keys = keys;
    pa.max_lists = max_lists; pa.max_keys = max_keys;
    return pa;
}

template <bool TINT>
static void sim_all(tetris_batch* b, const PlanArgs& pa, int fin) {
    for (int k = 0; k < pa.max_lists; k++)
        for (int i = 0; i < b->N; i++) {
            if (b->P == 1) plan_sim_lane<1, TINT>(pa, i, k, fin != 0, SHAPES.s, false);
            else if (b->P == 2) plan_sim_lane<2, TINT>(pa, i, k, fin != 0, SHAPES.s, false);
            else if (b->P == 3) plan_sim_lane<3, TINT>(pa, i, k, fin != 0, SHAPES.s, false);
            else plan_sim_lane<4, TINT>(pa, i, k, fin != 0, SHAPES.s, false);
        }
}

template <bool TINT, bool AUTO>
static void step_all(tetris_batch* b, const PlanArgs& pa) {
    for (int i = 0; i < b->N; i++) {
        if (b->P == 1) plan_step_lane<1, TINT, AUTO>(pa, i, SHAPES.s, false);
        else if (b->P == 2) plan_step_lane<2, TINT, AUTO>(pa, i, SHAPES.s, false);
        else if (b->P == 3) plan_step_lane<3, TINT, AUTO>(pa, i, SHAPES.s, false);
        else plan_step_lane<4, TINT, AUTO>(pa, i, SHAPES.s, false);
    }
}

extern "C" {

int tetris_take_errors(tetris_batch* b, uint32_t* bits) {
    const int rc = harness_take_errors_base(b, bits);
    if (rc) return rc;
    if (b->flags[F_LISTS]) *bits |= TETRIS_ERR_LISTS;
    b->flags[F_LISTS] = 0;
    return TETRIS_OK;
}

int tetris_action_lists_dev(tetris_batch* b, const uint8_t* player, int max_lists, int max_keys, int flags, int32_t* count,
                            uint8_t* lens, uint8_t* keys) {
    if (b->split) return fail(TETRIS_E_ARG, "tetris_action_lists_dev is not available on split batches");
    if (!count || !lens || !keys) return fail(TETRIS_E_ARG, "count/lens/keys are NULL");
    if (max_lists < 1 || max_keys < 1 || max_keys > 254) return fail(TETRIS_E_ARG, "max_lists >= 1, 1 <= max_keys <= 254");
    if (flags & ~TETRIS_LISTS_KEEP_NULL) return fail(TETRIS_E_ARG, "unknown flag");
    int rc = finish_call(b); if (rc) return rc;          // (the product polls its flag words here instead)
    const int KS = max_keys + 1;
    const size_t lanes = (size_t)b->N * 40;
    std::vector<uint8_t> hc(lanes), hl(lanes * PLAN_LANE_LISTS), hk(lanes * PLAN_LANE_LISTS * KS);
    uint32_t scratch_status[NFLAGS] = {0};
    for (size_t t = 0; t < lanes; t++) {
        if (b->P == 1) actions_body<1>(geo_of_batch(b), t, nullptr, player, b->H, SHAPES.s, hc.data(), hl.data(), hk.data(), PLAN_LANE_LISTS, KS, scratch_status);
        else if (b->P == 2) actions_body<2>(geo_of_batch(b), t, nullptr, player, b->H, SHAPES.s, hc.data(), hl.data(), hk.data(), PLAN_LANE_LISTS, KS, scratch_status);
        else if (b->P == 3) actions_body<3>(geo_of_batch(b), t, nullptr, player, b->H, SHAPES.s, hc.data(), hl.data(), hk.data(), PLAN_LANE_LISTS, KS, scratch_status);
        else actions_body<4>(geo_of_batch(b), t, nullptr, player, b->H, SHAPES.s, hc.data(), hl.data(), hk.data(), PLAN_LANE_LISTS, KS, scratch_status);
    }
    for (int i = 0; i < b->N; i++)
        plan_compact_serial(hc.data(), hl.data(), hk.data(), KS, (size_t)i * 40, (size_t)i, max_lists, max_keys,
                            (flags & TETRIS_LISTS_KEEP_NULL) != 0, count, lens, keys, b->flags);
    return TETRIS_OK;
}

int tetris_simulate_lists_dev(tetris_batch* b, const uint8_t* player, const int32_t* count, const uint8_t* lens, const uint8_t* keys,
                              int max_lists, int max_keys, int ms, int flags, uint32_t* cols, uint8_t* done, uint8_t* lines,
                              uint8_t* dead) {
    if (b->split) return fail(TETRIS_E_ARG, "tetris_simulate_lists_dev is not available on split batches");
    if (!count || !lens || !keys || !cols) return fail(TETRIS_E_ARG, "count/lens/keys/cols are NULL");
    if (max_lists < 1 || max_lists > 65535 || max_keys < 1 || max_keys > 255) return fail(TETRIS_E_ARG, "1 <= max_lists <= 65535, 1 <= max_keys <= 255");
    if (flags & ~TETRIS_SIM_FINALIZE) return fail(TETRIS_E_ARG, "unknown flag");
    int rc = finish_call(b); if (rc) return rc;
    PlanArgs pa = plan_args(b, player, count, lens, keys, max_lists, max_keys, ms);
    pa.cols = cols;
    const int fin = (flags & TETRIS_SIM_FINALIZE) ? 1 : 0;
    if (fin) { pa.a.done = done; pa.a.lines = lines; pa.a.dead = dead; }
    if (b->tint) sim_all<true>(b, pa, fin); else sim_all<false>(b, pa, fin);
    return TETRIS_OK;
}

int tetris_step_lists_dev(tetris_batch* b, const uint8_t* player, const int32_t* choice, const int32_t* count, const uint8_t* lens,
                          const uint8_t* keys, int max_lists, int max_keys, int ms, int flags, uint8_t* done, uint8_t* lines,
                          uint8_t* dead) {
    if (b->split) return fail(TETRIS_E_ARG, "tetris_step_lists_dev is not available on split batches");
    if (!choice || !count || !lens || !keys) return fail(TETRIS_E_ARG, "choice/count/lens/keys are NULL");
    if (max_lists < 1 || max_keys < 1 || max_keys > 255) return fail(TETRIS_E_ARG, "max_lists >= 1, 1 <= max_keys <= 255");
    if (flags & ~TETRIS_STEP_AUTO_RESET) return fail(TETRIS_E_ARG, "unknown flag");
    int rc = finish_call(b); if (rc) return rc;
    PlanArgs pa = plan_args(b, player, count, lens, keys, max_lists, max_keys, ms);
    pa.choice = choice;
    pa.a.done = done; pa.a.lines = lines; pa.a.dead = dead;
    const bool autoreset = (flags & TETRIS_STEP_AUTO_RESET) != 0;
    if (b->tint) { if (autoreset) step_all<true, true>(b, pa); else step_all<true, false>(b, pa); }
    else { if (autoreset) step_all<false, true>(b, pa); else step_all<false, false>(b, pa); }
    return TETRIS_OK;
}

}  // extern "C"
