// TEST INFRASTRUCTURE — NOT PRODUCT CODE, NOT A FALLBACK.
//
// The CPU test harness with the planning and heuristic-policy entry points (harness_policy.cpp, included whole) plus
// tetris_plan_deltas_dev of include/tetris_hip.h as a plain host loop over the same element logic
// (drl-tetris_amd/csrc/tetris_plan.h: plan_deltas_game).  "Device" pointers are host pointers here.
// __graft_entry__.build_harness compiles this file into libtetris_cpu_harness.so.  The checks and the PlanDeltaArgs fill are the
// product's (tetris_host.h: plan_deltas_args).
#include "harness_policy.cpp"

extern "C" {

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
