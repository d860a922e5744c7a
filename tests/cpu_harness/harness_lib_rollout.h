// Host side of the CPU harness, part 2 (as tetris_lib_rollout.h): tetris_rollout_launch and the rollout counters.  Needs
// harness_lib_batch.h.  "Device" pointers are host pointers here.

// the counters of one rollout call, as the product takes them: a copy of the per-game words before, and afterwards
// (now - then) mod 2^32 per game summed in 64 bits (the words are cumulative and wrap)
static std::vector<uint32_t> game_words(tetris_batch* b) {
    std::vector<uint32_t> w((size_t)4 * b->N);
    for (int i = 0; i < b->N; i++) {
        unsigned long long t[4];
        totals_of_game(geo_of_batch(b), i, t);
        for (int k = 0; k < 4; k++) w[(size_t)k * b->N + i] = (uint32_t)t[k];
    }
    return w;
}
static int rollout_counters_begin(tetris_batch* b) {
    int rc = check_batch(b);
    if (rc) return rc;
    b->words_before = game_words(b);
    return TETRIS_OK;
}
static int rollout_counters_end(tetris_batch* b, uint64_t counters[4]) {
    const std::vector<uint32_t> now = game_words(b), & before = b->words_before;
    for (int k = 0; k < 4; k++)
        for (int i = 0; i < b->N; i++) counters[k] += (uint32_t)(now[(size_t)k * b->N + i] - before[(size_t)k * b->N + i]);
    return TETRIS_OK;
}

extern "C" {

int tetris_rollout_launch(tetris_batch* b, int launches, int steps_per_launch, uint32_t policy_seed, uint64_t first_step, int ms,
                          float* elapsed_ms) {
    int rc = rollout_launch_check(launches, steps_per_launch);
    if (rc) return rc;
    // the harness looks at the flag words after every launch, so the margin only has to cover one launch
    MarginGuard margin_guard(b, (uint32_t)(2 * steps_per_launch + 16));
    for (int l = 0; l < launches && !rc; l++) {
        KArgs a = base_args(b, b->N, nullptr);
        a.ms = ms; a.steps = steps_per_launch; a.policy_seed = policy_seed;
        a.first_step = first_step + (uint64_t)l * (uint64_t)steps_per_launch;
        run<M_ROLLOUT>(b, a);
        rc = finish_call(b);
    }
    if (elapsed_ms) *elapsed_ms = 0.0f;
    return rc;
}

}  // extern "C"
