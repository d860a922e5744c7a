// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there):
// both capacity limits of include/tetris_hip.h where the limit is the END OF THE ALLOCATION.
// A fresh process has RNG tables of exactly two chunks, a vector of 2 * 65536 * 624 bytes; with
// tetris_debug_table_limit(b, 2) the draw limit is the last byte of it, so a table read that the clamps of table_byte /
// table_group_raw (tetris_engine.h) let past the limit is a heap-buffer-overflow here.  (On the GPU the tests keep the limit below
// the allocation: tests/test_capacity.py.)  65 games (a block of 64 and one more) of one and of two players, O pieces laid side by
// side to draw 1238, then 16 steps each of step_rt, step_keys, the auto-reset step, the list step with the finalized simulation of
// all lists before it, the policy step, and the random rollout un-fused and fused — each from the same boards, each must end games
// with TETRIS_ERR_STREAM.  Then the queue: two players at 10 ms, 8 packets pending on player 1, 16 random steps: a ninth packet must
// be refused (TETRIS_ERR_FIFO) without a write past qcount / qdelay.
#include "standalone.h"

static const int N = 65, H = 20, STEPS = 16, L = 64, K = 48;
static const uint8_t O_ONLY[7] = {6, 6, 6, 6, 6, 6, 6};

static int expect_bits(tetris_batch* b, uint32_t want, const char* what, int ended, uint32_t seen = 0) {
    uint32_t bits = 0;
    CHECK(tetris_take_errors(b, &bits));
    bits |= seen;
    if (bits != want || !ended) { fprintf(stderr, "%s: error bits %u (want %u), %d games ended\n", what, bits, want, ended); return 1; }
    return 0;
}

static int draws(int P) {
    std::vector<int16_t> seeds(N);
    for (int i = 0; i < N; i++) seeds[i] = (int16_t)(12345 + 7919 * i);
    tetris_batch* b = nullptr;
    CHECK(tetris_create(&b, N, P, H, 10, O_ONLY, 0, seeds.data()));
    if (tetris_table_chunks(b) != 2) { fprintf(stderr, "the tables have %d chunks, not 2\n", tetris_table_chunks(b)); return 1; }
    CHECK(tetris_debug_table_limit(b, 2));
    std::vector<uint8_t> rot(N, 0), trans(N), player(N), done(N), lines((size_t)P * N), dead((size_t)P * N);
    for (int s = 0; s < 2 * CHUNK - 12; s++) {                   // two draws at the reset, one per step: 1238
        for (int i = 0; i < N; i++) { trans[i] = (uint8_t)(2 * ((s / P) % 5)); player[i] = (uint8_t)(s % P); }
        CHECK(tetris_step_rt(b, rot.data(), trans.data(), player.data(), 400, done.data(), nullptr, nullptr));
        for (int i = 0; i < N; i++) if (done[i]) { fprintf(stderr, "game %d ended in preparation step %d\n", i, s); return 1; }
    }
    if (tetris_table_chunks(b) != 2) { fprintf(stderr, "the tables grew past the limit\n"); return 1; }
    uint32_t bits = 0;
    CHECK(tetris_take_errors(b, &bits));
    if (bits) { fprintf(stderr, "the preparation raised %u\n", bits); return 1; }
    std::vector<uint32_t> blob((size_t)N * tetris_snapshot_words(b));
    CHECK(tetris_snapshot(b, nullptr, N, blob.data()));
    std::vector<uint8_t> keys((size_t)N * P * 16), lens((size_t)N * P);
    std::vector<int32_t> count(N), choice(N);
    std::vector<uint8_t> l_lens((size_t)N * L), l_keys((size_t)N * L * K), s_done((size_t)L * N);
    std::vector<uint32_t> cols((size_t)L * P * 10 * N);
    const int16_t weights[8] = {76, -71, -18, -51, 0, 0, 0, 0};
    uint32_t s = 7u + (uint32_t)P;
    const char* names[] = {"step_rt", "step_keys", "auto-reset step", "list step", "policy step", "rollout", "fused rollout"};
    for (int path = 0; path < 7; path++) {
        CHECK(tetris_restore(b, nullptr, N, blob.data()));
        int ended = 0;
        uint32_t seen = 0;
        uint64_t counters[4] = {0, 0, 0, 0};
        if (path == 5) CHECK(tetris_rollout_random(b, STEPS, 1, 0xD71, 0, 400, counters, nullptr));
        if (path == 6) CHECK(tetris_rollout_random(b, 1, STEPS, 0xD71, 0, 400, counters, nullptr));
        if (path >= 5) ended = (int)counters[1];
        for (int step = 0; step < STEPS && path < 5; step++) {
            for (int i = 0; i < N; i++) { rot[i] = (uint8_t)(lcg(s) & 3u); trans[i] = (uint8_t)(lcg(s) % 10u); player[i] = (uint8_t)(step % P); }
            if (path == 0) CHECK(tetris_step_rt(b, rot.data(), trans.data(), player.data(), 400, done.data(), lines.data(), dead.data()));
            if (path == 1) {
                std::fill(keys.begin(), keys.end(), 0); std::fill(lens.begin(), lens.end(), 1);
                for (int i = 0; i < N; i++) {
                    uint8_t* k = &keys[((size_t)i * P + player[i]) * 16];
                    int n = 0;
                    for (int r = 0; r < rot[i]; r++) k[n++] = 8;
                    k[n++] = 2;
                    for (int t = 0; t < trans[i]; t++) k[n++] = 3;
                    k[n++] = 7;
                    lens[(size_t)i * P + player[i]] = (uint8_t)n;
                }
                CHECK(tetris_step_keys(b, nullptr, N, keys.data(), lens.data(), 16, 400, done.data(), lines.data(), dead.data()));
            }
            if (path == 2) CHECK(tetris_step_rt_dev_ex(b, rot.data(), trans.data(), player.data(), 400, done.data(), lines.data(), dead.data(), TETRIS_STEP_AUTO_RESET));
            if (path == 3) {
                CHECK(tetris_action_lists_dev(b, player.data(), L, K, 0, count.data(), l_lens.data(), l_keys.data()));
                CHECK(tetris_simulate_lists_dev(b, player.data(), count.data(), l_lens.data(), l_keys.data(), L, K, 400, TETRIS_SIM_FINALIZE, cols.data(),
                                                s_done.data(), nullptr, nullptr));
                uint32_t sim_bits = 0;
                CHECK(tetris_take_errors(b, &sim_bits));
                if (sim_bits) { fprintf(stderr, "a simulation raised %u\n", sim_bits); return 1; }
                for (int i = 0; i < N; i++) choice[i] = (int32_t)(lcg(s) % 64u);
                CHECK(tetris_step_lists_dev(b, player.data(), choice.data(), count.data(), l_lens.data(), l_keys.data(), L, K, 400, TETRIS_STEP_AUTO_RESET,
                                            done.data(), lines.data(), dead.data()));
                CHECK(tetris_take_errors(b, &sim_bits));           // (the step's own, so that the next simulation's check starts from none)
                seen |= sim_bits;
            }
            if (path == 4) CHECK(tetris_step_policy_dev(b, player.data(), weights, 0, 400, TETRIS_STEP_AUTO_RESET, done.data(), lines.data(), dead.data(), rot.data(), trans.data()));
            CHECK(tetris_sync(b));
            for (int i = 0; i < N; i++) ended += done[i] && (path >= 2 || step < 10);        // (without auto-reset an ended game stays done)
        }
        if (expect_bits(b, TETRIS_ERR_STREAM, names[path], ended, seen)) return 1;
        if (tetris_table_chunks(b) != 2) { fprintf(stderr, "%s: the tables grew past the limit\n", names[path]); return 1; }
    }
    tetris_destroy(b);
    return 0;
}

static int queue() {
    const int P = 2;
    tetris_batch* b = nullptr;
    CHECK(tetris_create(&b, N, P, H, 10, O_ONLY, 0, nullptr));
    std::vector<uint8_t> rot(N, 0), trans(N), player(N, 0), done(N), lines((size_t)P * N), dead((size_t)P * N);
    for (int s = 0; s < 35; s++) {
        for (int i = 0; i < N; i++) trans[i] = (uint8_t)(2 * (s % 5));
        CHECK(tetris_step_rt(b, rot.data(), trans.data(), player.data(), 10, done.data(), nullptr, nullptr));
    }
    std::vector<tetris_record> rec((size_t)N * P);
    CHECK(tetris_observe_records(b, nullptr, N, rec.data(), nullptr, nullptr));
    for (int i = 0; i < N; i++) if (rec[(size_t)i * P + 1].fifo_len != 8) { fprintf(stderr, "game %d: %d packets pending, not 8\n", i, rec[(size_t)i * P + 1].fifo_len); return 1; }
    uint32_t s = 3u;
    int ended = 0;
    uint64_t counters[4] = {0, 0, 0, 0};
    for (int step = 0; step < STEPS; step++) {
        for (int i = 0; i < N; i++) { rot[i] = (uint8_t)(lcg(s) & 3u); trans[i] = (uint8_t)(lcg(s) % 10u); player[i] = (uint8_t)(step % P); }
        if (step < 12) CHECK(tetris_step_rt_dev_ex(b, rot.data(), trans.data(), player.data(), 10, done.data(), lines.data(), dead.data(), 0));
        else CHECK(tetris_rollout_random(b, 1, 1, 0xD71, (uint64_t)step, 10, counters, nullptr));
        CHECK(tetris_sync(b));
    }
    for (int i = 0; i < N; i++) ended += done[i];
    CHECK(tetris_observe_records(b, nullptr, N, rec.data(), nullptr, nullptr));
    if (expect_bits(b, TETRIS_ERR_FIFO, "queue", ended + (int)counters[1])) return 1;
    tetris_destroy(b);
    return 0;
}

static int refusals() {
    const int P = 2;
    tetris_batch* b = nullptr;
    REFUSED(tetris_create(&b, N, P, 3, 10, O_ONLY, 0, nullptr));                                                      // create_check
    CHECK(tetris_create(&b, N, P, H, 10, O_ONLY, 0, nullptr));
    const int32_t past[1] = {N};
    std::vector<uint8_t> keys((size_t)N * P * 4), lens((size_t)N * P, 5), player(N, 2), l_lens((size_t)N * L), l_keys((size_t)N * L * K), out((size_t)N * P * H * 10);
    std::vector<int32_t> count(N, -7);
    std::vector<uint32_t> cols(16);
    const int16_t weights[8] = {76, -71, -18, -51, 0, 0, 0, 0};
    REFUSED(tetris_reset(b, past, 1, nullptr));                                                                       // check_idx
    REFUSED(tetris_step_rt(b, keys.data(), keys.data(), player.data(), 400, nullptr, nullptr, nullptr));              // check_players
    REFUSED(tetris_step_keys(b, nullptr, N, nullptr, lens.data(), 4, 400, nullptr, nullptr, nullptr));                // keys_check
    REFUSED(tetris_make_actions(b, nullptr, N, keys.data(), lens.data(), 4));                                         // keys_pack
    REFUSED(tetris_get_actions(b, nullptr, N, nullptr, l_keys.data(), l_lens.data(), count.data(), 0, K));            // get_actions_check
    REFUSED(tetris_get_actions(b, nullptr, N, nullptr, l_keys.data(), l_lens.data(), count.data(), 2, K));            // get_actions_gather
    if (count[0] != 2 || count[1] != -7) { fprintf(stderr, "get_actions: count %d, %d\n", count[0], count[1]); return 1; }
    REFUSED(tetris_observe_packed(b, nullptr, N, nullptr, nullptr, out.data(), out.data()));                          // observe_packed_outputs_check
    REFUSED(tetris_enumerate_drops(b, nullptr, N + 1, nullptr, out.data(), (int8_t*)out.data(), out.data(), nullptr)); // enumerate_check
    REFUSED(tetris_action_lists_dev(b, nullptr, L, 255, 0, count.data(), l_lens.data(), l_keys.data()));              // action_lists_check
    REFUSED(tetris_simulate_lists_dev(b, nullptr, count.data(), l_lens.data(), l_keys.data(), L, K, 400, 2, cols.data(), nullptr, nullptr, nullptr));   // simulate_lists_check
    REFUSED(tetris_step_lists_dev(b, nullptr, nullptr, count.data(), l_lens.data(), l_keys.data(), L, K, 400, 0, nullptr, nullptr, nullptr));           // step_lists_check
    REFUSED(tetris_step_policy_dev(b, nullptr, nullptr, 0, 400, 0, nullptr, nullptr, nullptr, nullptr, nullptr));     // policy_check
    REFUSED(tetris_rollout_policy(b, 1, 0, weights, 0, 0, 400, nullptr, nullptr));                                    // rollout_policy_check
    REFUSED(tetris_rollout_launch(b, 0, 1, 0xD71, 0, 400, nullptr));                                                  // rollout_launch_check
    REFUSED(tetris_split_rollout_stage_dev(b, 0, 0xD71, 0, 400, nullptr, cols.data()));                               // split_stage_check
    REFUSED(tetris_debug_table_limit(b, 65));                                                                         // table_limit_check
    REFUSED(tetris_take_errors(b, nullptr));                                                                          // take_errors_check
    tetris_destroy(b);
    CHECK(tetris_create_split(&b, N, 0, H, 10, O_ONLY, 0, nullptr));
    REFUSED(tetris_reset_dev(b, nullptr, nullptr));                                                                   // not_on_split
    REFUSED(tetris_split_stage_dev(b, 0, nullptr, nullptr, nullptr, 400, nullptr, cols.data(), nullptr, nullptr, nullptr));   // split_step_check
    tetris_destroy(b);
    return 0;
}

int main() {
    if (draws(1) || draws(2) || queue() || refusals()) return 1;
    printf("capacity: draw limit at the end of the allocation (1 and 2 players, 7 step paths) and the ninth packet: clean\n");
    return 0;
}
