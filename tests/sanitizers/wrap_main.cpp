// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there):
// the built-in rollouts with the per-game counter words at 2^32, step numbers across 2^32
// and game ids that wrap inside the batch (tests/test_rollout_wrap.py compares the results with the oracle; here the
// sanitizers watch the same paths).  70 games of one, two and three players: the words G_EPISODE, G_STEPS, G_LINES, G_SENT are
// restored to 0xFFFFFFFF - (g mod 3), the game offset is 2^32 - 40, first_step 2^32 - 7; 40 / 60 / 120 steps of tetris_rollout_random
// at 3 000 ms (games end and are re-seeded) un-fused and fused, then 8 of tetris_rollout_policy.  counters[0] must be exactly the
// steps of the call, whatever the words held.
#include "standalone.h"

static const int N = 70, H = 20;
static const uint8_t ALL[7] = {0, 1, 2, 3, 4, 5, 6};

static int expect_steps(const uint64_t c[4], uint64_t steps, const char* what) {
    if (c[0] != steps || c[1] >> 32 || c[2] >> 32 || c[3] >> 32) {
        fprintf(stderr, "%s: counters %llu %llu %llu %llu, expected %llu env-steps\n", what, (unsigned long long)c[0], (unsigned long long)c[1],
                (unsigned long long)c[2], (unsigned long long)c[3], (unsigned long long)steps);
        return 1;
    }
    return 0;
}

static int wrap(int P) {
    const int K = P == 1 ? 40 : (P == 2 ? 60 : 120);      // (steps in which games of P players end at 3 000 ms per step)
    const uint64_t offset = (1ull << 32) - 40, first = (1ull << 32) - 7;
    std::vector<int16_t> seeds(N);
    for (int i = 0; i < N; i++) seeds[i] = (int16_t)(uint16_t)(12345u + 7919u * (uint32_t)(offset + (uint64_t)i));
    tetris_batch* b = nullptr;
    CHECK(tetris_create(&b, N, P, H, 10, ALL, 0, seeds.data()));
    CHECK(tetris_set_game_offset(b, offset));
    const int words = tetris_snapshot_words(b);
    std::vector<uint32_t> blob((size_t)N * words);
    CHECK(tetris_snapshot(b, nullptr, N, blob.data()));
    for (int g = 0; g < N; g++)
        for (int w = 1; w <= 4; w++) blob[(size_t)g * words + w] = 0xFFFFFFFFu - (uint32_t)(g % 3);
    CHECK(tetris_restore(b, nullptr, N, blob.data()));
    uint64_t c[4] = {0, 0, 0, 0};
    CHECK(tetris_rollout_random(b, K, 1, 0xD71, first, 3000, c, nullptr));
    if (expect_steps(c, (uint64_t)N * K, "un-fused rollout")) return 1;
    if (!c[1]) { fprintf(stderr, "%d players: no episode ended\n", P); return 1; }
    uint64_t c4[4] = {0, 0, 0, 0};
    CHECK(tetris_rollout_random(b, K / 4, 4, 0xD71, first + K - 2, 3000, c4, nullptr));
    if (expect_steps(c4, (uint64_t)N * K, "fused rollout")) return 1;
    const int16_t weights[8] = {34, -79, 0, -10, 0, -32, -93, -34};
    uint64_t cp[4] = {0, 0, 0, 0};
    CHECK(tetris_rollout_policy(b, 4, 1, weights, 0, first, 400, cp, nullptr));
    CHECK(tetris_rollout_policy(b, 1, 4, weights, 0, first + 4, 400, cp, nullptr));
    if (expect_steps(cp, (uint64_t)N * 8, "policy rollout")) return 1;
    std::vector<uint32_t> totals((size_t)4 * N);
    CHECK(tetris_rollout_game_totals_dev(b, totals.data()));
    for (int g = 0; g < N; g++)
        if (totals[g] != (uint32_t)(0xFFFFFFFFu - (uint32_t)(g % 3) + 2u * K + 8u)) { fprintf(stderr, "game %d: env-step word %u\n", g, totals[g]); return 1; }
    uint32_t bits = 0;
    CHECK(tetris_take_errors(b, &bits));
    if (bits) { fprintf(stderr, "error bits %u\n", bits); return 1; }
    tetris_destroy(b);
    return 0;
}

int main() {
    if (wrap(1) || wrap(2) || wrap(3)) return 1;
    printf("wrap: counter words at 2^32, steps across 2^32, game ids wrapping inside the batch (1, 2 and 3 players): clean\n");
    return 0;
}
