// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there):
// tetris_traj_observe_dev, tetris_traj_select_dev and tetris_traj_batch_dev on 65 games (a block of 64 and one more), one
// and two players, heights 8 and 7, every row of a window of 5 rows, selections with and without the augmented copy into lists
// larger than, equal to and smaller than the result, and minibatches of 1, 64 and 131 entries with mirrored, repeated, -1 and
// out-of-range ones — with buffers of exactly the documented sizes on the heap so that a read or write past an end is reported.
#include "standalone.h"

static int run(int P, int H) {
    const int N = 65, T = 5;
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    std::vector<int16_t> seeds(N);
    for (int i = 0; i < N; i++) seeds[i] = (int16_t)(4321 + 7919 * i);
    tetris_batch* b = nullptr;
    if (tetris_create(&b, N, P, H, 10, map, 0, seeds.data())) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
    uint32_t s = 17u + (uint32_t)(P + H);
    std::vector<uint8_t> player(N), rot(N), trans(N), done(N), lines((size_t)P * N), dead((size_t)P * N);
    std::vector<uint8_t> w_action((size_t)T * N * 4), w_done((size_t)T * N), mask((size_t)T * N);
    std::vector<float> w_prob((size_t)T * N), w_value(2 * (size_t)T * N), w_reward((size_t)T * N), adv((size_t)T * N), target((size_t)T * N);
    std::vector<uint32_t> w_obs((size_t)T * N * P * 12);
    tetris_traj traj;
    memset(&traj, 0, sizeof traj);
    traj.capacity = T;
    traj.d_action = w_action.data(); traj.d_prob = w_prob.data(); traj.d_value = w_value.data(); traj.d_reward = w_reward.data();
    traj.d_done = w_done.data();
    tetris_traj_obs obs = {T, 0, w_obs.data()};
    int rc = 0;
    for (int row = 0; row < T && !rc; row++) {
        for (int i = 0; i < N; i++) { player[i] = (uint8_t)(lcg(s) % (uint32_t)P); rot[i] = (uint8_t)(lcg(s) & 3u); trans[i] = (uint8_t)(lcg(s) % 10u); }
        rc = tetris_traj_observe_dev(b, &obs, row, row & 1 ? player.data() : nullptr);
        if (!rc) rc = tetris_step_rt_dev_ex(b, rot.data(), trans.data(), player.data(), 400, done.data(), lines.data(), dead.data(), TETRIS_STEP_AUTO_RESET);
        for (int i = 0; i < N; i++) { w_action[((size_t)row * N + i) * 4 + 1] = trans[i]; w_action[((size_t)row * N + i) * 4 + 2] = (uint8_t)(lcg(s) % 7u); }
    }
    long long k = 0;
    for (auto& v : mask) { v = (uint8_t)(lcg(s) % 3u == 0 ? 1 + lcg(s) % 255u : 0); k += v != 0; }
    for (int rows : {1, T})
        for (int augment = 0; augment < 2 && !rc; augment++)
            for (long long cap : {0LL, k / 2, 2 * k, 2 * k + 7}) {
                std::vector<int32_t> index((size_t)cap);
                int32_t count = -5, dummy = 0;
                rc = tetris_traj_select_dev(b, mask.data(), rows, augment ? TETRIS_SELECT_AUGMENT : 0, cap ? index.data() : &dummy, cap, &count);
                if (rc) break;
                if (count < 0) { fprintf(stderr, "count not written\n"); rc = 1; break; }
            }
    for (int M : {1, 64, 131}) {
        if (rc) break;
        std::vector<int32_t> index((size_t)M);
        for (int j = 0; j < M; j++) {
            uint32_t e = lcg(s) % (uint32_t)(T * N);
            if (j % 7 == 3) e = 0xFFFFFFFFu;
            if (j % 11 == 5) e = (uint32_t)(T * N);
            if (j % 5 == 0) e = (uint32_t)(T * N - 1);
            if (lcg(s) & 1u) e |= 0x80000000u;
            index[(size_t)j] = (int32_t)e;
        }
        std::vector<uint8_t> visual((size_t)P * M * H * 10), vector((size_t)P * M * 12), piece((size_t)P * M), action((size_t)M * 3), o_done(M), valid(M);
        std::vector<float> prob(M), o_adv(M), o_target(M), reward(M);
        tetris_traj_batch out = {visual.data(), vector.data(), piece.data(), action.data(), prob.data(), o_adv.data(), o_target.data(), reward.data(),
                                 o_done.data(), valid.data()};
        rc = tetris_traj_batch_dev(b, &traj, &obs, adv.data(), M == 64 ? nullptr : target.data(), index.data(), M, &out);
        tetris_traj_batch only = {};
        only.d_vector = vector.data() + 0;
        if (!rc) rc = tetris_traj_batch_dev(b, &traj, &obs, nullptr, nullptr, index.data(), M, &only);
    }
    if (!rc) {
        int32_t index[1] = {0}, count = 0;
        tetris_traj_batch none = {};
        REFUSED(tetris_traj_observe_dev(b, &obs, T, nullptr));                                        // traj_observe_args
        REFUSED(tetris_traj_select_dev(b, mask.data(), 0, 0, index, 1, &count));                      // traj_select_args
        REFUSED(tetris_traj_batch_dev(b, &traj, &obs, nullptr, nullptr, index, -1, &none));           // traj_batch_args
    }
    if (rc) fprintf(stderr, "P=%d H=%d: rc %d: %s\n", P, H, rc, tetris_last_error());
    tetris_destroy(b);
    return rc;
}

int main() {
    int rc = 0;
    for (int P = 1; P <= 2; P++)
        for (int H : {8, 7}) rc |= run(P, H);
    printf(rc ? "FAILED\n" : "batch: ran clean\n");
    return rc ? 1 : 0;
}
