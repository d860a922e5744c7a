// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there):
// tetris_replay_add_dev, tetris_replay_sample_dev, tetris_replay_update_prios_dev and tetris_replay_gather_dev on 65
// games, one and two players, heights 8 and 7 — adds that fit, wrap and overflow the ring, with and without the mirrored copies
// and the optional arrays; samples of 0, 1, n and n + 7 entries from rings of 1, tile - 1, tile + 1 and 2 tile + 5 priorities of
// random bits (NaNs among them) with cursors that say 0, a part and all of it and one that says nonsense; updates and gathers
// with -1, max_size and out-of-range indices, every number of steps — with buffers of exactly the documented sizes on the heap,
// so that a read or write past an end is reported.
#include "standalone.h"

struct Ring {
    std::vector<uint32_t> obs;
    std::vector<uint8_t> action, done, flags;
    std::vector<float> prob, adv, target, reward, prio;
    std::vector<int32_t> cursor;
    tetris_replay rp;
    Ring(int C, int k_step, int S, bool arrays = true)
        : obs(arrays ? (size_t)C * S * 12 : 0), action(arrays ? (size_t)C * 4 : 0), done(arrays ? C : 0), flags(arrays ? C : 0),
          prob(arrays ? C : 0), adv(arrays ? C : 0), target(arrays ? C : 0), reward(arrays ? C : 0), prio((size_t)(C - k_step)), cursor(4) {
        rp.capacity = C; rp.k_step = k_step;
        rp.d_obs = arrays ? obs.data() : nullptr; rp.d_action = arrays ? action.data() : nullptr; rp.d_prob = arrays ? prob.data() : nullptr;
        rp.d_adv = arrays ? adv.data() : nullptr; rp.d_target = arrays ? target.data() : nullptr; rp.d_reward = arrays ? reward.data() : nullptr;
        rp.d_done = arrays ? done.data() : nullptr; rp.d_flags = arrays ? flags.data() : nullptr;
        rp.d_prio = prio.data(); rp.d_cursor = cursor.data();
    }
};

static int run(int P, int H) {
    const int N = 65, T = 5, K = 3;
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    std::vector<int16_t> seeds(N, 1234);
    tetris_batch* b = nullptr;
    if (tetris_create(&b, N, P, H, 10, map, 0, seeds.data())) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
    uint32_t s = 29u + (uint32_t)(P + H);
    std::vector<uint8_t> w_action((size_t)T * N * 4), w_done((size_t)T * N), mask((size_t)T * N);
    std::vector<float> w_prob((size_t)T * N), w_value(2 * (size_t)T * N), w_reward((size_t)T * N), adv((size_t)T * N), target((size_t)T * N), prio((size_t)T * N);
    std::vector<uint32_t> w_obs((size_t)T * N * P * 12);
    for (auto& v : w_obs) v = lcg(s);
    for (auto& v : w_action) v = (uint8_t)(lcg(s) % 7u);
    tetris_traj traj;
    memset(&traj, 0, sizeof traj);
    traj.capacity = T;
    traj.d_action = w_action.data(); traj.d_prob = w_prob.data(); traj.d_value = w_value.data(); traj.d_reward = w_reward.data();
    traj.d_done = w_done.data();
    tetris_traj_obs obs = {T, 0, w_obs.data()};
    // ---- add: rings that take the batch, that wrap on the second call and that are smaller than one batch
    for (int density = 0; density < 3; density++) {
        int k = 0;
        for (auto& m : mask) { m = density == 0 ? 0 : density == 1 ? (uint8_t)(lcg(s) % 3u == 0) : 1; k += m != 0; }
        for (int augment = 0; augment < 2; augment++)
            for (int max_size : {1, k / 2 + 1, k + 1, 3 * k + 7}) {
                Ring r(max_size + K, K, P);
                for (int call = 0; call < 3; call++)
                    OK(tetris_replay_add_dev(b, &r.rp, &traj, &obs, call ? adv.data() : nullptr, call ? target.data() : nullptr,
                                             call == 2 ? prio.data() : nullptr, mask.data(), T - (call == 1), augment));
                if (r.cursor[0] < 0 || r.cursor[0] > max_size || r.cursor[1] < r.cursor[0] || r.cursor[1] > max_size) { fprintf(stderr, "cursor\n"); return 1; }
                // ---- gather and update on what the adds left
                const int M = 70;
                std::vector<int32_t> index(M);
                for (int j = 0; j < M; j++) index[j] = (int32_t)(lcg(s) % (uint32_t)max_size);
                index[0] = -1; index[1] = max_size; index[2] = max_size - 1; index[3] = max_size + K; index[4] = INT32_MIN; index[5] = INT32_MAX;
                for (int steps = 1; steps <= K + 1; steps++) {
                    const size_t m = (size_t)M * steps;
                    std::vector<uint8_t> visual(m * P * H * 10), vector(m * P * 12), piece(m * P), action(m * 3), o_done(m), valid(m);
                    std::vector<float> f_prob(m), f_adv(m), f_target(m), f_reward(m);
                    tetris_traj_batch out = {visual.data(), vector.data(), piece.data(), action.data(), f_prob.data(), f_adv.data(), f_target.data(),
                                             f_reward.data(), o_done.data(), valid.data()};
                    OK(tetris_replay_gather_dev(b, &r.rp, index.data(), M, steps, &out));
                    if (valid[0] || valid[(size_t)steps] || !valid[2 * (size_t)steps]) { fprintf(stderr, "valid\n"); return 1; }
                }
                std::vector<float> np(M, 0.5f);
                OK(tetris_replay_update_prios_dev(b, &r.rp, index.data(), np.data(), M));
                tetris_traj_batch none;
                memset(&none, 0, sizeof none);
                REFUSED(tetris_replay_gather_dev(b, &r.rp, index.data(), M, K + 2, &none));
                REFUSED(tetris_replay_gather_dev(b, &r.rp, index.data(), M, 0, &none));
                REFUSED(tetris_replay_add_dev(b, &r.rp, &traj, &obs, nullptr, nullptr, nullptr, mask.data(), T + 1, 0));
                REFUSED(tetris_replay_add_dev(b, &r.rp, &traj, &obs, nullptr, nullptr, nullptr, mask.data(), T, 2));
            }
    }
    // ---- sample: priorities only
    for (int size : {1, SORT_TILE - 1, SORT_TILE + 1, 2 * SORT_TILE + 5}) {
        Ring r(size + K, K, P, false);
        for (auto& v : r.prio) { const uint32_t bits = (lcg(s) << 8) ^ lcg(s); memcpy(&v, &bits, 4); }
        for (int n : {0, size / 2, size, size + 100, -3}) {
            r.cursor[0] = 0; r.cursor[1] = n;
            const int live = n < 0 ? 0 : n > size ? size : n;
            for (int M : {0, 1, live, live + 7}) {
                std::vector<int32_t> index((size_t)M), count(1, -1), rank((size_t)size);
                std::vector<float> weight((size_t)M), key((size_t)size);
                OK(tetris_replay_sample_dev(b, &r.rp, M, 0.7f, 0.5f, 5u, ((uint64_t)9 << 32) | (uint32_t)M, M ? index.data() : (int32_t*)&count[0],
                                            M ? weight.data() : (float*)&key[0], count.data(), (M & 1) ? rank.data() : nullptr, (M & 1) ? key.data() : nullptr));
                if (count[0] != (M < live ? M : live)) { fprintf(stderr, "count %d, M %d, n %d\n", count[0], M, n); return 1; }
                for (int j = 0; j < M; j++)
                    if ((j < count[0]) != (index[j] >= 0 && index[j] < live)) { fprintf(stderr, "index[%d] = %d\n", j, index[j]); return 1; }
            }
        }
        REFUSED(tetris_replay_sample_dev(b, &r.rp, -1, 0.7f, 0.5f, 5u, 0, r.cursor.data(), r.prio.data(), r.cursor.data(), nullptr, nullptr));
        REFUSED(tetris_replay_gather_dev(b, &r.rp, r.cursor.data(), 1, 1, nullptr));
    }
    tetris_destroy(b);
    return 0;
}

int main() {
    for (int P = 1; P <= 2; P++)
        for (int H : {8, 7})
            if (run(P, H)) return 1;
    printf("replay: ok\n");
    return 0;
}
