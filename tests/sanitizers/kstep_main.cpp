// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there,
// NAME = kstep): the serial forms of tetris_replay_gather_steps_dev and tetris_kstep_target_dev on M = 65 samples of a ring with
// k_step = 37, the sparse step set of filter [2, 3] (13 steps) and the single step 37, one and two players — ring mode with indices
// at max_size - 1, -1, max_size and both ends of int32, array mode on the gathered rows, Q (K = 7 and 1) and V mode, float32 and
// binary16, with and without the optional outputs — with buffers of exactly the documented sizes on the heap, so that a read or
// write past an end is reported; then one refused call per argument rule.
#include "standalone.h"

#include <climits>
#include <memory>

typedef std::unique_ptr<uint8_t[], void (*)(void*)> Aligned;
static Aligned aligned(size_t bytes) { return Aligned((uint8_t*)aligned_alloc(16, (bytes + 15) / 16 * 16), free); }

// `count` elements of the element type, exactly: values in [-1, 1]
static Aligned elements(uint32_t& s, size_t count, bool f16) {
    Aligned mem = aligned(count * (f16 ? 2 : 4));
    for (size_t i = 0; i < count; i++) {
        const float v = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
        if (f16) ((uint16_t*)mem.get())[i] = plan_f32_to_f16(v);
        else ((float*)mem.get())[i] = v;
    }
    return mem;
}

static int run(int P) {
    const int M = 65, K_STEP = 37, MAX_SIZE = 120, C = MAX_SIZE + K_STEP, H = 8;
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    tetris_batch* b = nullptr;
    if (tetris_create(&b, 4, P, H, 10, map, 0, nullptr)) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
    uint32_t s = 41u + (uint32_t)P;
    std::vector<uint32_t> obs((size_t)C * P * 12);
    std::vector<uint8_t> action((size_t)C * 4), done(C), flags(C);
    std::vector<float> prob(C), adv(C), target(C), reward(C), prio(MAX_SIZE);
    std::vector<int32_t> cursor(4);
    for (int i = 0; i < MAX_SIZE; i++) {
        for (int w = 0; w < P * 12; w++) obs[(size_t)i * P * 12 + w] = lcg(s);
        reward[i] = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
        done[i] = lcg(s) % 9u == 0 ? (uint8_t)(1 + lcg(s) % 255u) : (uint8_t)0;
        flags[i] = (uint8_t)(lcg(s) & 1u);
    }
    tetris_replay rp = {C, K_STEP, obs.data(), action.data(), prob.data(), adv.data(), target.data(), reward.data(), done.data(), flags.data(),
                        prio.data(), cursor.data()};
    std::vector<int32_t> index(M);
    for (int j = 0; j < M; j++) index[j] = (int32_t)(lcg(s) % (uint32_t)MAX_SIZE);
    index[0] = MAX_SIZE - 1; index[1] = -1; index[2] = MAX_SIZE; index[3] = INT_MIN; index[4] = INT_MAX; index[5] = 0;
    uint64_t sparse = 0u;
    for (int st = 1; st <= K_STEP; st++)
        if (st % 2 && st % 3) sparse |= 1ull << st;
    const uint64_t one = 1u;
    for (uint64_t mask : {sparse, one << K_STEP, sparse | one, (one << (K_STEP + 1)) - one}) {
        // ---- the step-list gather: outputs sized for M * n samples
        const int n = __builtin_popcountll(mask);
        const size_t m = (size_t)M * n;
        std::vector<uint8_t> visual(m * P * H * 10), vector(m * P * 12), piece(m * P), o_action(m * 3), o_done(m), valid(m);
        std::vector<float> f_prob(m), f_adv(m), f_target(m), f_reward(m);
        tetris_traj_batch out = {visual.data(), vector.data(), piece.data(), o_action.data(), f_prob.data(), f_adv.data(), f_target.data(),
                                 f_reward.data(), o_done.data(), valid.data()};
        OK(tetris_replay_gather_steps_dev(b, &rp, index.data(), M, mask, &out));
        tetris_traj_batch none;
        memset(&none, 0, sizeof none);
        OK(tetris_replay_gather_steps_dev(b, &rp, index.data(), M, mask, &none));
        if (valid[0] != 1 || valid[(size_t)n] != 0 || valid[(size_t)5 * n] != 1) { fprintf(stderr, "valid\n"); return 1; }
        if (mask & 1ull) continue;                                  // (bit 0: the gather's own; the estimator refuses it)
        // ---- the estimator over the ring, and over the rows of the full gather
        const size_t full = (size_t)M * (K_STEP + 1);
        std::vector<float> g_reward(full);
        std::vector<uint8_t> g_done(full);
        memset(&none, 0, sizeof none);
        none.d_reward = g_reward.data(); none.d_done = g_done.data();
        OK(tetris_replay_gather_dev(b, &rp, index.data(), M, K_STEP + 1, &none));
        for (int K : {7, 1})
            for (int mode : {TETRIS_KSTEP_Q, TETRIS_KSTEP_V})
                for (int f16 = 0; f16 < 2; f16++)
                    for (int ring = 0; ring < 2; ring++)
                        for (int V : {1, K}) {
                            if (mode == TETRIS_KSTEP_Q && V != 1) continue;
                            const size_t per = mode == TETRIS_KSTEP_Q ? (size_t)40 * K : (size_t)V;
                            Aligned x = elements(s, m * per, f16 != 0);
                            std::vector<float> t_target(M), t_values(m);
                            std::vector<uint8_t> t_dt(M);
                            tetris_kstep_target t;
                            memset(&t, 0, sizeof t);
                            t.d_out = x.get();
                            t.d_reward = ring ? reward.data() : g_reward.data(); t.d_done = ring ? done.data() : g_done.data();
                            t.d_index = ring ? index.data() : nullptr; t.max_size = ring ? MAX_SIZE : 0;
                            t.M = M; t.k_step = K_STEP; t.step_mask = mask; t.mode = mode; t.n_pieces = K; t.n_values = V;
                            t.used_pieces = K == 7 ? 0x2D : 1; t.flags = (f16 ? TETRIS_LOSS_F16 : 0) | (ring ? TETRIS_KSTEP_TRUNCATE : 0);
                            t.gamma = 0.99f; t.lam = 0.9f;
                            t.d_target = t_target.data(); t.d_values = t_values.data(); t.d_done_time = t_dt.data();
                            OK(tetris_kstep_target_dev(b, &t));
                            if (ring && (t_target[1] != 0.0f || t_dt[2] != 0 || t_values[(size_t)3 * n] != 0.0f)) { fprintf(stderr, "an invalid sample\n"); return 1; }
                            t.d_values = nullptr; t.d_done_time = nullptr;
                            OK(tetris_kstep_target_dev(b, &t));
                            if (K != 7 || mode != TETRIS_KSTEP_Q || f16 || !ring || mask != sparse) continue;
                            t.d_values = t_values.data();
                            tetris_kstep_target bad = t;                           // kstep_target_args
                            REFUSED(tetris_kstep_target_dev(b, nullptr));
                            REFUSED(tetris_kstep_target_dev(nullptr, &t));
                            bad.M = -1; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.k_step = 0; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.k_step = 64; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.step_mask = 0u; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.step_mask |= 1u; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.step_mask |= 1ull << (K_STEP + 1); REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.n_pieces = 3; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.mode = TETRIS_KSTEP_V; bad.n_values = 2; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.mode = 2; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.used_pieces = 0; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.used_pieces = 0x80; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.flags = 2; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.max_size = 0; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.d_index = nullptr; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.d_out = x.get() + 4; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.d_target = nullptr; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.d_done = nullptr; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.M = 1 << 29; REFUSED(tetris_kstep_target_dev(b, &bad)); bad = t;
                            bad.M = 0; OK(tetris_kstep_target_dev(b, &bad));
                        }
    }
    // ---- the gather's own rules (replay_gather_steps_args)
    tetris_traj_batch none;
    memset(&none, 0, sizeof none);
    REFUSED(tetris_replay_gather_steps_dev(b, &rp, index.data(), M, 0u, &none));
    REFUSED(tetris_replay_gather_steps_dev(b, &rp, index.data(), M, 1ull << (K_STEP + 1), &none));
    REFUSED(tetris_replay_gather_steps_dev(b, &rp, index.data(), 1 << 30, 6u, &none));
    REFUSED(tetris_replay_gather_steps_dev(b, &rp, index.data(), -1, 2u, &none));
    REFUSED(tetris_replay_gather_steps_dev(b, &rp, nullptr, M, 2u, &none));
    REFUSED(tetris_replay_gather_steps_dev(b, &rp, index.data(), M, 2u, nullptr));
    REFUSED(tetris_replay_gather_steps_dev(b, nullptr, index.data(), M, 2u, &none));
    tetris_replay wide = rp;
    wide.k_step = 64; wide.capacity = MAX_SIZE / 2 + 64;
    REFUSED(tetris_replay_gather_steps_dev(b, &wide, index.data(), M, 2u, &none));
    tetris_destroy(b);
    return 0;
}

int main() {
    int rc = run(1) | run(2);
    printf(rc ? "FAILED\n" : "kstep: ran clean\n");
    return rc ? 1 : 0;
}
