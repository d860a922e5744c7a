// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there):
// tetris_select_eval_dev, tetris_step_eval_dev and tetris_step_eval_observe_dev on 65 games (a block of 64 and one more),
// every mode, float32 and binary16 evaluations, K = 7 and 1, one and two players, with buffers of exactly the documented
// sizes on the heap so that a read or write past an end is reported.
#include "standalone.h"

#include <memory>

static int refusals(tetris_batch* b, tetris_act_eval e, uint8_t* done, uint8_t* visual, uint8_t* vector, uint8_t* piece) {
    tetris_act_eval bad = e;
    bad.n_pieces = 5;
    REFUSED(tetris_select_eval_dev(b, &bad));                                                              // act_args
    REFUSED(tetris_step_eval_dev(b, &e, 400, 2, done, nullptr, nullptr));                                  // step_eval_check
    REFUSED(tetris_step_eval_observe_dev(b, &e, 400, 0, done, nullptr, nullptr, nullptr, nullptr, vector, piece));   // step_eval_observe_check
    REFUSED(tetris_step_rt_dev_ex(b, nullptr, e.d_trans, nullptr, 400, done, nullptr, nullptr, 0));        // step_rt_check
    REFUSED(tetris_step_rt_observe_dev(b, e.d_rot, e.d_trans, nullptr, 400, done, nullptr, nullptr, 4, nullptr, visual, vector, piece));   // step_rt_observe_check
    REFUSED(tetris_observe_packed_dev(b, nullptr, 66, nullptr, visual, vector, piece));                    // observe_packed_check
    uint32_t cols[4] = {0};
    int32_t count[1] = {0};
    REFUSED(tetris_plan_deltas_dev(b, nullptr, count, cols, 257, 1e-3f, 0, cols, nullptr, nullptr));       // plan_deltas_args
    return 0;
}

static int run(int P, int K, bool f16) {
    const int N = 65, H = 20;
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    std::vector<int16_t> seeds(N);
    for (int i = 0; i < N; i++) seeds[i] = (int16_t)(12345 + 7919 * i);
    tetris_batch* b = nullptr;
    if (tetris_create(&b, N, P, H, 10, map, 0, seeds.data())) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
    uint32_t s = 7u + (uint32_t)(P * 100 + K * 10 + f16);
    const size_t n_eval = (size_t)N * 40 * K, V = 7;
    // 16-byte aligned, exactly n_eval elements
    std::unique_ptr<uint8_t[], void (*)(void*)> eval_mem((uint8_t*)aligned_alloc(16, (n_eval * (f16 ? 2 : 4) + 15) / 16 * 16), free);
    std::vector<float> eval32(n_eval), value32((size_t)N * V);
    for (size_t k = 0; k < n_eval; k++) eval32[k] = (float)(lcg(s) % 2001) / 1000.0f - 0.5f;
    for (auto& v : value32) v = (float)(lcg(s) % 100) / 10.0f;
    eval32[3] = NAN; eval32[5 * 40 * K] = INFINITY;
    std::vector<uint16_t> value16(value32.size());
    for (size_t k = 0; k < value32.size(); k++) value16[k] = plan_f32_to_f16(value32[k]);
    if (f16) for (size_t k = 0; k < n_eval; k++) ((uint16_t*)eval_mem.get())[k] = plan_f32_to_f16(eval32[k]);
    else memcpy(eval_mem.get(), eval32.data(), n_eval * 4);
    std::vector<uint8_t> player(N), rot(N), trans(N), piece(N), done(N), lines((size_t)P * N), dead((size_t)P * N);
    std::vector<uint8_t> visual((size_t)P * N * H * 10), vector((size_t)P * N * 12), obs_piece((size_t)P * N);
    std::vector<float> chosen(N), value(2 * (size_t)N), entropy(N), table(40);
    for (int k = 0; k < 40; k++) table[k] = 1.0f / (float)(k + 1);
    int rc = 0;
    for (int step = 0; step < 24 && !rc; step++) {
        for (int i = 0; i < N; i++) player[i] = (uint8_t)(lcg(s) % (uint32_t)P);
        tetris_act_eval e;
        memset(&e, 0, sizeof e);
        e.d_action_eval = eval_mem.get();
        e.d_state_eval = f16 ? (const void*)value16.data() : (const void*)value32.data();
        e.n_pieces = K; e.n_values = (int)V;
        e.mode = step % 4;
        e.flags = f16 ? TETRIS_ACT_F16 | TETRIS_ACT_VALUE_F16 : 0;
        e.sample_seed = 99; e.draw = (uint64_t)step; e.epsilon = 0.5f;
        e.table = e.mode == TETRIS_ACT_RANK ? table.data() : nullptr;
        e.d_player = player.data();
        e.d_rot = rot.data(); e.d_trans = trans.data(); e.d_piece = piece.data();
        e.d_eval = chosen.data(); e.d_value = value.data(); e.d_entropy = e.mode == TETRIS_ACT_PI ? entropy.data() : nullptr;
        rc = tetris_select_eval_dev(b, &e);
        if (!rc) rc = tetris_step_eval_dev(b, &e, 400, TETRIS_STEP_AUTO_RESET, done.data(), lines.data(), dead.data());
        if (!rc) rc = tetris_step_eval_observe_dev(b, &e, 400, step & 1, done.data(), lines.data(), dead.data(), player.data(), visual.data(),
                                                   vector.data(), obs_piece.data());
        for (int i = 0; i < N && !rc; i++) if (rot[i] > 3 || trans[i] > 9 || piece[i] >= K) { fprintf(stderr, "choice out of range\n"); rc = 1; }
        // a round that ended is reset by hand where the step did not (every other observe step runs without auto-reset)
        if (!rc && !(step & 1)) rc = tetris_reset_dev(b, done.data(), nullptr);
        if (!rc && step == 23) rc = refusals(b, e, done.data(), visual.data(), vector.data(), obs_piece.data());
    }
    if (rc) fprintf(stderr, "P=%d K=%d f16=%d: rc %d: %s\n", P, K, (int)f16, rc, tetris_last_error());
    tetris_destroy(b);
    return rc;
}

int main() {
    int rc = 0;
    for (int P = 1; P <= 2; P++)
        for (int K : {7, 1})
            for (int f16 = 0; f16 < 2; f16++) rc |= run(P, K, f16 != 0);
    printf(rc ? "FAILED\n" : "act_eval: ran clean\n");
    return rc ? 1 : 0;
}
