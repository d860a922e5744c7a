// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there):
// tetris_step_eval_dev, tetris_traj_record_dev and tetris_traj_advantages_dev on 65 games (a block of 64 and one more), one
// and two players, every row of a window of 19 rows and advantages over 1, 16, 17 and 19 of them, with buffers of exactly the
// documented sizes on the heap so that a read or write past an end is reported.
#include "standalone.h"

static int run(int P) {
    const int N = 65, H = 8, T = 19;
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    std::vector<int16_t> seeds(N);
    for (int i = 0; i < N; i++) seeds[i] = (int16_t)(4321 + 7919 * i);
    tetris_batch* b = nullptr;
    if (tetris_create(&b, N, P, H, 10, map, 0, seeds.data())) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
    uint32_t s = 11u + (uint32_t)P;
    std::vector<float> eval((size_t)N * 40 * 7), state((size_t)N * 7);
    std::vector<uint8_t> player(N), rot(N), trans(N), piece(N), done(N), lines((size_t)P * N), dead((size_t)P * N);
    std::vector<float> chosen(N), value(2 * (size_t)N);
    std::vector<uint8_t> w_action((size_t)T * N * 4), w_done((size_t)T * N), closed((size_t)T * N);
    std::vector<float> w_prob((size_t)T * N), w_value(2 * (size_t)T * N), w_reward((size_t)T * N), boot(N), adv((size_t)T * N), target((size_t)T * N);
    tetris_traj traj;
    memset(&traj, 0, sizeof traj);
    traj.capacity = T;
    traj.d_action = w_action.data(); traj.d_prob = w_prob.data(); traj.d_value = w_value.data(); traj.d_reward = w_reward.data();
    traj.d_done = w_done.data();
    int rc = 0, ended = 0;
    for (int step = 0; step < T && !rc; step++) {
        for (auto& v : eval) v = (float)(lcg(s) % 2001) / 1000.0f;
        for (auto& v : state) v = (float)(lcg(s) % 100) / 10.0f - 5.0f;
        for (int i = 0; i < N; i++) player[i] = (uint8_t)(lcg(s) % (uint32_t)P);
        tetris_act_eval e;
        memset(&e, 0, sizeof e);
        e.d_action_eval = eval.data(); e.d_state_eval = state.data();
        e.n_pieces = 7; e.n_values = 7;
        e.mode = TETRIS_ACT_PI;
        e.sample_seed = 5; e.draw = (uint64_t)step;
        e.d_player = player.data();
        e.d_rot = rot.data(); e.d_trans = trans.data(); e.d_piece = piece.data();
        e.d_eval = chosen.data(); e.d_value = (step & 1) ? value.data() : nullptr;
        rc = tetris_step_eval_dev(b, &e, 400, TETRIS_STEP_AUTO_RESET, done.data(), lines.data(), dead.data());
        if (!rc) rc = tetris_traj_record_dev(b, &traj, step, &e, done.data(), dead.data());
        for (int i = 0; i < N; i++) ended += done[i];
    }
    for (auto& v : boot) v = (float)(lcg(s) % 100) / 10.0f - 5.0f;
    for (int rows : {1, 16, 17, T})
        if (!rc) rc = tetris_traj_advantages_dev(b, &traj, rows, P == 2 ? -0.98f : 0.98f, 0.96f, 0.95f, rows & 1 ? boot.data() : nullptr, adv.data(),
                                                 target.data(), rows == 16 ? nullptr : closed.data());
    if (!rc) {
        tetris_act_eval e;
        memset(&e, 0, sizeof e);
        e.d_rot = rot.data(); e.d_trans = trans.data(); e.d_piece = piece.data(); e.d_eval = chosen.data();
        REFUSED(tetris_traj_record_dev(b, &traj, T, &e, done.data(), dead.data()));                                              // traj_record_args
        REFUSED(tetris_traj_advantages_dev(b, &traj, T + 1, 0.98f, 0.96f, 0.95f, nullptr, adv.data(), target.data(), nullptr));   // traj_adv_args
    }
    if (!rc && !ended) { fprintf(stderr, "no game ended\n"); rc = 1; }
    if (rc) fprintf(stderr, "P=%d: rc %d: %s\n", P, rc, tetris_last_error());
    tetris_destroy(b);
    return rc;
}

int main() {
    int rc = 0;
    for (int P = 1; P <= 2; P++) rc |= run(P);
    printf(rc ? "FAILED\n" : "traj: ran clean\n");
    return rc ? 1 : 0;
}
