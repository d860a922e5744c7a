// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there,
// NAME = net_input): the serial form of tetris_net_input_dev on M = 1, 15, 17, 33 and 257 samples — one and two players, H = 4, 9,
// 20 and 31, every number of items, pad on and off, both layouts, float32 and binary16, a window's index list (mirrored entries, -1
// and T N among them), a row of the window and the replay ring with a count and a step list — with records and outputs of exactly the
// documented sizes on the heap, so that a read or write past an end is reported; then one refused call per argument rule.
#include "standalone.h"

#include <memory>
#include <vector>

typedef std::unique_ptr<uint8_t[], void (*)(void*)> Aligned;
static Aligned aligned(size_t bytes) { return Aligned((uint8_t*)aligned_alloc(16, (bytes + 15) / 16 * 16), free); }

// `count` random words: every bit of every column word, those at and above H included
static Aligned words(uint32_t& s, size_t count) {
    Aligned mem = aligned(count * 4);
    for (size_t i = 0; i < count; i++) ((uint32_t*)mem.get())[i] = (lcg(s) << 8) ^ lcg(s);
    return mem;
}

static int run() {
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    uint32_t s = 99u;
    const int T = 2, N = 33, k_step = 3, max_size = 41, cap = max_size + k_step;
    int n_case = 0;
    for (int P : {1, 2})
        for (int H : {4, 9, 20, 31}) {
            tetris_batch* b = nullptr;
            if (tetris_create(&b, N, P, H, 10, map, 0, nullptr)) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
            Aligned rec = words(s, (size_t)T * N * P * 12), ring_obs = words(s, (size_t)cap * P * 12);
            tetris_traj_obs obs = {T, 0, (uint32_t*)rec.get()};
            std::vector<uint8_t> action(cap * 4), done(cap), flags(cap);
            std::vector<float> fl(cap), prio(max_size);
            std::vector<int32_t> cursor(4);
            for (int i = 0; i < cap; i++) flags[i] = (uint8_t)(lcg(s) & 1u);
            tetris_replay rp = {cap, k_step, (uint32_t*)ring_obs.get(), action.data(), fl.data(), fl.data(), fl.data(), fl.data(), done.data(),
                                flags.data(), prio.data(), cursor.data()};
            for (int M : {1, 15, 17, 33, 257})
                for (int n_items = 0; n_items <= 4; n_items++, n_case++) {
                    const int pad = n_case % 3 != 0, f16 = n_case % 2, last = (n_case / 2) % 2, form = n_case % 4;      // 0, 1: index list
                    const int steps = form == 3 ? 2 : form == 2 ? k_step + 1 : 1, m = form == 1 ? N : M, samples = m * steps;
                    const int C = 1 + n_items, Hp = H + (pad ? 2 : 0), Wp = pad ? 12 : 10, esize = f16 ? 2 : 4;
                    std::vector<int32_t> index(m);
                    const uint32_t total = form >= 2 ? (uint32_t)max_size : (uint32_t)(T * N);
                    for (int j = 0; j < m; j++) index[j] = (int32_t)((lcg(s) % total) | ((lcg(s) & 1u) && form < 2 ? 0x80000000u : 0u));
                    index[m - 1] = -1;
                    if (m > 2) { index[m - 2] = (int32_t)total; index[m - 3] = (int32_t)(total - 1); }
                    // exactly the documented sizes, on the heap, one element past a 16-byte boundary for odd cases
                    const size_t lead = (n_case / 4) % 2 ? (size_t)esize : 0;
                    Aligned visual = aligned(lead + (size_t)P * samples * C * Hp * Wp * esize), vector = aligned(lead + (size_t)P * samples * 12 * esize);
                    std::vector<uint8_t> piece((size_t)P * samples), valid(samples);
                    tetris_net_input in;
                    memset(&in, 0, sizeof in);
                    if (form >= 2) { in.replay = &rp; in.d_index = index.data(); in.steps = form == 2 ? steps : 0; in.step_mask = form == 3 ? 0xAu : 0u; }
                    else { in.obs = &obs; in.d_index = form == 0 ? index.data() : nullptr; in.row = 1; }
                    in.M = m; in.n_items = n_items;
                    const int order[4] = {TETRIS_INPUT_HOLES, TETRIS_INPUT_CUMSUM, TETRIS_INPUT_HEIGHT, TETRIS_INPUT_SHADOW};
                    for (int i = 0; i < n_items; i++) in.items[i] = order[(i + n_case) % 4];
                    in.flags = (f16 ? TETRIS_INPUT_F16 : 0) | (last ? TETRIS_INPUT_CHANNELS_LAST : 0) | (pad ? TETRIS_INPUT_PAD : 0);
                    in.d_visual = visual.get() + lead; in.d_vector = vector.get() + lead; in.d_piece = piece.data(); in.d_valid = valid.data();
                    // (the buffers above are rounded up to 16 bytes by aligned(): the exact ends are checked on copies below)
                    std::vector<uint8_t> vis_exact((size_t)P * samples * C * Hp * Wp * esize), vec_exact((size_t)P * samples * 12 * esize);
                    OK(tetris_net_input_dev(b, &in));
                    if ((uintptr_t)vis_exact.data() % esize == 0 && (uintptr_t)vec_exact.data() % esize == 0) {
                        in.d_visual = vis_exact.data(); in.d_vector = vec_exact.data();
                        OK(tetris_net_input_dev(b, &in));
                        if (memcmp(vis_exact.data(), visual.get() + lead, vis_exact.size()) || memcmp(vec_exact.data(), vector.get() + lead, vec_exact.size())) {
                            fprintf(stderr, "two calls differ\n");
                            return 1;
                        }
                    }
                    if (form != 0 || M != 17 || n_items != 4) continue;
                    // ---- the argument rules (input_args), where this case is an index list
                    tetris_net_input bad = in;
                    tetris_traj_obs bad_obs = obs;
                    REFUSED(tetris_net_input_dev(b, nullptr));
                    REFUSED(tetris_net_input_dev(nullptr, &in));
                    bad.replay = &rp; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad.obs = nullptr; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad_obs.d_obs = nullptr; bad.obs = &bad_obs; REFUSED(tetris_net_input_dev(b, &bad));
                    bad_obs.d_obs = obs.d_obs + 1; REFUSED(tetris_net_input_dev(b, &bad));
                    bad_obs = obs; bad_obs.capacity = 0; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad.d_index = nullptr; bad.row = T; bad.M = N; REFUSED(tetris_net_input_dev(b, &bad));
                    bad.row = -1; REFUSED(tetris_net_input_dev(b, &bad));
                    bad.row = 0; bad.M = N - 1; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad.M = -1; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad.n_items = 5; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad.items[2] = 0; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad.items[3] = bad.items[0]; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad.flags |= 8; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad.d_visual = (uint8_t*)in.d_visual + 1; REFUSED(tetris_net_input_dev(b, &bad)); bad = in;
                    bad.obs = nullptr; bad.replay = &rp; bad.steps = 0; REFUSED(tetris_net_input_dev(b, &bad));
                    bad.steps = k_step + 2; REFUSED(tetris_net_input_dev(b, &bad));
                    bad.step_mask = 1ull << (k_step + 1); REFUSED(tetris_net_input_dev(b, &bad));
                    bad.step_mask = 0; bad.steps = 1; bad.d_index = nullptr; REFUSED(tetris_net_input_dev(b, &bad));
                }
            tetris_destroy(b);
        }
    // three players: refused
    tetris_batch* b3 = nullptr;
    if (tetris_create(&b3, 4, 3, 8, 10, map, 0, nullptr)) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
    Aligned rec = words(s, 4 * 3 * 12);
    tetris_traj_obs obs = {1, 0, (uint32_t*)rec.get()};
    tetris_net_input in;
    memset(&in, 0, sizeof in);
    in.obs = &obs; in.M = 4;
    REFUSED(tetris_net_input_dev(b3, &in));
    tetris_destroy(b3);
    return 0;
}

int main() {
    const int rc = run();
    printf(rc ? "FAILED\n" : "net_input: ran clean\n");
    return rc;
}
