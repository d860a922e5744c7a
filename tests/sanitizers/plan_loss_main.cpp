// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there,
// NAME = plan_loss): tetris_plan_loss_dev in its serial form on M = 5 samples — one mirrored index, one that names no entry — and
// on 1, 16, 17 and 33, heights 20 and 7, K = 7 and 1, V = 1 and K, float32 and binary16 in and out, with and without a valid mask
// and the optional output, the pieces as a uint8 [M] array and as byte 2 of an action array [M][3], with buffers of exactly the
// documented sizes on the heap so that a read or write past an end is reported; records of random words (kinds 0, 1 and 2); then
// one refused call per argument rule.
#include "standalone.h"

#include <memory>

// the elements of the element type from float32 values, in a heap block of exactly their size
static std::unique_ptr<uint8_t[]> elements(const std::vector<float>& v, bool f16) {
    std::unique_ptr<uint8_t[]> mem(new uint8_t[v.size() * (f16 ? 2 : 4)]);
    if (f16) for (size_t k = 0; k < v.size(); k++) ((uint16_t*)mem.get())[k] = plan_f32_to_f16(v[k]);
    else memcpy(mem.get(), v.data(), v.size() * 4);
    return mem;
}

static int run(tetris_batch* b, int H, int N, int M, int K, int V, bool f16, bool g16, bool masked, bool stride3) {
    uint32_t s = 7u + (uint32_t)(M * 1000 + K * 100 + V * 10 + f16 * 2 + g16 + H);
    const int T = 2, total = T * N;
    const size_t n = (size_t)M * H * 10 * K;
    // operator new gives 16-byte aligned blocks of exactly the size asked for
    std::unique_ptr<uint32_t[]> rec(new uint32_t[(size_t)total * TETRIS_PLAN_REC_WORDS]);
    for (size_t w = 0; w < (size_t)total * TETRIS_PLAN_REC_WORDS; w++) rec[w] = lcg(s) * 256u + (lcg(s) & 255u);
    for (int at = 0; at < total; at++) {
        rec[(size_t)at * TETRIS_PLAN_REC_WORDS + 20] = lcg(s) % 3;
        rec[(size_t)at * TETRIS_PLAN_REC_WORDS + 21] = (lcg(s) % 300) | ((lcg(s) % 300) << 16);
    }
    tetris_traj_plan plan = {T, 0, rec.get()};
    std::vector<float> phi32(n), v32((size_t)M * V);
    for (auto& x : phi32) x = (float)(lcg(s) % 1300) / 1000.0f - 0.1f;              // below e, inside, above 1
    for (auto& x : v32) x = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
    std::unique_ptr<float[]> old(new float[M]), adv(new float[M]), target(new float[M]), terms(new float[6 * (size_t)M]), stats(new float[TETRIS_LOSS_STATS]);
    std::unique_ptr<int32_t[]> index(new int32_t[M]);
    std::unique_ptr<uint8_t[]> valid(new uint8_t[M]), pieces(new uint8_t[stride3 ? 3 * (size_t)M : (size_t)M]);
    for (int m = 0; m < M; m++) {
        old[m] = m % 5 == 0 ? 0.0f : (float)(1 + lcg(s) % 1000) / 2000.0f;
        adv[m] = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
        target[m] = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
        index[m] = (int32_t)(lcg(s) % (uint32_t)total);
        valid[m] = (uint8_t)(m % 7 != 3);
        pieces[stride3 ? 3 * (size_t)m + 2 : (size_t)m] = (uint8_t)(lcg(s) % 12);  // pieces past K - 1 among them
    }
    index[M / 2] = (int32_t)((uint32_t)index[M / 2] | 0x80000000u);                // the mirrored image
    if (M > 1) index[M - 1] = -1;                                                  // names no entry
    if (M > 2) index[1] = total;
    std::unique_ptr<uint8_t[]> phi = elements(phi32, f16), v = elements(v32, f16);
    std::unique_ptr<uint8_t[]> grad(new uint8_t[n * (g16 ? 2 : 4)]), grad_v(new uint8_t[(size_t)M * V * (g16 ? 2 : 4)]);
    tetris_plan_loss p;
    memset(&p, 0, sizeof p);
    p.d_phi = phi.get(); p.d_v = v.get(); p.d_index = index.get(); p.d_piece = pieces.get() + (stride3 ? 2 : 0); p.piece_stride = stride3 ? 3 : 1;
    p.d_prob_old = old.get(); p.d_adv = adv.get(); p.d_target = target.get(); p.d_valid = masked ? valid.get() : nullptr;
    p.M = M; p.n_pieces = K; p.n_values = V;
    p.flags = (f16 ? TETRIS_LOSS_F16 | TETRIS_LOSS_VALUE_F16 : 0) | (g16 ? TETRIS_LOSS_GRAD_F16 : 0);
    p.small_fill = masked ? 1e-3f : 0.0f;
    p.clip = 0.15f; p.value_loss = 0.3f; p.policy_loss = 1.0f; p.entropy_loss = 0.01f; p.impossibility_loss = 0.1f; p.grad_scale = 128.0f;
    p.d_grad_phi = grad.get(); p.d_grad_v = grad_v.get(); p.d_terms = masked ? terms.get() : nullptr; p.d_stats = stats.get();
    if (((uintptr_t)p.d_phi | (uintptr_t)p.d_grad_phi | (uintptr_t)plan.d_rec) & 15u) { fprintf(stderr, "operator new gave an unaligned block\n"); return 1; }
    const int rc = tetris_plan_loss_dev(b, &plan, &p);
    if (rc) { fprintf(stderr, "H=%d M=%d K=%d V=%d f16=%d g16=%d: rc %d: %s\n", H, M, K, V, (int)f16, (int)g16, rc, tetris_last_error()); return rc; }
    if (M != 5 || K != 7 || f16 || g16 || !masked || H != 20) return 0;
    tetris_plan_loss bp = p;                                           // plan_loss_args
    tetris_traj_plan none = {T, 0, nullptr}, empty = {0, 0, rec.get()}, odd = {T, 0, rec.get() + 1};
    REFUSED(tetris_plan_loss_dev(b, &plan, nullptr));
    REFUSED(tetris_plan_loss_dev(b, nullptr, &p));
    REFUSED(tetris_plan_loss_dev(b, &none, &p));
    REFUSED(tetris_plan_loss_dev(b, &empty, &p));
    REFUSED(tetris_plan_loss_dev(b, &odd, &p));
    REFUSED(tetris_plan_loss_dev(nullptr, &plan, &p));                 // check_batch
    bp.n_pieces = 3; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.n_values = 2; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.d_index = nullptr; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.d_piece = nullptr; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.d_stats = nullptr; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.M = -1; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.clip = -1.0f; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.flags = 8; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.piece_stride = 0; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.d_phi = phi.get() + 4; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.d_grad_phi = grad.get() + 8; REFUSED(tetris_plan_loss_dev(b, &plan, &bp)); bp = p;
    bp.M = 0;                                                          // no samples: the statistics are zeroed, nothing else is touched
    if (tetris_plan_loss_dev(b, &plan, &bp) != TETRIS_OK || stats[0] != 0.0f) { fprintf(stderr, "M = 0\n"); return 1; }
    return 0;
}

int main() {
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    int rc = 0;
    for (int H : {20, 7}) {
        tetris_batch* b = nullptr;
        const int N = 4;
        if (tetris_create(&b, N, H == 20 ? 2 : 1, H, 10, map, 0, nullptr)) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
        for (int M : {5, 1, 16, 17, 33})
            for (int K : {7, 1})
                for (int V : {1, K})
                    for (int types = 0; types < 4; types++)
                        for (int masked = 0; masked < 2; masked++)
                            rc |= run(b, H, N, M, K, V, (types & 1) != 0, (types & 2) != 0, masked != 0, (M + types) % 2 == 1);
        tetris_destroy(b);
    }
    {   // three players and a split batch: the window's own rules
        tetris_batch* b = nullptr;
        uint32_t* rec = (uint32_t*)aligned_alloc(16, 448);
        memset(rec, 0, 448);
        tetris_traj_plan plan = {1, 0, rec};
        tetris_plan_loss p;
        memset(&p, 0, sizeof p);
        if (tetris_create(&b, 1, 3, 20, 10, map, 0, nullptr)) return 1;
        if (tetris_plan_loss_dev(b, &plan, &p) != TETRIS_E_ARG) { fprintf(stderr, "three players: not refused\n"); rc = 1; }
        tetris_destroy(b);
        if (tetris_create_split(&b, 1, 0, 20, 10, map, 0, nullptr)) return 1;
        if (tetris_plan_loss_dev(b, &plan, &p) != TETRIS_E_ARG) { fprintf(stderr, "a split batch: not refused\n"); rc = 1; }
        tetris_destroy(b);
        free(rec);
    }
    printf(rc ? "FAILED\n" : "plan_loss: ran clean\n");
    return rc ? 1 : 0;
}
