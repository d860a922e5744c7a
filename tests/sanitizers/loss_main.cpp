// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there,
// NAME = loss): tetris_ppo_loss_dev and tetris_dqn_loss_dev on 1, 64, 65 and 257 samples, K = 7 and 1, V = 1 and K, float32 and
// binary16 in and out, with and without a valid mask, weights and the optional outputs, with buffers of exactly the documented
// sizes on the heap so that a read or write past an end is reported; out-of-range action bytes; then one refused call per
// argument rule.
#include "standalone.h"

#include <memory>

typedef std::unique_ptr<uint8_t[], void (*)(void*)> Aligned;
static Aligned aligned(size_t bytes) { return Aligned((uint8_t*)aligned_alloc(16, (bytes + 15) / 16 * 16), free); }

// `count` elements of the element type from float32 values
static Aligned elements(const std::vector<float>& v, bool f16) {
    Aligned mem = aligned(v.size() * (f16 ? 2 : 4));
    if (f16) for (size_t k = 0; k < v.size(); k++) ((uint16_t*)mem.get())[k] = plan_f32_to_f16(v[k]);
    else memcpy(mem.get(), v.data(), v.size() * 4);
    return mem;
}

static int run(tetris_batch* b, int M, int K, int V, bool f16, bool g16, bool masked) {
    uint32_t s = 11u + (uint32_t)(M * 1000 + K * 100 + V * 10 + f16 * 2 + g16);
    const size_t n = (size_t)M * 40 * K;
    std::vector<float> pi32(n), v32((size_t)M * V), q32(n), old(M), adv(M), target(M), weight(M), terms(6 * (size_t)M), prio(M), q(M), stats(TETRIS_LOSS_STATS);
    for (auto& x : pi32) x = (float)(lcg(s) % 1000) / 40000.0f;
    for (auto& x : q32) x = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
    for (auto& x : v32) x = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
    for (int m = 0; m < M; m++) {
        old[m] = m % 5 == 0 ? 0.0f : (float)(1 + lcg(s) % 1000) / 20000.0f;
        adv[m] = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
        target[m] = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
        weight[m] = m % 4 == 1 ? 0.0f : (float)(lcg(s) % 1000) / 1000.0f;
    }
    std::vector<uint8_t> action(3 * (size_t)M), valid(M);
    for (auto& a : action) a = (uint8_t)(lcg(s) % 12);                 // r, t and piece past their ranges among them
    for (int m = 0; m < M; m++) valid[m] = (uint8_t)(m % 7 != 3);
    Aligned pi = elements(pi32, f16), Q = elements(q32, f16), v = elements(v32, f16);
    Aligned grad = aligned(n * (g16 ? 2 : 4));
    std::vector<uint8_t> grad_v((size_t)M * V * (g16 ? 2 : 4));
    const int flags = (f16 ? TETRIS_LOSS_F16 | TETRIS_LOSS_VALUE_F16 : 0) | (g16 ? TETRIS_LOSS_GRAD_F16 : 0);
    tetris_ppo_loss p;
    memset(&p, 0, sizeof p);
    p.d_pi = pi.get(); p.d_v = v.get(); p.d_action = action.data(); p.d_prob_old = old.data(); p.d_adv = adv.data(); p.d_target = target.data();
    p.d_valid = masked ? valid.data() : nullptr;
    p.M = M; p.n_pieces = K; p.n_values = V; p.flags = flags;
    p.clip = 0.15f; p.value_loss = 0.3f; p.policy_loss = 1.0f; p.entropy_loss = 0.01f; p.entropy_floor_loss = 1.0f; p.rescaled_entropy = 0.5f;
    p.entropy_floor = 3.62f; p.max_entropy = 3.6888795f; p.grad_scale = 128.0f;
    p.d_grad_pi = grad.get(); p.d_grad_v = grad_v.data(); p.d_terms = masked ? terms.data() : nullptr; p.d_stats = stats.data();
    int rc = tetris_ppo_loss_dev(b, &p);
    tetris_dqn_loss d;
    memset(&d, 0, sizeof d);
    d.d_Q = Q.get(); d.d_action = action.data(); d.d_target = target.data(); d.d_weight = masked ? weight.data() : nullptr;
    d.d_valid = masked ? valid.data() : nullptr;
    d.M = M; d.n_pieces = K; d.flags = flags & ~TETRIS_LOSS_VALUE_F16; d.optimistic_prios = 0.25f; d.grad_scale = 128.0f;
    d.d_grad_Q = grad.get(); d.d_new_prio = prio.data(); d.d_q = masked ? q.data() : nullptr; d.d_stats = stats.data();
    if (!rc) rc = tetris_dqn_loss_dev(b, &d);
    if (rc) { fprintf(stderr, "M=%d K=%d V=%d f16=%d g16=%d: rc %d: %s\n", M, K, V, (int)f16, (int)g16, rc, tetris_last_error()); return rc; }
    if (M != 65 || K != 7 || f16) return 0;
    tetris_ppo_loss bp = p;                                            // ppo_loss_args, loss_common_check
    REFUSED(tetris_ppo_loss_dev(b, nullptr));
    bp.n_pieces = 3; REFUSED(tetris_ppo_loss_dev(b, &bp)); bp = p;
    bp.n_values = 2; REFUSED(tetris_ppo_loss_dev(b, &bp)); bp = p;
    bp.d_adv = nullptr; REFUSED(tetris_ppo_loss_dev(b, &bp)); bp = p;
    bp.d_stats = nullptr; REFUSED(tetris_ppo_loss_dev(b, &bp)); bp = p;
    bp.M = -1; REFUSED(tetris_ppo_loss_dev(b, &bp)); bp = p;
    bp.clip = -1.0f; REFUSED(tetris_ppo_loss_dev(b, &bp)); bp = p;
    bp.flags = 8; REFUSED(tetris_ppo_loss_dev(b, &bp)); bp = p;
    bp.d_pi = pi.get() + 4; REFUSED(tetris_ppo_loss_dev(b, &bp));
    tetris_dqn_loss bd = d;                                            // dqn_loss_args
    REFUSED(tetris_dqn_loss_dev(b, nullptr));
    bd.n_pieces = 0; REFUSED(tetris_dqn_loss_dev(b, &bd)); bd = d;
    bd.d_new_prio = nullptr; REFUSED(tetris_dqn_loss_dev(b, &bd)); bd = d;
    bd.flags = TETRIS_LOSS_VALUE_F16; REFUSED(tetris_dqn_loss_dev(b, &bd)); bd = d;
    REFUSED(tetris_dqn_loss_dev(nullptr, &d));                         // check_batch
    bd.M = 0;                                                          // no samples: the statistics are zeroed, nothing else is touched
    if (tetris_dqn_loss_dev(b, &bd) != TETRIS_OK || stats[0] != 0.0f) { fprintf(stderr, "M = 0\n"); return 1; }
    return 0;
}

int main() {
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    tetris_batch* b = nullptr;
    if (tetris_create(&b, 4, 1, 20, 10, map, 0, nullptr)) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
    int rc = 0;
    for (int M : {1, 64, 65, 257})
        for (int K : {7, 1})
            for (int V : {1, K})
                for (int types = 0; types < 4; types++)
                    for (int masked = 0; masked < 2; masked++) rc |= run(b, M, K, V, (types & 1) != 0, (types & 2) != 0, masked != 0);
    tetris_destroy(b);
    printf(rc ? "FAILED\n" : "loss: ran clean\n");
    return rc ? 1 : 0;
}
