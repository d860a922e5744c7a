// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there,
// NAME = head): the serial forms of tetris_q_head_dev, tetris_q_head_grad_dev, tetris_policy_head_dev and
// tetris_policy_head_grad_dev on M = 1, 17 and 65 samples — K = 7 and 1, every mode with separate piece values on and off, the
// piece mask {0, 2, 5}, v absent, [M][1] and [M][K], w [M][1] and [M][K + 1], float32 and binary16, with and without A — with
// buffers of exactly the documented sizes on the heap, so that a read or write past an end is reported; then one refused call per
// argument rule.
#include "standalone.h"

#include <memory>

typedef std::unique_ptr<uint8_t[], void (*)(void*)> Aligned;
static Aligned aligned(size_t bytes) { return Aligned((uint8_t*)aligned_alloc(16, (bytes + 15) / 16 * 16), free); }

// `count` elements of the element type: values in [-3, 3]; the sanitizer's red zone begins within 15 bytes of the last one
static Aligned elements(uint32_t& s, size_t count, bool f16) {
    Aligned mem = aligned(count * (f16 ? 2 : 4));
    for (size_t i = 0; i < count; i++) {
        const float v = (float)(lcg(s) % 6001) / 1000.0f - 3.0f;
        if (f16) ((uint16_t*)mem.get())[i] = plan_f32_to_f16(v);
        else ((float*)mem.get())[i] = v;
    }
    return mem;
}

static int run() {
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    tetris_batch* b = nullptr;
    if (tetris_create(&b, 4, 1, 8, 10, map, 0, nullptr)) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
    uint32_t s = 77u;
    for (int M : {1, 17, 65})
        for (int K : {7, 1})
            for (int f16 = 0; f16 < 2; f16++) {
                const size_t big = (size_t)M * 40 * K;
                const int flags = f16 ? TETRIS_HEAD_F16 | TETRIS_HEAD_VALUE_F16 : 0;
                for (int Kv : {0, 1, K})
                    for (int mode : {TETRIS_HEAD_MEAN, TETRIS_HEAD_MAX, TETRIS_HEAD_NONE})
                        for (int sep = 0; sep < 2; sep++) {
                            Aligned a = elements(s, big, f16), G = elements(s, big, f16), v = elements(s, (size_t)M * (Kv ? Kv : 1), f16);
                            Aligned Q = aligned(big * (f16 ? 2 : 4)), A = aligned(big * (f16 ? 2 : 4)), ga = aligned(big * (f16 ? 2 : 4));
                            Aligned gv = aligned((size_t)M * (Kv ? Kv : 1) * (f16 ? 2 : 4));
                            std::vector<float> V(M);
                            tetris_q_head q;
                            memset(&q, 0, sizeof q);
                            q.d_a = a.get(); q.d_v = Kv ? v.get() : nullptr; q.d_grad_Q = G.get();
                            q.M = M; q.n_pieces = K; q.n_values = Kv; q.mode = mode; q.separate_piece_values = sep;
                            q.used_pieces = K == 7 ? 0x25 : 1; q.flags = flags; q.advantage_range = 0.5f;
                            q.d_Q = Q.get(); q.d_V = V.data(); q.d_A = sep ? A.get() : nullptr; q.d_grad_a = ga.get(); q.d_grad_v = Kv ? gv.get() : nullptr;
                            OK(tetris_q_head_dev(b, &q));
                            OK(tetris_q_head_grad_dev(b, &q));
                            if (M != 17 || K != 7 || Kv != 7 || mode != TETRIS_HEAD_MAX || !sep || f16) continue;
                            // ---- the argument rules (q_head_args), once
                            tetris_q_head bad = q;
                            REFUSED(tetris_q_head_dev(b, nullptr));
                            REFUSED(tetris_q_head_grad_dev(b, nullptr));
                            REFUSED(tetris_q_head_dev(nullptr, &q));
                            bad.M = 0; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.n_pieces = 3; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.n_values = 2; REFUSED(tetris_q_head_grad_dev(b, &bad)); bad = q;
                            bad.mode = 3; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.used_pieces = 0; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.used_pieces = 0x80; REFUSED(tetris_q_head_grad_dev(b, &bad)); bad = q;
                            bad.flags = 4; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.d_a = nullptr; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.d_Q = nullptr; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.d_V = nullptr; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.d_grad_Q = nullptr; REFUSED(tetris_q_head_grad_dev(b, &bad)); bad = q;
                            bad.d_grad_a = nullptr; REFUSED(tetris_q_head_grad_dev(b, &bad)); bad = q;
                            bad.d_grad_v = nullptr; REFUSED(tetris_q_head_grad_dev(b, &bad)); bad = q;
                            bad.d_a = a.get() + 4; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.d_A = A.get() + 8; REFUSED(tetris_q_head_dev(b, &bad)); bad = q;
                            bad.d_grad_a = ga.get() + 4; REFUSED(tetris_q_head_grad_dev(b, &bad));
                        }
                for (int W : {1, K + 1}) {
                    const size_t nv = (size_t)M * (W == 1 ? 1 : K), nw = (size_t)M * W;
                    Aligned x = elements(s, big, f16), w = elements(s, nw, f16), g = elements(s, big, f16), gv = elements(s, nv, f16);
                    Aligned pi = aligned(big * (f16 ? 2 : 4)), pv = aligned(nv * (f16 ? 2 : 4)), gx = aligned(big * (f16 ? 2 : 4)), gw = aligned(nw * (f16 ? 2 : 4));
                    tetris_policy_head p;
                    memset(&p, 0, sizeof p);
                    p.d_x = x.get(); p.d_w = w.get(); p.d_grad_pi = g.get(); p.d_grad_v = gv.get();
                    p.M = M; p.n_pieces = K; p.n_values = W; p.flags = flags;
                    p.d_pi = pi.get(); p.d_v = pv.get(); p.d_grad_x = gx.get(); p.d_grad_w = gw.get();
                    OK(tetris_policy_head_dev(b, &p));
                    OK(tetris_policy_head_grad_dev(b, &p));
                    if (M != 17 || K != 7 || W != 8 || f16) continue;
                    tetris_policy_head bad = p;                              // policy_head_args
                    REFUSED(tetris_policy_head_dev(b, nullptr));
                    REFUSED(tetris_policy_head_grad_dev(b, nullptr));
                    bad.M = -1; REFUSED(tetris_policy_head_dev(b, &bad)); bad = p;
                    bad.n_pieces = 2; REFUSED(tetris_policy_head_dev(b, &bad)); bad = p;
                    bad.n_values = 7; REFUSED(tetris_policy_head_grad_dev(b, &bad)); bad = p;
                    bad.flags = 8; REFUSED(tetris_policy_head_dev(b, &bad)); bad = p;
                    bad.d_x = nullptr; REFUSED(tetris_policy_head_dev(b, &bad)); bad = p;
                    bad.d_w = nullptr; REFUSED(tetris_policy_head_dev(b, &bad)); bad = p;
                    bad.d_pi = nullptr; REFUSED(tetris_policy_head_grad_dev(b, &bad)); bad = p;
                    bad.d_v = nullptr; REFUSED(tetris_policy_head_dev(b, &bad)); bad = p;
                    bad.d_grad_pi = nullptr; REFUSED(tetris_policy_head_grad_dev(b, &bad)); bad = p;
                    bad.d_grad_v = nullptr; REFUSED(tetris_policy_head_grad_dev(b, &bad)); bad = p;
                    bad.d_grad_x = nullptr; REFUSED(tetris_policy_head_grad_dev(b, &bad)); bad = p;
                    bad.d_grad_w = nullptr; REFUSED(tetris_policy_head_grad_dev(b, &bad)); bad = p;
                    bad.d_pi = pi.get() + 4; REFUSED(tetris_policy_head_dev(b, &bad)); bad = p;
                    bad.d_grad_x = gx.get() + 8; REFUSED(tetris_policy_head_grad_dev(b, &bad));
                }
            }
    tetris_destroy(b);
    return 0;
}

int main() {
    const int rc = run();
    printf(rc ? "FAILED\n" : "head: ran clean\n");
    return rc;
}
