// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there,
// NAME = res): the serial forms of tetris_res_layer_dev, tetris_res_layer_grad_x_dev and tetris_res_layer_grad_w_dev on M = 1 and 17
// samples — float32 and binary16, every join, with and without ELU, Ci < Co (8, 32) and Ci > Co (40, 32), Hp = 5, and at M = 1 the
// default shape (Hp = 22, 128 channels) — with buffers of exactly the documented sizes on the heap, so that a read or write past an
// end is reported; then one refused call per argument rule.
#include "standalone.h"

#include <memory>

typedef std::unique_ptr<uint8_t[], void (*)(void*)> Aligned;
static Aligned aligned(size_t bytes) { return Aligned((uint8_t*)aligned_alloc(16, (bytes + 15) / 16 * 16), free); }

// `count` elements of the element type: values in [-1, 1]; the sanitizer's red zone begins within 15 bytes of the last one
static Aligned elements(uint32_t& s, size_t count, bool f16) {
    Aligned mem = aligned(count * (f16 ? 2 : 4));
    for (size_t i = 0; i < count; i++) {
        const float v = (float)(lcg(s) % 2001) / 1000.0f - 1.0f;
        if (f16) ((uint16_t*)mem.get())[i] = plan_f32_to_f16(v);
        else ((float*)mem.get())[i] = v;
    }
    return mem;
}

static int run() {
    const uint8_t map[7] = {0, 1, 2, 3, 4, 5, 6};
    tetris_batch* b = nullptr;
    if (tetris_create(&b, 4, 1, 8, 10, map, 0, nullptr)) { fprintf(stderr, "create: %s\n", tetris_last_error()); return 1; }
    uint32_t s = 93u;
    for (int M : {1, 17})
        for (int f16 = 0; f16 < 2; f16++)
            for (int join : {TETRIS_RES_JOIN_NONE, TETRIS_RES_JOIN_ADD, TETRIS_RES_JOIN_TRUNCATE_ADD})
                for (int shape = 0; shape < (M == 1 ? 3 : 2); shape++) {
                    const int Hp = shape == 2 ? 22 : 5, Ci = shape == 0 ? 8 : shape == 1 ? 40 : 128, Co = shape == 2 ? 128 : 32;
                    const int act = (shape + join + f16) % 2 ? TETRIS_RES_ACT_ELU : TETRIS_RES_ACT_NONE;
                    const int Cout = join == TETRIS_RES_JOIN_NONE ? Co : join == TETRIS_RES_JOIN_ADD ? (Ci > Co ? Ci : Co) : (Ci < Co ? Ci : Co);
                    const size_t es = f16 ? 2 : 4, pos = (size_t)M * Hp * 12, nx = pos * Ci, nw = (size_t)9 * Ci * Co, no = pos * Cout;
                    Aligned x = elements(s, nx, f16), w = elements(s, nw, f16), bias = elements(s, Co, false), g = elements(s, no, f16);
                    Aligned out = aligned(no * es), gx = aligned(nx * es), gw = aligned(nw * 4), gb = aligned((size_t)Co * 4);
                    tetris_res_layer k;
                    memset(&k, 0, sizeof k);
                    k.d_x = x.get(); k.d_w = w.get(); k.d_bias = (const float*)bias.get(); k.d_grad_out = g.get(); k.d_y = out.get();
                    k.M = M; k.height = Hp; k.in_channels = Ci; k.out_channels = Co; k.join = join; k.activation = act;
                    k.flags = f16 ? TETRIS_RES_F16 : 0;
                    k.d_out = out.get(); k.d_grad_x = gx.get(); k.d_grad_w = (float*)gw.get(); k.d_grad_b = (float*)gb.get();
                    OK(tetris_res_layer_dev(b, &k));
                    OK(tetris_res_layer_grad_x_dev(b, &k));
                    OK(tetris_res_layer_grad_w_dev(b, &k));
                    if (M != 17 || shape != 0 || join != TETRIS_RES_JOIN_ADD || f16) continue;
                    // ---- the argument rules (res_args), once
                    tetris_res_layer bad = k;
                    bad.activation = TETRIS_RES_ACT_ELU;
                    const tetris_res_layer elu = bad;
                    REFUSED(tetris_res_layer_dev(b, nullptr));
                    REFUSED(tetris_res_layer_grad_x_dev(b, nullptr));
                    REFUSED(tetris_res_layer_grad_w_dev(b, nullptr));
                    REFUSED(tetris_res_layer_dev(nullptr, &k));
                    bad.M = 0; REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.height = 3; REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.height = 34; REFUSED(tetris_res_layer_grad_w_dev(b, &bad)); bad = k;
                    bad.in_channels = 12; REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.in_channels = 520; REFUSED(tetris_res_layer_grad_x_dev(b, &bad)); bad = k;
                    bad.out_channels = 48; REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.out_channels = 544; REFUSED(tetris_res_layer_grad_w_dev(b, &bad)); bad = k;
                    bad.join = 3; REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.activation = 2; REFUSED(tetris_res_layer_grad_x_dev(b, &bad)); bad = k;
                    bad.flags = 2; REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.d_x = nullptr; REFUSED(tetris_res_layer_dev(b, &bad)); REFUSED(tetris_res_layer_grad_w_dev(b, &bad)); bad = k;
                    bad.d_w = nullptr; REFUSED(tetris_res_layer_dev(b, &bad)); REFUSED(tetris_res_layer_grad_x_dev(b, &bad)); bad = k;
                    bad.d_bias = nullptr; REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.d_out = nullptr; REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.d_grad_out = nullptr; REFUSED(tetris_res_layer_grad_x_dev(b, &bad)); REFUSED(tetris_res_layer_grad_w_dev(b, &bad)); bad = k;
                    bad = elu; bad.d_y = nullptr; REFUSED(tetris_res_layer_grad_x_dev(b, &bad)); REFUSED(tetris_res_layer_grad_w_dev(b, &bad)); bad = k;
                    bad.d_grad_x = nullptr; REFUSED(tetris_res_layer_grad_x_dev(b, &bad)); bad = k;
                    bad.d_grad_w = nullptr; REFUSED(tetris_res_layer_grad_w_dev(b, &bad)); bad = k;
                    bad.d_grad_b = nullptr; REFUSED(tetris_res_layer_grad_w_dev(b, &bad)); bad = k;
                    bad.d_x = x.get() + 4; REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.d_w = w.get() + 8; REFUSED(tetris_res_layer_grad_x_dev(b, &bad)); bad = k;
                    bad.d_grad_w = (float*)(gw.get() + 4); REFUSED(tetris_res_layer_grad_w_dev(b, &bad)); bad = k;
                    bad.d_out = x.get(); REFUSED(tetris_res_layer_dev(b, &bad)); bad = k;
                    bad.d_grad_x = w.get(); REFUSED(tetris_res_layer_grad_x_dev(b, &bad)); bad = k;
                    bad.d_grad_b = (float*)(x.get() + 64); REFUSED(tetris_res_layer_grad_w_dev(b, &bad));
                }
    tetris_destroy(b);
    return 0;
}

int main() {
    const int rc = run();
    printf(rc ? "FAILED\n" : "res: ran clean\n");
    return rc;
}
