// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
//
// A stand-alone program over the CPU harness for AddressSanitizer and UBSan (standalone.h; built and run by the line given there,
// NAME = kbd): the serial forms of tetris_kbd_conv_dev, tetris_kbd_conv_grad_x_dev and tetris_kbd_conv_grad_w_dev on M = 1, 17 and
// 65 samples — K = 7 and 1, float32 and binary16, a small image (Hp = 5, C = 32) and, at M = 1, the default one (Hp = 22,
// C = 128) — with buffers of exactly the documented sizes on the heap, so that a read or write past an end is reported; then one
// refused call per argument rule.
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
    uint32_t s = 91u;
    for (int M : {1, 17, 65})
        for (int K : {7, 1})
            for (int f16 = 0; f16 < 2; f16++)
                for (int full = 0; full < (M == 1 ? 2 : 1); full++) {
                    const int Hp = full ? 22 : 5, C = full ? 128 : 32, O = 4 * K;
                    const size_t es = f16 ? 2 : 4, nx = (size_t)M * Hp * 12 * C, nw = (size_t)Hp * 3 * C * O, no = (size_t)M * 40 * K;
                    Aligned x = elements(s, nx, f16), w = elements(s, nw, f16), bias = elements(s, O, false), g = elements(s, no, f16);
                    Aligned out = aligned(no * es), gx = aligned(nx * es), gw = aligned(nw * 4), gb = aligned((size_t)O * 4);
                    tetris_kbd_conv k;
                    memset(&k, 0, sizeof k);
                    k.d_x = x.get(); k.d_w = w.get(); k.d_bias = (const float*)bias.get(); k.d_grad_out = g.get();
                    k.M = M; k.n_pieces = K; k.height = Hp; k.channels = C; k.flags = f16 ? TETRIS_KBD_F16 : 0;
                    k.d_out = out.get(); k.d_grad_x = gx.get(); k.d_grad_w = (float*)gw.get(); k.d_grad_b = (float*)gb.get();
                    OK(tetris_kbd_conv_dev(b, &k));
                    OK(tetris_kbd_conv_grad_x_dev(b, &k));
                    OK(tetris_kbd_conv_grad_w_dev(b, &k));
                    if (M != 17 || K != 7 || f16) continue;
                    // ---- the argument rules (kbd_args), once
                    tetris_kbd_conv bad = k;
                    REFUSED(tetris_kbd_conv_dev(b, nullptr));
                    REFUSED(tetris_kbd_conv_grad_x_dev(b, nullptr));
                    REFUSED(tetris_kbd_conv_grad_w_dev(b, nullptr));
                    REFUSED(tetris_kbd_conv_dev(nullptr, &k));
                    bad.M = 0; REFUSED(tetris_kbd_conv_dev(b, &bad)); bad = k;
                    bad.n_pieces = 0; REFUSED(tetris_kbd_conv_dev(b, &bad)); bad = k;
                    bad.n_pieces = 8; REFUSED(tetris_kbd_conv_grad_x_dev(b, &bad)); bad = k;
                    bad.height = 3; REFUSED(tetris_kbd_conv_dev(b, &bad)); bad = k;
                    bad.height = 34; REFUSED(tetris_kbd_conv_grad_w_dev(b, &bad)); bad = k;
                    bad.channels = 48; REFUSED(tetris_kbd_conv_dev(b, &bad)); bad = k;
                    bad.channels = 544; REFUSED(tetris_kbd_conv_grad_x_dev(b, &bad)); bad = k;
                    bad.flags = 2; REFUSED(tetris_kbd_conv_dev(b, &bad)); bad = k;
                    bad.d_x = nullptr; REFUSED(tetris_kbd_conv_dev(b, &bad)); REFUSED(tetris_kbd_conv_grad_w_dev(b, &bad)); bad = k;
                    bad.d_w = nullptr; REFUSED(tetris_kbd_conv_dev(b, &bad)); REFUSED(tetris_kbd_conv_grad_x_dev(b, &bad)); bad = k;
                    bad.d_bias = nullptr; REFUSED(tetris_kbd_conv_dev(b, &bad)); bad = k;
                    bad.d_out = nullptr; REFUSED(tetris_kbd_conv_dev(b, &bad)); bad = k;
                    bad.d_grad_out = nullptr; REFUSED(tetris_kbd_conv_grad_x_dev(b, &bad)); REFUSED(tetris_kbd_conv_grad_w_dev(b, &bad)); bad = k;
                    bad.d_grad_x = nullptr; REFUSED(tetris_kbd_conv_grad_x_dev(b, &bad)); bad = k;
                    bad.d_grad_w = nullptr; REFUSED(tetris_kbd_conv_grad_w_dev(b, &bad)); bad = k;
                    bad.d_grad_b = nullptr; REFUSED(tetris_kbd_conv_grad_w_dev(b, &bad)); bad = k;
                    bad.d_x = x.get() + 4; REFUSED(tetris_kbd_conv_dev(b, &bad)); bad = k;
                    bad.d_w = w.get() + 8; REFUSED(tetris_kbd_conv_grad_x_dev(b, &bad)); bad = k;
                    bad.d_grad_w = (float*)(gw.get() + 4); REFUSED(tetris_kbd_conv_grad_w_dev(b, &bad)); bad = k;
                    bad.d_out = x.get(); REFUSED(tetris_kbd_conv_dev(b, &bad)); bad = k;
                    bad.d_grad_x = w.get(); REFUSED(tetris_kbd_conv_grad_x_dev(b, &bad)); bad = k;
                    bad.d_grad_b = (float*)(x.get() + 64); REFUSED(tetris_kbd_conv_grad_w_dev(b, &bad));
                }
    tetris_destroy(b);
    return 0;
}

int main() {
    const int rc = run();
    printf(rc ? "FAILED\n" : "kbd: ran clean\n");
    return rc;
}
