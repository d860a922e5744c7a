// Kernel bodies of the network's input side (include/tetris_hip.h: tetris_net_input_dev): the fixed arithmetic between a packed
// observation record and a network's first learned layer — the cast to float, apply_visual_pad (agents/networks/network_utils.py:
// 71-77) and visual_stack (network_utils.py:79-93), as resblock / resblock_kbd (agents/networks/builders/sventon_architectures.py:
// 25-29) and the legacy encoder (legacy_build_blocks.py:31) apply them — without the uint8 planes in between.
//
// `__host__ __device__` like tetris_head.h: tetris_hip.hip wraps these in a gfx950 kernel (k_net_input: tetris_dev_input.h), the
// CPU harness (tests/cpu_harness) runs them through input_run_serial (tetris_host.h) in plain host loops.  Integers throughout:
// every value is in [0, 33] and exact in float32 and binary16, so host and device give the same bits.
//
// THE SAMPLE.  Sample j of a call names an entry of a window or of the replay ring, mirrored or not, or no entry: input_entry,
// which is batch_entry / batch_index_entry of tetris_batch.h (the rules of tetris_traj_batch_dev and tetris_replay_gather_dev)
// over the TrajBatchArgs inside InputArgs; the row form (no index list) is entry row N + j.  Slot sl of the entry is a 48-byte
// record (tetris_batch.h): col[c], c = 0..9, is record word c — word 9 - c for a mirrored sample — AND plan_row_mask(H): bits at
// and above H carry no meaning and reach no channel.  No entry: col[c] = 0 and keep = 0, else keep = 1.
//
// THE PADDED COLUMN WORD.  Column x of the image P is the 64-bit word pw[x], bit y = P[y][x] (Hp <= 33 rows):
//   pad:     pw[0] = pw[11] = 2^(H+2) - 1 (the walls: ones in every row, the top pad's row included: the second pad covers it);
//            pw[1 + c] = col[c] << 1 | 2^(H+1) (a zero on top, the column, a one below);  Wp = 12, Hp = H + 2.
//   no pad:  pw[c] = col[c];  Wp = 10, Hp = H.
// No entry: pw[x] = 0 for every x.
//
// THE CHANNELS.  bit = (pw[x] >> y) & 1.  cum = popcount(pw[x] & (2^(y+1) - 1)): tf.cumsum along the rows, top first.
//   code 0 (channel 0)    P       = bit
//   TETRIS_INPUT_CUMSUM   cumsum  = cum
//   TETRIS_INPUT_SHADOW   shadow  = min(cum, 1)
//   TETRIS_INPUT_HEIGHT   height  = y, keep = 0: 0 (a sample that is no sample is zeros in every channel)
//   TETRIS_INPUT_HOLES    holes   = shadow - bit
// Channel ch of the call is code (chan >> 4 ch) & 15: 0, then the caller's items in their order.
//
// THE OUTPUTS.  visual element (sl, j, ch, y, x) is at ((sl M + j) C + ch) Hp Wp + y Wp + x, channels-last at
// ((sl M + j) Hp Wp + y Wp + x) C + ch.  vector element (sl, j, k) is byte k of the three words obs_vector_words gives
// (batch_scalars: the mirrored sample's one-hot quirk kept, zeros for no entry); piece and valid as tetris_traj_batch_dev writes
// them.  An element is float32, or binary16 with f16.  Every element of every output that is given is written, nothing past it.
#pragma once
#include "tetris_batch.h"
#include "tetris_plan.h"

namespace te {

constexpr int INPUT_BLOCK = 8;                   // samples of one slot per workgroup of k_net_input
constexpr int INPUT_THREADS = 256;               // its threads
constexpr int INPUT_MAX_ITEMS = 4;
constexpr int INPUT_MAX_W = NCOL + 2;            // columns of the padded image
constexpr int INPUT_RAW = 0, INPUT_CUMSUM = TETRIS_INPUT_CUMSUM, INPUT_SHADOW = TETRIS_INPUT_SHADOW, INPUT_HEIGHT = TETRIS_INPUT_HEIGHT,
              INPUT_HOLES = TETRIS_INPUT_HOLES;

struct InputArgs {
    TrajBatchArgs ba;            // how a sample finds its record: m, n_slots, H, total, index, obs, steps, limit, flags, step_mask (no output)
    uint32_t row_base;           // the row form (ba.index NULL): sample j is entry row_base + j
    int pad, f16, last;          // TETRIS_INPUT_PAD, _F16, _CHANNELS_LAST
    int C, Hp, Wp, E;            // channels, rows and columns of the image, elements of a sample-slot: C Hp Wp
    uint32_t chan;               // the code of channel ch in bits 4 ch .. 4 ch + 3
    // a flat offset r inside a sample-slot is (a, b, c) = (r / dA, r % dA / dB, r % dB): (ch, y, x), channels-last (y, x, ch)
    uint32_t dA, dB, mE, mA, mB; // the divisors and the reciprocals of E, dA, dB (input_magic)
    void* visual;                // each output: or NULL
    void* vector;
    uint8_t* piece;
    uint8_t* valid;
};

TE_HD int input_blocks(int m) { return (m + INPUT_BLOCK - 1) / INPUT_BLOCK; }

// e / d for e, d < 2^16 by one multiplication: magic = floor(2^32 / d) + 1 is exact while e d < 2^32 (d = 1 has no 32-bit magic)
TE_HD uint32_t input_magic(uint32_t d) { return d > 1u ? 0xFFFFFFFFu / d + 1u : 0u; }
TE_HD uint32_t input_div(uint32_t e, uint32_t d, uint32_t magic) { return d == 1u ? e : (uint32_t)(((uint64_t)e * magic) >> 32); }

struct InputPos { int j, ch, y, x; };
// element e of a run of samples that starts at sample 0
TE_HD InputPos input_pos(const InputArgs& ia, uint32_t e) {
    InputPos p;
    const uint32_t j = input_div(e, (uint32_t)ia.E, ia.mE), r = e - j * (uint32_t)ia.E;
    const uint32_t a = input_div(r, ia.dA, ia.mA), rest = r - a * ia.dA;
    const uint32_t b = input_div(rest, ia.dB, ia.mB), c = rest - b * ia.dB;
    p.j = (int)j;
    if (ia.last) { p.y = (int)a; p.x = (int)b; p.ch = (int)c; }
    else { p.ch = (int)a; p.y = (int)b; p.x = (int)c; }
    return p;
}
// the next element in memory order
template <bool LAST>
TE_HD void input_next(const InputArgs& ia, InputPos& p) {
    if (LAST) {
        if (++p.ch < ia.C) return;
        p.ch = 0;
        if (++p.x < ia.Wp) return;
        p.x = 0;
        if (++p.y < ia.Hp) return;
        p.y = 0; p.j++;
    } else {
        if (++p.x < ia.Wp) return;
        p.x = 0;
        if (++p.y < ia.Hp) return;
        p.y = 0;
        if (++p.ch < ia.C) return;
        p.ch = 0; p.j++;
    }
}

// sample j of the call
TE_HD BatchEntry input_entry(const InputArgs& ia, int j) {
    if (ia.ba.index) return batch_entry(ia.ba, j);
    return batch_index_entry(ia.row_base + (uint32_t)j, ia.ba.total);
}
// the record word behind column x of the image: 0..9, or -1 for a wall
TE_HD int input_source(const InputArgs& ia, const BatchEntry& en, int x) {
    const int c = ia.pad ? x - 1 : x;
    if (c < 0 || c >= NCOL) return -1;
    return en.mirror ? NCOL - 1 - c : c;
}
// pw[x] from the record word of input_source (`word` is not read for a wall)
TE_HD uint64_t input_column(const InputArgs& ia, const BatchEntry& en, int x, uint32_t word) {
    if (!en.valid) return 0ull;
    const int H = ia.ba.H;
    if (!ia.pad) return (uint64_t)(word & plan_row_mask(H));
    const int c = x - 1;
    if (c < 0 || c >= NCOL) return (1ull << (H + 2)) - 1ull;
    return ((uint64_t)(word & plan_row_mask(H)) << 1) | (1ull << (H + 1));
}
TE_HD int input_popcount(uint64_t v) { return __builtin_popcountll(v); }
TE_HD int input_popcount(uint32_t v) { return __builtin_popcount(v); }
// the value of channel code `code` at row y of a column; W = uint64_t, or uint32_t where the image has at most 32 rows (the
// word's low half is then all of it, and (2 << 31) - 1 wraps to thirty-two ones)
template <class W>
TE_HD uint32_t input_cell(W pw, uint32_t keep, int y, uint32_t code) {
    const uint32_t bit = (uint32_t)(pw >> y) & 1u;
    const uint32_t cum = (uint32_t)input_popcount((W)(pw & (W)(((W)2 << y) - (W)1)));
    const uint32_t shadow = cum ? 1u : 0u;
    return code == (uint32_t)INPUT_RAW ? bit : code == (uint32_t)INPUT_CUMSUM ? cum : code == (uint32_t)INPUT_SHADOW ? shadow
         : code == (uint32_t)INPUT_HEIGHT ? (keep ? (uint32_t)y : 0u) : shadow - bit;
}
TE_HD uint32_t input_code(const InputArgs& ia, int ch) { return (ia.chan >> (4 * ch)) & 15u; }

// the binary16 bits of an integer v in [0, 2047] (exact)
TE_HD uint16_t input_f16_bits(uint32_t v) {
    if (v == 0u) return (uint16_t)0;
    const uint32_t e = 31u - (uint32_t)clz32(v);                 // v = 1.f x 2^e, e <= 10
    return (uint16_t)(((e + 15u) << 10) | ((v << (10u - e)) & 0x3FFu));
}
// element `at` of an output from the integer v
TE_HD void input_store(void* out, size_t at, uint32_t v, int f16) {
    if (f16) reinterpret_cast<uint16_t*>(out)[at] = input_f16_bits(v);
    else reinterpret_cast<float*>(out)[at] = (float)v;
}
// byte k of the three vector words
TE_HD uint32_t input_vector_byte(uint32_t v0, uint32_t v1, uint32_t v2, int k) {
    const uint32_t w = k < 4 ? v0 : k < 8 ? v1 : v2;
    return (w >> (8 * (k & 3))) & 255u;
}

// Serial form of sample j, slot sl (CPU harness; the kernel streams a workgroup's run of samples out in memory order instead)
TE_HD void input_sample_slot(const InputArgs& ia, int j, int sl) {
    const BatchEntry en = input_entry(ia, j);
    const uint32_t* rec = ia.ba.obs + ((size_t)en.at * ia.ba.n_slots + sl) * OBS_WORDS;
    const size_t s = (size_t)sl * ia.ba.m + j;
    if (ia.visual) {
        uint64_t pw[INPUT_MAX_W];
        for (int x = 0; x < ia.Wp; x++) {
            const int c = input_source(ia, en, x);
            pw[x] = input_column(ia, en, x, c < 0 ? 0u : rec[c]);
        }
        const uint32_t keep = en.valid ? 1u : 0u;
        for (int ch = 0; ch < ia.C; ch++)
            for (int y = 0; y < ia.Hp; y++)
                for (int x = 0; x < ia.Wp; x++) {
                    const size_t at = ia.last ? ((size_t)y * ia.Wp + x) * ia.C + ch : ((size_t)ch * ia.Hp + y) * ia.Wp + x;
                    input_store(ia.visual, s * (size_t)ia.E + at, input_cell(pw[x], keep, y, input_code(ia, ch)), ia.f16);
                }
    }
    uint32_t v0, v1, v2, piece;
    batch_scalars(en, rec[10], rec[11], v0, v1, v2, piece);
    if (ia.vector)
        for (int k = 0; k < 12; k++) input_store(ia.vector, s * 12 + (size_t)k, input_vector_byte(v0, v1, v2, k), ia.f16);
    if (ia.piece) ia.piece[s] = (uint8_t)piece;
    if (sl == 0 && ia.valid) ia.valid[j] = en.valid ? (uint8_t)1 : (uint8_t)0;
}

}  // namespace te
