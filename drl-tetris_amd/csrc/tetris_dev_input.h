// Kernels of libtetris_hip.so, part 10: the network's input side, padded plane stacks from packed records (bodies: tetris_input.h).
// Needs tetris_dev_vec.h.

// ---- the network inputs (tetris_input.h).  One launch per call.  A workgroup takes INPUT_BLOCK = 8 consecutive samples of one
// slot (blockIdx.y).  Its run of `visual` is 8 E contiguous elements in both layouts — [M] is the outer index of a slot — so the
// kernel is a store stream with a small head:
//   head: thread (sample, k), k = 0..11, 96 of the 256: the sample's entry (input_entry: the index load is shared by the twelve),
//     ONE record word — the one behind column k of the image, mirror and pad resolved — into the padded column word pw[sample][k]
//     in LDS, and element k of `vector` from the record's two scalar words (the twelve threads read the same two words; their
//     stores are 12 consecutive elements per sample).  Thread k = 0 also writes `piece` and, in slot 0, `valid`.
//   stream: every lane builds 16 bytes of consecutive output elements — 4 float32 or 8 binary16 — from the flat offset: (sample,
//     channel, y, x) by three multiplications with the reciprocals the host put into InputArgs, then along memory order without a
//     division; per element one LDS read of pw, two shifts, a popcount and selects (input_cell).  A wave instruction stores 1 KB
//     contiguous, non-temporal.  The vectors start at the first 16-byte boundary of the run, wherever the output's base lies: the
//     at most 3 (7) elements before it and behind the last whole vector leave one by one, so an output that is only aligned to
//     its element streams at the same rate.
// W, the type of a column word in LDS, is uint32_t where the image has at most 32 rows — every height but 31 with the pad — and
// uint64_t for the 33 rows of that one: with 64-bit words throughout the stream took up to 10 % longer.  With one channel both
// layouts are the same memory: the host launches the channels-first form.  The element type's conversion is the hardware's
// (v_cvt_f32_u32, v_cvt_f16_f32: exact for these integers), not plan_f32_to_f16.  Lanes of a wave read at most a few distinct pw
// words at a time (consecutive x of one or two samples); equal addresses broadcast.  LDS: 416 or 800 bytes.  No workgroup waits
// for another; no atomics.
template <class W>
struct InputShared {
    alignas(8) W pw[INPUT_BLOCK][INPUT_MAX_W];
    uint32_t keep[INPUT_BLOCK];
};
static_assert(INPUT_BLOCK * 12 <= INPUT_THREADS, "a thread per (sample, vector element)");
static_assert(INPUT_BLOCK * 5 * 33 * 12 < (1 << 16), "input_div: a workgroup's offsets stay below 2^16");

template <typename T>
__device__ __forceinline__ T input_encode(uint32_t v) {
    if constexpr (sizeof(T) == 2) return __builtin_bit_cast(uint16_t, (_Float16)(float)v);
    else return (float)v;
}
template <class W>
__device__ __forceinline__ uint32_t input_value(const InputArgs& ia, const InputShared<W>& sh, const InputPos& p) {
    return input_cell<W>(sh.pw[p.j][p.x], sh.keep[p.j], p.y, input_code(ia, p.ch));
}

template <typename T, bool LAST, class W>
__device__ __forceinline__ void input_stream(const InputArgs& ia, const InputShared<W>& sh, int sl, int first, int nb) {
    constexpr int EPV = 16 / (int)sizeof(T);
    const uint32_t total = (uint32_t)nb * (uint32_t)ia.E, t = threadIdx.x;
    T* out = (T*)ia.visual + ((size_t)sl * ia.ba.m + first) * (size_t)ia.E;
    const uint32_t lead = (uint32_t)((16u - (uint32_t)((uintptr_t)out & 15u)) & 15u) / (uint32_t)sizeof(T);
    const uint32_t head = lead < total ? lead : total;
    const uint32_t nvec = (total - head) / EPV, tail = head + nvec * EPV;
    for (uint32_t v = t; v < nvec; v += INPUT_THREADS) {
        const uint32_t e0 = head + v * EPV;
        InputPos p = input_pos(ia, e0);
        uint32_t val[EPV];
        TE_UNROLL
        for (int q = 0; q < EPV; q++) {
            val[q] = input_value(ia, sh, p);
            input_next<LAST>(ia, p);
        }
        u32x4 w;
        if constexpr (sizeof(T) == 2) {
            w.x = (uint32_t)input_encode<T>(val[0]) | ((uint32_t)input_encode<T>(val[1]) << 16);
            w.y = (uint32_t)input_encode<T>(val[2]) | ((uint32_t)input_encode<T>(val[3]) << 16);
            w.z = (uint32_t)input_encode<T>(val[4]) | ((uint32_t)input_encode<T>(val[5]) << 16);
            w.w = (uint32_t)input_encode<T>(val[6]) | ((uint32_t)input_encode<T>(val[7]) << 16);
        } else {
            w.x = f2u(input_encode<T>(val[0])); w.y = f2u(input_encode<T>(val[1]));
            w.z = f2u(input_encode<T>(val[2])); w.w = f2u(input_encode<T>(val[3]));
        }
        __builtin_nontemporal_store(w, reinterpret_cast<u32x4*>(out + e0));
    }
    // the elements before the first vector and behind the last: fewer than 2 EPV
    const uint32_t edge = head + (total - tail);
    if (t < edge) {
        const uint32_t e = t < head ? t : tail + (t - head);
        out[e] = input_encode<T>(input_value(ia, sh, input_pos(ia, e)));
    }
}

template <typename T, bool LAST, class W>
__global__ __launch_bounds__(INPUT_THREADS) void k_net_input(InputArgs ia) {
    __shared__ InputShared<W> sh;
    const int t = (int)threadIdx.x, sl = (int)blockIdx.y, first = (int)blockIdx.x * INPUT_BLOCK, nb = imin(INPUT_BLOCK, ia.ba.m - first);
    const int s = t / 12, k = t - s * 12;
    if (s < nb) {
        const int j = first + s;
        const BatchEntry en = input_entry(ia, j);
        const uint32_t* rec = ia.ba.obs + ((size_t)en.at * ia.ba.n_slots + sl) * OBS_WORDS;
        if (ia.visual && k < ia.Wp) {
            const int c = input_source(ia, en, k);
            sh.pw[s][k] = (W)input_column(ia, en, k, c < 0 ? 0u : rec[c]);
            if (k == 0) sh.keep[s] = en.valid ? 1u : 0u;
        }
        if (ia.vector || ia.piece) {
            uint32_t v0, v1, v2, piece;
            batch_scalars(en, rec[10], rec[11], v0, v1, v2, piece);
            const size_t at = (size_t)sl * ia.ba.m + j;
            if (ia.vector) ((T*)ia.vector)[at * 12 + (size_t)k] = input_encode<T>(input_vector_byte(v0, v1, v2, k));
            if (ia.piece && k == 0) ia.piece[at] = (uint8_t)piece;
        }
        if (ia.valid && k == 0 && sl == 0) ia.valid[j] = en.valid ? (uint8_t)1 : (uint8_t)0;
    }
    if (!ia.visual) return;
    __syncthreads();
    input_stream<T, LAST, W>(ia, sh, sl, first, nb);
}
