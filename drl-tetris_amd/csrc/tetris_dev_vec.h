// Kernels of libtetris_hip.so, part 0: no kernel, but what the kernel headers share to move runs of float32 or binary16 elements
// between memory and LDS 16 bytes at a time: the vector type, its elements, the hardware's binary16 decode and the step from a
// runtime (K, f16) to template arguments.  Needs tetris_game_kernel.h (u2f, f2u, plan_f32_to_f16).  Loops stay with their kernels.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// binary16 bits -> float32 by the hardware's conversion.  Exact, as act_f16_to_f32 (tetris_act.h) is, but nobody has compared the
// two on NaNs: a kernel keeps the one it was written and tested with.
__device__ __forceinline__ float vec_f16_to_f32(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }

// element j of a 16-byte vector as float32, a binary16 through `decode` (j is not a constant: selects, no indexed registers)
template <bool F16, class D>
__device__ __forceinline__ float vec_element(const u32x4& q, int j, D decode) {
    const int w = F16 ? j >> 1 : j;
    const uint32_t word = w == 0 ? q.x : w == 1 ? q.y : w == 2 ? q.z : q.w;
    return F16 ? decode((uint16_t)((j & 1) ? word >> 16 : word & 0xFFFFu)) : u2f(word);
}
// 0 | val into element j of a zeroed 16-byte vector (j is not a constant: selects, no indexed registers)
template <bool F16>
__device__ __forceinline__ void vec_put(u32x4& q, int j, float val) {
    const int w = F16 ? j >> 1 : j;
    const uint32_t bits = F16 ? (uint32_t)plan_f32_to_f16(val) << ((j & 1) * 16) : f2u(val);
    q.x |= w == 0 ? bits : 0u; q.y |= w == 1 ? bits : 0u; q.z |= w == 2 ? bits : 0u; q.w |= w == 3 ? bits : 0u;
}

// Runtime value -> template argument on the device, as with_flag / with_value of tetris_host.h on the host: f(F16, a...) with
// std::true_type or std::false_type, and f(K, F16, a...) with K = std::integral_constant<int, 7 or 1> (the argument rules admit
// no other K).  f is a generic lambda that names its body with them (act_gather<NT, K(), F16()>(a...)) and captures nothing:
// what the body needs goes through as a... — a closure of references changed the kernels' code (profiles/layout/isa_compare_agent.txt).
template <class F, class... A>
__device__ __forceinline__ void vec_with_f16(bool f16, F&& f, A&&... a) { if (f16) f(std::true_type{}, a...); else f(std::false_type{}, a...); }
template <class F, class... A>
__device__ __forceinline__ void vec_with_k_f16(int K, bool f16, F&& f, A&&... a) {
    if (K == 7) {
        if (f16) f(std::integral_constant<int, 7>{}, std::true_type{}, a...); else f(std::integral_constant<int, 7>{}, std::false_type{}, a...);
    } else {
        if (f16) f(std::integral_constant<int, 1>{}, std::true_type{}, a...); else f(std::integral_constant<int, 1>{}, std::false_type{}, a...);
    }
}
