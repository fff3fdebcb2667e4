// Small helpers shared by the kernels (everything but otto_covis.hip, which keeps its own):
// 64-lane reductions, order-preserving integer images of floats, 16-byte loads and stores, workspace alignment.
#pragma once
#include "common.h"

namespace otto {

// 256-byte alignment of a workspace piece, in the caller's integer type (size_t and int64_t layouts both exist)
template <typename T>
constexpr T align256(T b) { return (b + 255) / 256 * 256; }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// the operations of wave_reduce: a is the lane's own value, b the other lane's; Max / Min keep a unless b beats it, so a
// NaN never wins over a number
struct Sum { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Or  { template <typename T> __device__ T operator()(T a, T b) const { return a | b; } };
struct And { template <typename T> __device__ T operator()(T a, T b) const { return a & b; } };
struct Max { template <typename T> __device__ T operator()(T a, T b) const { return b > a ? b : a; } };
struct Min { template <typename T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };

// Reduction over the 64 lanes of a wave; every lane gets the result. Butterfly in the order 32, 16, ..., 1: a
// floating-point sum is pinned to that order.
template <typename Op, typename T>
__device__ __forceinline__ T wave_reduce(T v, Op op = Op()) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}

// Order-preserving image of a float: a < b as numbers <=> ordered_key(a) < ordered_key(b) as unsigned integers.
// float32: the bits as they are (-0.0 sorts below +0.0).
__device__ __forceinline__ uint32_t ordered_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_key_inv(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
// float64: -0.0 folded onto +0.0
__device__ __forceinline__ uint64_t ordered_key(double x) {
    const uint64_t b = x == 0.0 ? 0ull : (uint64_t)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_key_inv(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)b);
}
// image of a ranking score: larger = better, never 0; every NaN -> 1, below -inf
__device__ __forceinline__ uint64_t score_key(double x) { return x != x ? 1ull : ordered_key(x); }

}  // namespace otto
