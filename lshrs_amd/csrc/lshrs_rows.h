// lshrs_rows.h - what the kernels over stored rows share (rerank.hip, scan.hip, query.hip), each rule stated once: the element
// types of a stored row and their EXACT conversions to f32, the wave's sum, the orderable key of a score, the 64-bit item the
// bitonic networks sort, and (bitonic_pass.inc) one pass of the LDS network.  The project's exactness claims (a score is computed from the very
// f32 the stored bits denote; an order by key is the order by score) rest on what stands here.
// Everything is inline (no state, nothing exported), like lshrs_common.h.
#ifndef LSHRS_ROWS_H
#define LSHRS_ROWS_H

#include "lshrs_common.h"

namespace lshrs {

// ------------------------------------------------------------------------------------------
// element types: float itself, and tags for rows of 16 bits (uint16_t) and of 8 bits (int8_t / uint8_t)
// ------------------------------------------------------------------------------------------
struct Bf16 {};
struct F16 {};
struct I8 {};
struct F8E4M3 {};

template <typename E> struct RowElem;                 // T: what a row holds
template <> struct RowElem<float> { using T = float; };
template <> struct RowElem<Bf16> { using T = uint16_t; };
template <> struct RowElem<F16> { using T = uint16_t; };
template <> struct RowElem<I8> { using T = int8_t; };
template <> struct RowElem<F8E4M3> { using T = uint8_t; };
template <typename E> using RowT = typename RowElem<E>::T;
template <typename E> constexpr int kRowPerDword = 4 / (int)sizeof(RowT<E>);      // elements a dword holds: 1, 2 or 4

// A lone element to f32, exactly.  e4m3fn goes through gfx950's fp8 conversion, which reads the OCP encoding (not MI300's
// fnuz): subnormals kept, 0x7f / 0xff -> NaN.
__device__ __forceinline__ float row_elem_f32(float, float v) { return v; }
__device__ __forceinline__ float row_elem_f32(Bf16, uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ float row_elem_f32(F16, uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
__device__ __forceinline__ float row_elem_f32(I8, int8_t v) { return (float)v; }
__device__ __forceinline__ float row_elem_f32(F8E4M3, uint8_t v) { return __builtin_amdgcn_cvt_f32_fp8((int)v, 0); }

// One dword of a row to its 1, 2 or 4 elements as f32, exactly, in memory order (x[0] = the lowest address).
__device__ __forceinline__ void row_unpack(float, uint32_t w, float (&x)[1]) { x[0] = __uint_as_float(w); }
__device__ __forceinline__ void row_unpack(Bf16, uint32_t w, float (&x)[2]) {
  x[0] = __uint_as_float(w << 16);
  x[1] = __uint_as_float(w & 0xffff0000u);
}
__device__ __forceinline__ void row_unpack(F16, uint32_t w, float (&x)[2]) {
  x[0] = (float)__builtin_bit_cast(_Float16, (uint16_t)w);
  x[1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
}
__device__ __forceinline__ void row_unpack(I8, uint32_t w, float (&x)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = (float)(int8_t)(w >> (8 * j));
}
__device__ __forceinline__ void row_unpack(F8E4M3, uint32_t w, float (&x)[4]) {
  // (one conversion per byte, like int8's: each result feeds a packed FMA as it is - the pairwise conversion's pairs would
  // have to be taken apart first)
  x[0] = __builtin_amdgcn_cvt_f32_fp8((int)w, 0);
  x[1] = __builtin_amdgcn_cvt_f32_fp8((int)w, 1);
  x[2] = __builtin_amdgcn_cvt_f32_fp8((int)w, 2);
  x[3] = __builtin_amdgcn_cvt_f32_fp8((int)w, 3);
}

// the sum of a value over the wave's 64 lanes, in every lane (a butterfly: the same tree of additions in each)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ------------------------------------------------------------------------------------------
// the orderable key of a score, and the items the networks sort
// ------------------------------------------------------------------------------------------
// The bits of a float as an unsigned number in the floats' own (sign-magnitude) order, ascending: a negative float's bits
// complemented, the others' with the sign bit set - so -0.0 lies below +0.0, and a NaN wherever its bits put it.  DESC: the
// complement of that, arm by arm.  (Both in one text: written as ~ of the ascending form the compiler loses an instruction.)
template <bool DESC>
__device__ __forceinline__ uint32_t orderable_bits(uint32_t u) {
  if (u & 0x80000000u) return DESC ? u : ~u;
  return DESC ? (u ^ 0x7fffffffu) : (u | 0x80000000u);
}
// Ascending key of a score (the scan's selection: NaN is kept out by its callers).  Every key is above 0: the key of -inf is
// 0x007fffff.
__device__ __forceinline__ uint32_t asc_key(float f) { return orderable_bits<false>(__float_as_uint(f)); }
__device__ __forceinline__ float asc_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// Descending key: ascending key == descending score, +0.0 ahead of -0.0, and NaN after everything (no other score has the key
// 0xFFFFFFFF: its ascending key would be 0).
__device__ __forceinline__ uint32_t desc_key(float f) {
  if (f != f) return 0xFFFFFFFFu;
  return orderable_bits<true>(__float_as_uint(f));
}

// An item: the key above a 32-bit tie-breaker, one 64-bit compare for both.
__device__ __forceinline__ uint64_t key_item(uint32_t key, uint32_t low) { return ((uint64_t)key << 32) | low; }
// ... of a score at a position of its list: ascending items == descending scores, ties by ascending position, NaN last; ~0 (the
// padding of a list to the network's size) sorts behind every real item (no position is 0xFFFFFFFF).
__device__ __forceinline__ uint64_t desc_item(float score, uint32_t pos) { return key_item(desc_key(score), pos); }

// One compare-exchange pass of the LDS bitonic network over such items: bitonic_pass.inc, a text the kernels #include (it says
// why it is no function here).

}  // namespace lshrs

#endif
