// rerank.hip - part of liblshrs_hip.so, the gfx950 (MI355X / CDNA4) implementation of the lshrs hot path.
// K2 cosine of gathered candidates (gather + dot + norm), L2 normalisation, K3 per-query descending order (LDS bitonic
// network; longer lists through global memory).
// One translation unit per kernel family (round 5): what is shared lives in lshrs_common.h and - the element types of a stored
// row and their exact conversions, the wave's sum, the orderable key of a score and the networks' item: shared with scan.hip
// and query.hip - in lshrs_rows.h; measurement switches (-DLSHRS_AB_*, tools/ab_build.py) are local to the unit whose kernel
// they alter and reported through lshrs_build_flags().
// Two layers are texts #included where they run (each says why it is no function): cos_finish.inc, the end of a candidate;
// bitonic_pass.inc, one pass of the LDS network (also query.hip's).
// ABI and reference citations: include/lshrs_hip.h.  Design notes: DESIGN.md.
#include "lshrs_rows.h"

#include <type_traits>

using namespace lshrs;

namespace {
// ------------------------------------------------------------------------------------------
// K2: cosine of gathered candidates against a query.  One workgroup = one (query, slice of
// its candidates); the query sits in LDS, each wave streams whole candidate rows (16 B per
// lane per load, four rows in flight), reduces dot and ||c||^2 across the wave, and lane 0
// writes dot / (||c|| * ||q||).
// A corpus stored in 16 bits (bf16 / f16) takes the same kernel: each element is converted to
// f32 exactly in registers, every product and sum stays an f32 FMA against the f32 query; a
// 16-B load holds 8 elements, and eight rows are in flight to keep the bytes per wave of f32
// (their indices and row pointers in scalar registers: 114 VGPRs, four waves per SIMD).
// A corpus stored in 8 bits (int8 / OCP fp8 e4m3fn) likewise: a 16-B load holds 16 elements and
// sixteen rows are in flight, the bytes per wave of f32 and of 16 bits again (152 / 164 VGPRs,
// three waves per SIMD).  Its 32 sums are reduced together and 16 lanes finish the 16 rows at
// once: with a wave_sum and a lane-0 epilogue per row the 8-bit kernel was no faster than bf16.
// ------------------------------------------------------------------------------------------
constexpr int kCosThreads = 256;
constexpr int kCosWaves = kCosThreads / 64;
constexpr int kCosInflight = 4;

// per element type (lshrs_rows.h: the tags, RowT<E>, the conversions): rows in flight per wave, elements per 16-B load
template <typename E> struct CosElem {
  using T = RowT<E>;
  static constexpr int kVec = 4 * kRowPerDword<E>;
  static constexpr int kInflight = kRowPerDword<E> * kCosInflight;
};

// RAGGED (ABI 7, lshrs_cosine_ragged_f32): query qi has row_cnt[qi] candidates, listed - and scored - at row_off[qi] of the
// flat cand_idx / scores arrays (the candidate lists of a batch of LSH queries, lshrs/core/main.py:629-646); what is wrong with
// a candidate is OR-ed into err[0] (1 zero norm, 2 index outside the corpus) instead of a status byte per candidate.
// E: float, Bf16, F16, I8 or F8E4M3 - the corpus's element type (ldc in elements); queries, scores and status are f32 / u8 for
// all of them.
template <typename E, bool ALIGNED, bool RAGGED>
__global__ __launch_bounds__(kCosThreads) void cosine_kernel(const typename CosElem<E>::T* __restrict__ corpus, int64_t m,
                                                             int64_t ldc, int dim, const float* __restrict__ queries,
                                                             const int64_t* __restrict__ cand_idx, int c, int slices,
                                                             float* __restrict__ scores, uint8_t* __restrict__ status,
                                                             uint8_t* __restrict__ qstatus,
                                                             const int64_t* __restrict__ row_off,
                                                             const int32_t* __restrict__ row_cnt, int32_t* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) float qlds[];  // dim floats (+ pad to 4) + kCosWaves partials
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // (16- and 8-bit rows: the wave index said to be wave-uniform, so that a wave's candidate indices and row pointers sit in scalar
  // registers - eight / sixteen rows in flight then leave the vector registers for the data)
  const int wave = std::is_same_v<E, float> ? tid >> 6 : __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = blockIdx.x / slices;
  const int slice = blockIdx.x % slices;
  int64_t obase = (int64_t)qi * c;
  if (RAGGED) {
    c = row_cnt[qi];
    obase = row_off[qi];
    if (slice * ((c + slices - 1) / slices) >= c) return;     // (nothing in this slice: the whole workgroup leaves together)
  }
  const int dim4 = (dim + 3) & ~3;
  const float* __restrict__ qv = queries + (int64_t)qi * dim;

  float qq = 0.f;
  for (int k = tid; k < dim4; k += kCosThreads) {
    const float v = k < dim ? qv[k] : 0.f;
    qlds[k] = v;
    qq = __builtin_fmaf(v, v, qq);
  }
  qq = wave_sum(qq);
  float* part = qlds + dim4;
  if (lane == 0) part[wave] = qq;
  __syncthreads();
  float qnorm2 = 0.f;
#pragma unroll
  for (int w = 0; w < kCosWaves; ++w) qnorm2 += part[w];
  const float qnorm = sqrtf(qnorm2);
  if (slice == 0 && tid == 0 && qstatus != nullptr) qstatus[qi] = (qnorm == 0.f) ? 1 : 0;
  if (RAGGED && slice == 0 && tid == 0 && err != nullptr && qnorm == 0.f) atomicOr(err, 4);

  // candidates of this slice, dealt to waves in groups of kInflight
  using T = typename CosElem<E>::T;
  constexpr int kInflight = CosElem<E>::kInflight;
  const int per_slice = (c + slices - 1) / slices;
  const int c_begin = slice * per_slice;
  const int c_end = min(c, c_begin + per_slice);

  for (int base = c_begin + wave * kInflight; base < c_end; base += kCosWaves * kInflight) {
    const T* rowp[kInflight];
    int st[kInflight];
#pragma unroll
    for (int u = 0; u < kInflight; ++u) {
      const int ci = base + u;
      int64_t idx = 0;
      st[u] = 3;  // 3 = not a candidate (past the end)
      if (ci < c_end) {
        idx = cand_idx != nullptr ? cand_idx[obase + ci] : obase + ci;
        st[u] = (idx < 0 || idx >= m) ? 2 : 0;
      }
      rowp[u] = corpus + (st[u] == 0 ? idx : 0) * ldc;
    }
    float dot[kInflight], nn[kInflight];
#pragma unroll
    for (int u = 0; u < kInflight; ++u) { dot[u] = 0.f; nn[u] = 0.f; }

    // elements of a dword in memory order, dwords in order: the same sums per lane for every type
    constexpr int kPer = kRowPerDword<E>, kVec = CosElem<E>::kVec;
    if (ALIGNED) {
      // kVec elements per lane per load (dim, ldc multiples of kVec, 16-B aligned base): one 16-B load of the row
      for (int k = lane * kVec; k < dim; k += 64 * kVec) {
        float qx[kVec];
#pragma unroll
        for (int v = 0; v < kPer; ++v) {
          const f32x4 qv4 = *reinterpret_cast<const f32x4*>(qlds + k + 4 * v);
#pragma unroll
          for (int e = 0; e < 4; ++e) qx[4 * v + e] = qv4[e];
        }
        u32x4 cx[kInflight];
#pragma unroll
        for (int u = 0; u < kInflight; ++u) cx[u] = *reinterpret_cast<const u32x4*>(rowp[u] + k);
#pragma unroll
        for (int u = 0; u < kInflight; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float x[kPer];
            row_unpack(E{}, cx[u][e], x);
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
              dot[u] = __builtin_fmaf(x[j], qx[kPer * e + j], dot[u]);
              nn[u] = __builtin_fmaf(x[j], x[j], nn[u]);
            }
          }
      }
    } else {
      // any dim, row stride and address: one element per lane per load
      for (int k = lane; k < dim; k += 64) {
        const float qx = qlds[k];
#pragma unroll
        for (int u = 0; u < kInflight; ++u) {
          const float cx = row_elem_f32(E{}, rowp[u][k]);
          dot[u] = __builtin_fmaf(cx, qx, dot[u]);
          nn[u] = __builtin_fmaf(cx, cx, nn[u]);
        }
      }
    }
    if constexpr (sizeof(T) == 1) {
      // 8 bits: the 32 sums of the 16 rows (dot, ||c||^2) reduced together.  At each butterfly step a lane keeps one value of
      // every pair and sends the other (the same additions as wave_sum's, in the same tree: bit for bit its totals), so the
      // values per lane halve: 33 exchanges instead of 192.  Then lane L < 32 holds the dot of row bitrev4((L >> 1) & 15),
      // lane L + 32 its ||c||^2, and 16 lanes finish their rows at once.
      static_assert(kInflight == 16, "the transposed reduction below is written for 16 rows");
      float v[2 * kInflight];
#pragma unroll
      for (int u = 0; u < kInflight; ++u) { v[2 * u] = dot[u]; v[2 * u + 1] = nn[u]; }
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        const int mask = 32 >> s;
        const bool hi = (lane & mask) != 0;
#pragma unroll
        for (int i = 0; i < (16 >> s); ++i) {
          const float send = hi ? v[2 * i] : v[2 * i + 1];
          const float keep = hi ? v[2 * i + 1] : v[2 * i];
          v[i] = keep + __shfl_xor(send, mask);
        }
      }
      const float d = v[0] + __shfl_xor(v[0], 1);
      const float s2 = __shfl_xor(d, 32);
      const int ur = ((lane >> 1) & 1) << 3 | ((lane >> 2) & 1) << 2 | ((lane >> 3) & 1) << 1 | ((lane >> 4) & 1);
      int code = 3;
#pragma unroll
      for (int u = 0; u < kInflight; ++u) code = (u == ur) ? st[u] : code;
      if ((lane & 33) == 0 && code != 3) {
        const int64_t o = obase + base + ur;
#include "cos_finish.inc"
      }
      continue;
    }
#pragma unroll
    for (int u = 0; u < kInflight; ++u) {
      const float d = wave_sum(dot[u]);
      const float s2 = wave_sum(nn[u]);
      if (lane == 0 && st[u] != 3) {
        const int64_t o = obase + base + u;
        int code = st[u];
#include "cos_finish.inc"
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// l2_norm: out = x / ||x||, one workgroup per row (reference helper lshrs/utils/norm.py:48-61)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ X, int64_t ldx, int dim,
                                                           float* __restrict__ out, uint8_t* __restrict__ status) {
  __shared__ float part[4];
  const int64_t row = blockIdx.x;
  const float* x = X + row * ldx;
  float ss = 0.f;
  for (int k = threadIdx.x; k < dim; k += 256) ss = __builtin_fmaf(x[k], x[k], ss);
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float norm = sqrtf(part[0] + part[1] + part[2] + part[3]);
  if (threadIdx.x == 0 && status != nullptr) status[row] = (norm == 0.f) ? 1 : 0;
  float* o = out + row * (int64_t)dim;
  for (int k = threadIdx.x; k < dim; k += 256) o[k] = x[k] / norm;
}

// ------------------------------------------------------------------------------------------
// quantize_rows: an f32 row to 8-bit codes with its own symmetric scale, one workgroup per row.
// s = Q / max|x| (one f32 division), code = x * s rounded to nearest-even.  The scale is not
// kept: a cosine does not see it.  status: 0 written; 1 a non-finite element, 2 max|x| so small
// that Q / max|x| overflows - both rows written as zeros.  A zero row stays zero (status 0).
// ------------------------------------------------------------------------------------------
template <typename E> struct QuantCode;
template <> struct QuantCode<I8> {
  static constexpr float kQ = 127.f;
  __device__ static int8_t encode(float v) {       // clamped to [-127, 127]: -128 is never written
    return (int8_t)fminf(fmaxf(__builtin_rintf(v), -127.f), 127.f);
  }
};
template <> struct QuantCode<F8E4M3> {
  static constexpr float kQ = 448.f;
  // OCP e4m3fn, round to nearest-even; |v| <= 448 up to the rounding of x * s, never NaN
  __device__ static uint8_t encode(float v) {
    const uint32_t u = __float_as_uint(v) & 0x7fffffffu;
    const uint32_t sign = (__float_as_uint(v) >> 24) & 0x80u;
    uint32_t code;
    if (u < 0x3c800000u)                      // below 2^-6: multiples of 2^-9 (code 8 = 2^-6, the least normal)
      code = (uint32_t)__builtin_rintf(__uint_as_float(u) * 512.f);
    else                                      // 3 mantissa bits kept, ties to even; a carry moves into the exponent
      code = ((u + 0x7ffffu + ((u >> 20) & 1u)) >> 20) - (120u << 3);
    return (uint8_t)(sign | min(code, 0x7eu));  // (0x7e = 448, the largest finite code)
  }
};

template <typename E>
__global__ __launch_bounds__(256) void quantize_rows_kernel(const float* __restrict__ X, int64_t ldx, int dim,
                                                            typename CosElem<E>::T* __restrict__ out, int64_t ldo,
                                                            uint8_t* __restrict__ status) {
  __shared__ float pmax[4];
  __shared__ int pbad[4];
  const int64_t row = blockIdx.x;
  const float* x = X + row * ldx;
  float amax = 0.f;
  int bad = 0;
  for (int k = threadIdx.x; k < dim; k += 256) {
    const float a = fabsf(x[k]);
    bad |= !(a <= __FLT_MAX__);               // (inf and NaN)
    amax = fmaxf(amax, a);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    amax = fmaxf(amax, __shfl_xor(amax, off));
    bad |= __shfl_xor(bad, off);
  }
  if ((threadIdx.x & 63) == 0) {
    pmax[threadIdx.x >> 6] = amax;
    pbad[threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  amax = fmaxf(fmaxf(pmax[0], pmax[1]), fmaxf(pmax[2], pmax[3]));
  bad = pbad[0] | pbad[1] | pbad[2] | pbad[3];
  const float s = __fdiv_rn(QuantCode<E>::kQ, amax);
  const int code = bad ? 1 : (amax != 0.f && !(s <= __FLT_MAX__)) ? 2 : 0;
  if (threadIdx.x == 0) status[row] = (uint8_t)code;
  auto* o = out + row * ldo;
  for (int k = threadIdx.x; k < dim; k += 256) {
    const float v = (code == 0 && amax != 0.f) ? x[k] * s : 0.f;
    o[k] = QuantCode<E>::encode(v);
  }
}

// ------------------------------------------------------------------------------------------
// K3: descending order of each query's scores: bitonic network over 64-bit (key, position)
// pairs in LDS.  key ascending == score descending; NaN last; ties by ascending position.
// ------------------------------------------------------------------------------------------
constexpr int kTopkThreads = 256;

__global__ __launch_bounds__(kTopkThreads) void topk_kernel(const float* __restrict__ scores, int c, int cpad, int k,
                                                            int32_t* __restrict__ order, float* __restrict__ sorted) {
  extern __shared__ __attribute__((aligned(16))) uint64_t items[];
  const int qi = blockIdx.x;
  const float* s = scores + (int64_t)qi * c;
  for (int t = threadIdx.x; t < cpad; t += kTopkThreads)
    items[t] = t < c ? desc_item(s[t], (uint32_t)t) : ~0ull;   // (padding: behind every real item)
  __syncthreads();
  constexpr int kPassThreads = kTopkThreads, base = 0;
  const int n = cpad;
  for (int size = 2; size <= cpad; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
#include "bitonic_pass.inc"
    }
  for (int t = threadIdx.x; t < k; t += kTopkThreads) {
    const uint32_t pos = (uint32_t)items[t];
    order[(int64_t)qi * k + t] = (int32_t)pos;
    sorted[(int64_t)qi * k + t] = s[pos];
  }
}

// ---- lists longer than one LDS network: the same bitonic network over a global u64 array ------------
constexpr int kTopkChunk = 4096;  // items per workgroup-local stage (32 KiB of LDS)

__global__ void topk_fill_kernel(const float* __restrict__ scores, int c, int64_t cpad, uint64_t* __restrict__ items) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cpad) return;
  const int qi = blockIdx.y;
  items[(int64_t)qi * cpad + t] = t < c ? desc_item(scores[(int64_t)qi * c + t], (uint32_t)t) : ~0ull;
}

// All compare-exchange steps with stride < kTopkChunk of one merge size (or, with full = true, the whole
// network up to size kTopkChunk) on a chunk held in LDS.  Direction follows the GLOBAL index.
__global__ __launch_bounds__(kTopkThreads) void topk_local_kernel(uint64_t* __restrict__ rows, int64_t cpad, int64_t merge,
                                                                  bool full) {
  __shared__ uint64_t items[kTopkChunk];
  constexpr int kPassThreads = kTopkThreads, n = kTopkChunk;
  const int qi = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * kTopkChunk;
  uint64_t* g = rows + (int64_t)qi * cpad + base;
  for (int t = threadIdx.x; t < kTopkChunk; t += kTopkThreads) items[t] = g[t];
  __syncthreads();
  const int64_t first = full ? 2 : merge;
  const int64_t last = full ? kTopkChunk : merge;
  for (int64_t size = first; size <= last; size <<= 1) {
    const int top = (int)((size < (int64_t)kTopkChunk ? size : (int64_t)kTopkChunk) >> 1);
    for (int stride = top; stride > 0; stride >>= 1) {
#include "bitonic_pass.inc"
    }
  }
  for (int t = threadIdx.x; t < kTopkChunk; t += kTopkThreads) g[t] = items[t];
}

__global__ void topk_global_step_kernel(uint64_t* __restrict__ items, int64_t cpad, int64_t size, int64_t stride) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (cpad >> 1)) return;
  uint64_t* g = items + (int64_t)blockIdx.y * cpad;
  const int64_t lo = 2 * t - (t & (stride - 1));
  const int64_t hi = lo + stride;
  const bool up = ((lo & size) == 0);
  const uint64_t a = g[lo], b = g[hi];
  if ((a > b) == up) {
    g[lo] = b;
    g[hi] = a;
  }
}

__global__ void topk_emit_kernel(const float* __restrict__ scores, const uint64_t* __restrict__ items, int c, int64_t cpad,
                                 int k, int32_t* __restrict__ order, float* __restrict__ sorted) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k) return;
  const int qi = blockIdx.y;
  const uint32_t pos = (uint32_t)items[(int64_t)qi * cpad + t];
  order[(int64_t)qi * k + t] = (int32_t)pos;
  sorted[(int64_t)qi * k + t] = scores[(int64_t)qi * c + pos];
}

inline int64_t topk_pad(int64_t c) {
  int64_t cpad = kTopkChunk;
  while (cpad < c) cpad <<= 1;
  return cpad;
}
}  // namespace

// Ascending sort of every row of a (q, cpad) array of 64-bit items in global memory (cpad a power of two >= kTopkChunk): the
// network K3 runs for long lists, for the candidate path's lists that do not fit LDS (query.hip).
int lshrs_sort_u64_rows(uint64_t* items, int q, int64_t cpad, hipStream_t s) {
  if (q <= 0 || q > 65535 || cpad < kTopkChunk || (cpad & (cpad - 1)) != 0) return LSHRS_E_BADARG;
  const dim3 half((unsigned)(((cpad >> 1) + 255) / 256), (unsigned)q);
  const dim3 chunks((unsigned)(cpad / kTopkChunk), (unsigned)q);
  hipLaunchKernelGGL(topk_local_kernel, chunks, dim3(kTopkThreads), 0, s, items, cpad, (int64_t)kTopkChunk, true);
  for (int64_t size = 2 * (int64_t)kTopkChunk; size <= cpad; size <<= 1) {
    for (int64_t stride = size >> 1; stride >= kTopkChunk; stride >>= 1)
      hipLaunchKernelGGL(topk_global_step_kernel, half, dim3(256), 0, s, items, cpad, size, stride);
    hipLaunchKernelGGL(topk_local_kernel, chunks, dim3(kTopkThreads), 0, s, items, cpad, size, false);
  }
  return -(int)hipGetLastError();
}

namespace {
// The launcher behind the ten lshrs_cosine_{batch,ragged}_{f32,bf16,f16,i8,f8e4m3} entries, written once for every corpus element
// type and both forms: argument checks (before anything touches a device), slicing, the choice of the aligned path, the launch.
// Batch: c candidates for each query, listed at cand (or, cand == NULL, rows qi * c ..), a status byte each.  RAGGED: `total`
// candidates in all, query qi's row_cnt[qi] at row_off[qi] of cand, what is wrong with them in err.
//
// Slices per query: enough workgroups to fill 256 CUs several times over even for a single query - doubled while the launch
// has fewer than 4096 workgroups and a slice of a list of `len` more than two rounds of a workgroup's rows in flight, up to `cap`.
template <typename E>
int cos_slices(int32_t q, int64_t len, int cap) {
  const int per_block = kCosWaves * CosElem<E>::kInflight;
  int slices = 1;
  while ((int64_t)q * slices < 4096 && (len + slices - 1) / slices > 2 * per_block && slices < cap) slices *= 2;
  return slices;
}

template <typename E, bool RAGGED>
int cosine_launch(const typename CosElem<E>::T* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                  const int64_t* cand, int32_t c, const int64_t* row_off, const int32_t* row_cnt, int64_t total, float* scores,
                  uint8_t* status, uint8_t* qstatus, int32_t* err, void* stream) {
  const int64_t n = RAGGED ? total : c;
  if (q == 0 || n == 0) return 0;
  if (corpus == nullptr || queries == nullptr || scores == nullptr || m <= 0 || dim <= 0 || q < 0 || n < 0 || ldc < dim ||
      (RAGGED && (cand == nullptr || row_off == nullptr || row_cnt == nullptr)))
    return LSHRS_E_BADARG;
  if (dim > 16384) return LSHRS_E_TOOLARGE;
  if (!RAGGED && cand == nullptr && (int64_t)q * c > m) return LSHRS_E_BADARG;
  // from the list every query has; RAGGED: from the AVERAGE list (the lists of one batch are alike: a bucket per band each),
  // and no more than 1024
  const int slices = RAGGED ? cos_slices<E>(q, (total + q - 1) / q, 1024) : cos_slices<E>(q, c, INT32_MAX);
  if ((int64_t)q * slices > 0x7fffffffLL) return LSHRS_E_TOOLARGE;
  constexpr int kVec = CosElem<E>::kVec;
  const bool aligned = (dim % kVec == 0) && (ldc % kVec == 0) && ((reinterpret_cast<uintptr_t>(corpus) & 15) == 0);
  const size_t shmem = (size_t)(((dim + 3) & ~3) + kCosWaves) * sizeof(float);
  const dim3 grid((unsigned)((int64_t)q * slices)), block(kCosThreads);
  dispatch_bool(aligned, [&](auto al) {
    hipLaunchKernelGGL((cosine_kernel<E, decltype(al)::value, RAGGED>), grid, block, shmem, static_cast<hipStream_t>(stream),
                       corpus, m, ldc, dim, queries, cand, RAGGED ? 0 : c, slices, scores, status, qstatus, row_off, row_cnt, err);
  });
  return -(int)hipGetLastError();
}

template <typename E>
int cosine_batch(const typename CosElem<E>::T* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                 const int64_t* cand_idx, int32_t c, float* scores, uint8_t* status, uint8_t* qstatus, void* stream) {
  return cosine_launch<E, false>(corpus, m, ldc, dim, queries, q, cand_idx, c, nullptr, nullptr, 0, scores, status, qstatus, nullptr,
                                 stream);
}

template <typename E>
int cosine_ragged(const typename CosElem<E>::T* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                  const int64_t* cand_rows, const int64_t* row_off, const int32_t* row_cnt, int64_t total, float* scores,
                  int32_t* err, void* stream) {
  return cosine_launch<E, true>(corpus, m, ldc, dim, queries, q, cand_rows, 0, row_off, row_cnt, total, scores, nullptr, nullptr, err,
                                stream);
}

template <typename E>
int quantize_rows(const float* X, int64_t n, int64_t ldx, int32_t dim, typename CosElem<E>::T* out, int64_t ldo,
                  uint8_t* status, void* stream) {
  if (n == 0) return 0;
  if (X == nullptr || out == nullptr || status == nullptr || n < 0 || dim <= 0 || ldx < dim || ldo < dim)
    return LSHRS_E_BADARG;
  if (n > 0x7fffffffLL) return LSHRS_E_TOOLARGE;
  hipLaunchKernelGGL(quantize_rows_kernel<E>, dim3((unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream), X, ldx, dim,
                     out, ldo, status);
  return -(int)hipGetLastError();
}
}  // namespace

extern "C" {

int lshrs_cosine_batch_f32(const float* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                           const int64_t* cand_idx, int32_t c, float* scores, uint8_t* status, uint8_t* qstatus,
                           void* stream) {
  return cosine_batch<float>(corpus, m, ldc, dim, queries, q, cand_idx, c, scores, status, qstatus, stream);
}

int lshrs_cosine_batch_bf16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                            const int64_t* cand_idx, int32_t c, float* scores, uint8_t* status, uint8_t* qstatus,
                            void* stream) {
  return cosine_batch<Bf16>(corpus, m, ldc, dim, queries, q, cand_idx, c, scores, status, qstatus, stream);
}

int lshrs_cosine_batch_f16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                           const int64_t* cand_idx, int32_t c, float* scores, uint8_t* status, uint8_t* qstatus,
                           void* stream) {
  return cosine_batch<F16>(corpus, m, ldc, dim, queries, q, cand_idx, c, scores, status, qstatus, stream);
}

int lshrs_cosine_ragged_f32(const float* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                            const int64_t* cand_rows, const int64_t* row_off, const int32_t* row_cnt, int64_t total,
                            float* scores, int32_t* err, void* stream) {
  return cosine_ragged<float>(corpus, m, ldc, dim, queries, q, cand_rows, row_off, row_cnt, total, scores, err, stream);
}

int lshrs_cosine_ragged_bf16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                             const int64_t* cand_rows, const int64_t* row_off, const int32_t* row_cnt, int64_t total,
                             float* scores, int32_t* err, void* stream) {
  return cosine_ragged<Bf16>(corpus, m, ldc, dim, queries, q, cand_rows, row_off, row_cnt, total, scores, err, stream);
}

int lshrs_cosine_ragged_f16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                            const int64_t* cand_rows, const int64_t* row_off, const int32_t* row_cnt, int64_t total,
                            float* scores, int32_t* err, void* stream) {
  return cosine_ragged<F16>(corpus, m, ldc, dim, queries, q, cand_rows, row_off, row_cnt, total, scores, err, stream);
}

int lshrs_cosine_batch_i8(const int8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                          const int64_t* cand_idx, int32_t c, float* scores, uint8_t* status, uint8_t* qstatus,
                          void* stream) {
  return cosine_batch<I8>(corpus, m, ldc, dim, queries, q, cand_idx, c, scores, status, qstatus, stream);
}

int lshrs_cosine_batch_f8e4m3(const uint8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                              const int64_t* cand_idx, int32_t c, float* scores, uint8_t* status, uint8_t* qstatus,
                              void* stream) {
  return cosine_batch<F8E4M3>(corpus, m, ldc, dim, queries, q, cand_idx, c, scores, status, qstatus, stream);
}

int lshrs_cosine_ragged_i8(const int8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                           const int64_t* cand_rows, const int64_t* row_off, const int32_t* row_cnt, int64_t total,
                           float* scores, int32_t* err, void* stream) {
  return cosine_ragged<I8>(corpus, m, ldc, dim, queries, q, cand_rows, row_off, row_cnt, total, scores, err, stream);
}

int lshrs_cosine_ragged_f8e4m3(const uint8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const float* queries, int32_t q,
                               const int64_t* cand_rows, const int64_t* row_off, const int32_t* row_cnt, int64_t total,
                               float* scores, int32_t* err, void* stream) {
  return cosine_ragged<F8E4M3>(corpus, m, ldc, dim, queries, q, cand_rows, row_off, row_cnt, total, scores, err, stream);
}

int lshrs_quantize_rows_i8(const float* X, int64_t n, int64_t ldx, int32_t dim, int8_t* out, int64_t ldo, uint8_t* status,
                           void* stream) {
  return quantize_rows<I8>(X, n, ldx, dim, out, ldo, status, stream);
}

int lshrs_quantize_rows_f8e4m3(const float* X, int64_t n, int64_t ldx, int32_t dim, uint8_t* out, int64_t ldo,
                               uint8_t* status, void* stream) {
  return quantize_rows<F8E4M3>(X, n, ldx, dim, out, ldo, status, stream);
}

int lshrs_l2_normalize_f32(const float* X, int64_t n, int64_t ldx, int32_t dim, float* out, uint8_t* status,
                           void* stream) {
  if (n == 0) return 0;
  if (X == nullptr || out == nullptr || n < 0 || dim <= 0 || ldx < dim) return LSHRS_E_BADARG;
  if (n > 0x7fffffffLL) return LSHRS_E_TOOLARGE;
  hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream), X, ldx,
                     dim, out, status);
  return -(int)hipGetLastError();
}

int64_t lshrs_topk_workspace_bytes(int32_t q, int32_t c) {
  if (q < 0 || c < 0) return LSHRS_E_BADARG;
  if (c <= 16384) return 0;
  return (int64_t)q * topk_pad(c) * (int64_t)sizeof(uint64_t);
}

int lshrs_topk_desc_f32(const float* scores, int32_t q, int32_t c, int32_t k, int32_t* order, float* sorted,
                        void* workspace, void* stream) {
  if (q == 0 || k == 0) return 0;
  if (scores == nullptr || order == nullptr || sorted == nullptr || q < 0 || c <= 0 || k < 0 || k > c)
    return LSHRS_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (c <= 16384) {  // one LDS-resident network per query
    int cpad = 2;
    while (cpad < c) cpad <<= 1;
    const size_t shmem = (size_t)cpad * sizeof(uint64_t);
    if (shmem > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(topk_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
      if (e != hipSuccess) return -(int)e;
    }
    hipLaunchKernelGGL(topk_kernel, dim3((unsigned)q), dim3(kTopkThreads), shmem, s, scores, c, cpad, k, order, sorted);
    return -(int)hipGetLastError();
  }
  if (workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 7)) return LSHRS_E_BADARG;
  if (q > 65535) return LSHRS_E_TOOLARGE;
  uint64_t* items = static_cast<uint64_t*>(workspace);
  const int64_t cpad = topk_pad(c);
  hipLaunchKernelGGL(topk_fill_kernel, dim3((unsigned)((cpad + 255) / 256), (unsigned)q), dim3(256), 0, s, scores, c, cpad, items);
  const int rc = lshrs_sort_u64_rows(items, q, cpad, s);
  if (rc) return rc;
  hipLaunchKernelGGL(topk_emit_kernel, dim3((unsigned)((k + 255) / 256), (unsigned)q), dim3(256), 0, s, scores, items, c,
                     cpad, k, order, sorted);
  return -(int)hipGetLastError();
}

}  // extern "C"
