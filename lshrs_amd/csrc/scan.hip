// scan.hip - part of liblshrs_hip.so, the gfx950 (MI355X / CDNA4) implementation of the lshrs hot path.
// K6 exhaustive scan: every row of a device-resident (m, dim) block against a tile of 64 queries on the matrix cores
// (v_mfma_f32_32x32x16_bf16), keeping per query the `window` rows of the largest APPROXIMATE cosine.  The caller rescores the
// window exactly (lshrs_cosine_ragged_*) and settles the answer with lshrs_scan_epsilon (lshrs_amd/_exact.py).
//
// One workgroup = four waves = (a slice of the rows) x (64 queries).  A pass takes 256 rows, 64 per wave as two 32-row MFMA
// tiles.  The rows are the A operand, read from global memory straight into the registers the instruction wants (a lane's
// eight k-values of one row are contiguous: no LDS); the queries are the B operand, split once per launch into two bf16
// terms (hi = the f32's upper 16 bits, mid = the upper 16 bits of q - hi) and laid out in fragment order by
// scan_image_kernel, staged through LDS in chunks of 64 k so that any dim fits.  Within a chunk the lanes' halves take k in
// [32h, 32h + 32): MFMA step s multiplies k = 32h + 8s + j on both operands - a permutation of k, which a sum over k does not
// see - so that a lane's 32 elements of a row are ONE contiguous run (64 bytes of bf16).
// bf16, int8 and e4m3fn rows are exact in bf16 (one term); f16 and f32 rows enter as two terms (x_hi q_hi + x_hi q_mid +
// x_mid q_hi).  ||x||^2 is summed in f32 from the elements already in registers.  One-term rows: chunk c + 1's loads are
// issued before chunk c is multiplied.
// Selection: per query a buffer of `cap` 64-bit items {orderable score, ~row} - cap = the power of two at or above 2 * window,
// at least 64 - and a threshold item in LDS.  A finished output tile pushes what beats the threshold (an LDS ticket per
// query); when a buffer is full the workgroup prunes it to its `window` largest by rank counting (items in registers, handed
// round the wave by v_readlane) and raises the threshold.  Each slice leaves its sorted winners in the workspace;
// scan_merge_kernel orders the slices' winners of a query in LDS.  No global atomics but the error bits.
// Range scan (scan_above_kernel, lshrs_scan_above_*): the same first pass with no selection at all - every (query, live row)
// whose approximate score reaches the query's bar is emitted to flat arrays through one global cursor (lshrs_amd.exact_above).
// Self-join (scan_pairs_kernel, lshrs_scan_pairs_*): the range scan with a block of the stored rows themselves as the queries -
// image and norms built straight from the rows, every unordered pair of live rows multiplied once (a block scans the rows from
// its own first row on, a workgroup from its tile's; diagonal tiles masked lane by lane), one MFMA per step for the one-term
// types, whose image holds no mid term (lshrs_amd.exact_pairs_above).
// k-NN self-join (scan_kernel<E, ALIGNED, SELF = true>, lshrs_scan_knn_*): the top-k scan with a block of the stored rows
// themselves as the queries - image and norms from the rows as in the self-join, one MFMA per step for the one-term types, a
// row never pushed into its own window.  The FULL square, no triangle: a product would have to feed the window of its row side
// too, and those windows (256 rows a pass, per workgroup) do not fit in LDS beside the 64 of the query tile.
// Every layer is written once.  All four kernels: the image and the norms of the queries, whatever they are made of
// (scan_image_kernel<Q>, scan_norm_kernel<Q>, launched by scan_front), the pass - rows in, dot products and norms out
// (scan_pass.inc) - and the head of a finished tile (scan_tile_head).  The selection, the slices' winners and the merge: one
// text for f32 queries and for the rows as queries (scan_kernel, scan_merge_kernel; scan_select on the host).  The two
// emitting kernels: scoring and marking a tile (scan_mark) and writing its hits through the cursor (scan_emit); on the host
// their common refusals and the cursor's reset (scan_emit_begin).  The four plans: scan_rows_geometry and scan_front_bytes.
// The element types of a row, their exact conversions to f32 (a lone element, a dword's elements), the wave's sum and the
// orderable key of a score are not this unit's own: lshrs_rows.h, shared with the rerank (rerank.hip).
// ABI and reference citations: include/lshrs_hip.h, include/lshrs_knn.h.  Design notes, the epsilon derivation and the roof: DESIGN.md.
#include "lshrs_rows.h"
#include "lshrs_knn.h"

#include <initializer_list>
#include <type_traits>

using namespace lshrs;

namespace {
constexpr int kScanThreads = 256;
constexpr int kScanWaves = 4;
constexpr int kScanQTile = 64;        // queries per workgroup (two 32-column B blocks)
constexpr int kScanKChunk = 64;       // k per staged B chunk (four MFMA steps of 16)
constexpr int kScanPassRows = 256;    // rows per workgroup pass: 64 per wave, two 32-row tiles
constexpr int kScanMaxWindow = 128;
constexpr int kScanChunkBytes = kScanQTile * kScanKChunk * 2 * 2;   // both terms: 16 KiB
constexpr int kScanMaxDim = 16384;
constexpr int kScanMergeItems = 8192; // slices * window a merge workgroup sorts in LDS (64 KiB)

// per element type (lshrs_rows.h: the tags, RowT<E>, the conversions): bf16 terms per element (bf16, int8 and e4m3fn are exact
// in bf16; f16 and f32 enter as two), and what a lane's 32 elements of a chunk are in 16-B vectors and need in alignment
template <typename E> struct ScanElem {
  using T = RowT<E>;
  static constexpr int kTerms = (std::is_same_v<E, float> || std::is_same_v<E, F16>) ? 2 : 1;
  static constexpr int kVecs = 8 / kRowPerDword<E>, kAlign = 4 * kRowPerDword<E>;
};

template <typename E> struct ScanRaw { u32x4 v[ScanElem<E>::kVecs]; };   // 32 elements as they lie in memory

// an item of the selection = {asc_key(score), ~row}: larger = better score, then lower row.  0 = no item (every real key is
// above 0).

// ------------------------------------------------------------------------------------------
// queries -> B fragments and norms, one text for both kinds of query: rows of f32 (the `float` instantiation: src = the
// queries, ld = dim, row_ids = nullptr, qb = 0, qn = q) and a block [qb, qb + qn) of the stored rows themselves (the
// self-join: src = the corpus, its ld and row_ids).  An element is converted to f32 exactly, then split and summed in one
// order whatever it was, so an approximate score of the self-join is the one the same rows get as f32 queries.
// ------------------------------------------------------------------------------------------
// Workspace image: [qtile][chunk][term < kTerms][step s][column block cb][lane] x 16 bytes; lane (c = l & 31, h = l >> 5)
// holds query qtile * 64 + cb * 32 + c at k = chunk * 64 + 32 h + 8 s + j, j = 0 .. 7.  Zero beyond qn and dim, and for a
// dead row.  A one-term element is exact in bf16: its mid term is zero and the image holds hi only (half the bytes).
template <typename E>
__global__ __launch_bounds__(kScanThreads) void scan_image_kernel(const typename ScanElem<E>::T* __restrict__ src, int64_t ld,
                                                                  int dim, const int64_t* __restrict__ row_ids, int64_t qb, int qn,
                                                                  int nchunks, u32x4* __restrict__ image) {
  constexpr int kBTerms = ScanElem<E>::kTerms;
  const int chunk = blockIdx.x, qtile = blockIdx.y;
  u32x4* out = image + ((int64_t)qtile * nchunks + chunk) * (kBTerms * 512);
  for (int f = threadIdx.x; f < 512; f += kScanThreads) {
    const int lane = f & 63, cb = (f >> 6) & 1, s = f >> 7;
    const int qi = qtile * kScanQTile + cb * 32 + (lane & 31);
    const bool ok = qi < qn && (row_ids == nullptr || row_ids[qb + qi] >= 0);
    const typename ScanElem<E>::T* row = src + (qb + (ok ? qi : 0)) * ld;
    const int kbase = chunk * kScanKChunk + 32 * (lane >> 5) + 8 * s;
    uint32_t hb[8], mb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = kbase + j;
      const float v = (ok && k < dim) ? row_elem_f32(E{}, row[k]) : 0.f;
      const uint32_t b = __float_as_uint(v) & 0xffff0000u;
      hb[j] = b >> 16;
      mb[j] = __float_as_uint(v - __uint_as_float(b)) >> 16;
    }
    u32x4 hi, mid;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      hi[d] = hb[2 * d] | (hb[2 * d + 1] << 16);
      mid[d] = mb[2 * d] | (mb[2 * d + 1] << 16);
    }
    out[((0 * 4 + s) * 2 + cb) * 64 + lane] = hi;
    if constexpr (kBTerms == 2) out[((1 * 4 + s) * 2 + cb) * 64 + lane] = mid;
  }
}

// ||q|| in f32, one wave per query; 1 for a padding query of the last tile and for a dead row (neither sets an error bit, and
// nothing reaches the bar the kernels give them); err |= 4 for a live query of zero norm
template <typename E>
__global__ __launch_bounds__(kScanThreads) void scan_norm_kernel(const typename ScanElem<E>::T* __restrict__ src, int64_t ld,
                                                                 int dim, const int64_t* __restrict__ row_ids, int64_t qb, int qn,
                                                                 int qpad, float* __restrict__ qnorm, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int qi = blockIdx.x * kScanWaves + (threadIdx.x >> 6);
  if (qi >= qpad) return;
  const bool ok = qi < qn && (row_ids == nullptr || row_ids[qb + qi] >= 0);
  float ss = 0.f;
  if (ok) {
    const typename ScanElem<E>::T* row = src + (qb + qi) * ld;
    for (int k = lane; k < dim; k += 64) {
      const float v = row_elem_f32(E{}, row[k]);
      ss = __builtin_fmaf(v, v, ss);
    }
  }
  ss = wave_sum(ss);
  if (lane == 0) {
    const float n = ok ? sqrtf(ss) : 1.f;
    qnorm[qi] = n;
    if (n == 0.f && err != nullptr) atomicOr(err, 4);
  }
}

// ------------------------------------------------------------------------------------------
// a lane's 32 elements of one row of one chunk, as they lie in memory
// ------------------------------------------------------------------------------------------
template <typename E>
__device__ __forceinline__ ScanRaw<E> scan_load_vec(const typename ScanElem<E>::T* p) {
  ScanRaw<E> r;
  const u32x4* v = reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int i = 0; i < ScanElem<E>::kVecs; ++i) r.v[i] = v[i];
  return r;
}

// the same image built element by element: any address and stride, nothing read at k >= dim (zero bits are 0.0 in all five types)
template <typename E>
__device__ __forceinline__ ScanRaw<E> scan_load_elems(const typename ScanElem<E>::T* row, int k0, int dim) {
  using T = typename ScanElem<E>::T;
  constexpr int kPer = kRowPerDword<E>;
  ScanRaw<E> r;
#pragma unroll
  for (int i = 0; i < ScanElem<E>::kVecs; ++i)
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint32_t w = 0;
#pragma unroll
      for (int e = 0; e < kPer; ++e) {
        const int k = k0 + (i * 4 + d) * kPer + e;
        if (k < dim) {
          uint32_t bits;
          if constexpr (sizeof(T) == 4) bits = __float_as_uint(row[k]);
          else bits = (uint32_t)row[k] & ((1u << (8 * sizeof(T) % 32)) - 1u);
          w |= bits << (8 * (int)sizeof(T) * e % 32);
        }
      }
      r.v[i][d] = w;
    }
  return r;
}

// the eight elements of MFMA step s as f32 (exact): the 8 / kPer dwords behind them, each unpacked in memory order
template <typename E>
__device__ __forceinline__ void scan_elems8(const ScanRaw<E>& r, int s, float (&x)[8]) {
  constexpr int kPer = kRowPerDword<E>, kDwords = 8 / kPer;
#pragma unroll
  for (int d = 0; d < kDwords; ++d) {
    const int w = s * kDwords + d;                    // the dword among the 32 elements'
    float e[kPer];
    row_unpack(E{}, r.v[w >> 2][w & 3], e);
#pragma unroll
    for (int j = 0; j < kPer; ++j) x[kPer * d + j] = e[j];
  }
}

// raw elements -> the A fragments of the four steps (hi; mid for the two-term types) and += ||x||^2
template <typename E>
__device__ __forceinline__ void scan_fragments(const ScanRaw<E>& r, u32x4 (&hi)[4], u32x4 (&mid)[4], float& nn) {
  if constexpr (std::is_same_v<E, Bf16>) {          // (the stored bits ARE the fragment)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      hi[s] = r.v[s];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        float e[2];
        row_unpack(Bf16{}, r.v[s][d], e);
        nn = __builtin_fmaf(e[0], e[0], nn);
        nn = __builtin_fmaf(e[1], e[1], nn);
      }
    }
  } else {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float x[8];
      scan_elems8<E>(r, s, x);
      uint32_t hb[8], mb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        nn = __builtin_fmaf(x[j], x[j], nn);
        const uint32_t b = __float_as_uint(x[j]) & 0xffff0000u;
        hb[j] = b;
        if constexpr (ScanElem<E>::kTerms == 2) mb[j] = __float_as_uint(x[j] - __uint_as_float(b)) & 0xffff0000u;
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        hi[s][d] = (hb[2 * d] >> 16) | hb[2 * d + 1];
        if constexpr (ScanElem<E>::kTerms == 2) mid[s][d] = (mb[2 * d] >> 16) | mb[2 * d + 1];
      }
    }
  }
}

// One query's buffer to its `window` largest items, sorted descending, by one wave.  The items go to registers (NI = cap / 64 per
// lane); every lane ranks its own against all of them, which the wave hands round lane by lane (v_readlane: no LDS round trip
// per item); the kept ones go to their ranks.  Items are distinct (their rows are), so the ranks are a permutation.
template <int NI>
__device__ __forceinline__ void scan_prune_n(uint64_t* buf, int n, int window, uint64_t* thr, int* cnt, int lane) {
  uint32_t lo[NI], hi[NI];
  uint64_t mine[NI];
  int rank[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int idx = lane + 64 * j;
    mine[j] = idx < n ? buf[idx] : 0ull;
    lo[j] = (uint32_t)mine[j];
    hi[j] = (uint32_t)(mine[j] >> 32);
    rank[j] = 0;
  }
#pragma unroll
  for (int c = 0; c < NI; ++c) {
    if (64 * c >= n) break;                            // (uniform: n is the same in every lane)
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const uint64_t v = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi[c], i) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)lo[c], i);
#pragma unroll
      for (int j = 0; j < NI; ++j) rank[j] += v > mine[j] ? 1 : 0;      // (an empty place is 0: it outranks nothing)
    }
  }
#pragma unroll
  for (int j = 0; j < NI; ++j)
    if (mine[j] != 0ull && rank[j] < window) {
      buf[rank[j]] = mine[j];
      if (rank[j] == window - 1) *thr = mine[j];
    }
  if (lane == 0) *cnt = min(n, window);
}

// `all`: sort even when nothing has to go (the slice's last call).  cap is 64, 128 or 256 (scan_plan).
__device__ __forceinline__ void scan_prune(uint64_t* buf, int cap, int window, uint64_t* thr, int* cnt, int lane, bool all) {
  const int n = min(*cnt, cap);
  if (n <= window && !all) return;
  if (cap <= 64) scan_prune_n<1>(buf, n, window, thr, cnt, lane);
  else if (cap <= 128) scan_prune_n<2>(buf, n, window, thr, cnt, lane);
  else scan_prune_n<4>(buf, n, window, thr, cnt, lane);
}

// The head of a finished 32-row tile, for all three kernels: nn is this lane's half of its row's ||x||^2 (scan_pass.inc).
// Returns the row's norm (lane l and lane l ^ 32 hold row l & 31), sets err |= 1 for a live row of zero norm and leaves the
// live rows as a mask (bit rr = row rr of the tile).
__device__ __forceinline__ float scan_tile_head(float nn, bool live, int h, int32_t* __restrict__ err, uint32_t& livemask) {
  nn += __shfl_xor(nn, 32);
  const float xn = sqrtf(nn);
  if (live && xn == 0.f && h == 0 && err != nullptr) atomicOr(err, 1);
  livemask = (uint32_t)__ballot(live);
  return xn;
}

// ------------------------------------------------------------------------------------------
// the scan.  grid (slices, query tiles); dynamic LDS: B chunk | items [64][cap] | threshold [64] | count [64]
// SELF (the k-NN self-join): the queries are the block [qb, qb + q) of the stored rows; the image holds the rows' own terms
// (kBTerms = 1 for the one-term types: no mid MFMA, scan_pass.inc), a dead row of the block is nobody's query, and no row
// enters its own window (by position).  Every block scans all of [0, m).
// ------------------------------------------------------------------------------------------
// SELF, workgroups per CU.  At two the SELF instantiations fill 256 VGPRs and spill 12 to 36 bytes a lane to scratch, as seven of
// the ten others do; at one - the precedent of kScanPairsPerCu - the accumulators live in AGPRs and nothing is spilled.  Two was
// chosen on the measurement (200 000 x 768, k = 10, the first pass): 202 against 290 ms for bf16 rows, 363 against 507 ms for
// f32.  A selecting workgroup waits at more barriers than an emitting one (the ticket loop, the prunes), and at one per CU the
// CU has nothing to do meanwhile (k-NN self-join).
constexpr int kScanKnnPerCu = 2;

template <typename E, bool ALIGNED, bool SELF = false>
__global__ __launch_bounds__(kScanThreads, SELF ? kScanKnnPerCu : 2) void scan_kernel(const typename ScanElem<E>::T* __restrict__ corpus, int64_t m,
                                                            int64_t ldc, int dim, const int64_t* __restrict__ row_ids,
                                                            const u32x4* __restrict__ image, const float* __restrict__ qnorm,
                                                            int q, int window, int cap, int64_t rows_per_slice,
                                                            uint64_t* __restrict__ parts, int32_t* __restrict__ err, int64_t qb) {
  using T = typename ScanElem<E>::T;
  constexpr bool kTwo = ScanElem<E>::kTerms == 2;
  constexpr int kBTerms = SELF ? ScanElem<E>::kTerms : 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char scan_lds[];
  u32x4* bl = reinterpret_cast<u32x4*>(scan_lds);
  uint64_t* items = reinterpret_cast<uint64_t*>(scan_lds + kScanChunkBytes);
  uint64_t* thr = items + (size_t)kScanQTile * cap;
  int* cnt = reinterpret_cast<int*>(thr + kScanQTile);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int slice = blockIdx.x, slices = gridDim.x, qtile = blockIdx.y;
  const int nchunks = (dim + kScanKChunk - 1) / kScanKChunk;
  const int64_t row_begin = (int64_t)slice * rows_per_slice;
  const int64_t row_end = min(m, row_begin + rows_per_slice);
  const u32x4* bimg = image + (int64_t)qtile * nchunks * (kBTerms * 512);

  if (tid < kScanQTile) {
    thr[tid] = 0ull;
    cnt[tid] = 0;
  }
  float qn[2];
  bool qok[2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int qi = qtile * kScanQTile + cb * 32 + r;
    qok[cb] = qi < q;
    if constexpr (SELF) qok[cb] = qok[cb] && (row_ids == nullptr || row_ids[qb + qi] >= 0);
    qn[cb] = qnorm[qi];                   // (padded to whole tiles)
  }
  __syncthreads();

  for (int64_t base = row_begin; base < row_end; base += kScanPassRows) {
    bool live[2];
    int64_t row0[2];
    f32x16 acc[2][2];
    float nn[2];
#include "scan_pass.inc"

    // the finished 256 x 64 tile: acc[t][cb][i] is row (i & 3) + 8 (i >> 2) + 4 h of tile t, query cb * 32 + r
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      uint32_t livemask;
      const float xn = scan_tile_head(nn[t], live[t], h, err, livemask);
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int qc = cb * 32 + r;
        uint64_t* buf = items + (size_t)qc * cap;
        // (the scores replace the dot products in the accumulator; an item is rebuilt from its score where it is needed)
        const uint32_t rowlo = 0xffffffffu - (uint32_t)(row0[t] + 4 * h);
        uint32_t pend = 0;
        uint64_t bar = thr[qc];
        // SELF: the offset in this tile of the lane's own query row (qb + qtile * 64 + cb * 32 + r), -1 where it is not in it
        int own = -1;
        if constexpr (SELF) {
          const int64_t ahead = qb + (int64_t)qtile * kScanQTile + cb * 32 - row0[t];     // (uniform)
          own = (ahead < -32 || ahead > 32) ? -1 : (int)ahead + r;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int rr = (i & 3) + 8 * (i >> 2) + 4 * h;
          const float rn = __shfl(xn, rr);
          const float sc = acc[t][cb][i] / (rn * qn[cb]);
          acc[t][cb][i] = sc;
          const uint64_t it = key_item(asc_key(sc), rowlo - (uint32_t)((i & 3) + 8 * (i >> 2)));
          if (qok[cb] && ((livemask >> rr) & 1u) && (!SELF || rr != own) && sc == sc && it > bar) pend |= 1u << i;
        }
        for (;;) {
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (pend & (1u << i)) {
              const int pos = atomicAdd(&cnt[qc], 1);
              if (pos < cap) {
                buf[pos] = key_item(asc_key(acc[t][cb][i]), rowlo - (uint32_t)((i & 3) + 8 * (i >> 2)));
                pend &= ~(1u << i);
              }
            }
          if (!__syncthreads_or(pend != 0)) break;
          // a buffer overflowed: every wave prunes its share of the queries, then those left out try again
          for (int qq = wave; qq < kScanQTile; qq += kScanWaves)
            scan_prune(items + (size_t)qq * cap, cap, window, thr + qq, cnt + qq, lane, false);
          __syncthreads();
          bar = thr[qc];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const uint64_t it = key_item(asc_key(acc[t][cb][i]), rowlo - (uint32_t)((i & 3) + 8 * (i >> 2)));
            if (!(it > bar)) pend &= ~(1u << i);
          }
        }
      }
    }
  }

  // the slice's winners of every query, sorted, zero items behind them
  __syncthreads();
  for (int qq = wave; qq < kScanQTile; qq += kScanWaves) {
    const int qi = qtile * kScanQTile + qq;
    if (qi >= q) continue;
    uint64_t* buf = items + (size_t)qq * cap;
    scan_prune(buf, cap, window, thr + qq, cnt + qq, lane, true);
    const int kept = cnt[qq];
    uint64_t* out = parts + ((int64_t)qi * slices + slice) * window;
    for (int j = lane; j < window; j += 64) out[j] = j < kept ? buf[j] : 0ull;
  }
}

// ------------------------------------------------------------------------------------------
// one pass of a workgroup as a function, for scan_above_kernel: the text of scan_pass.inc (which says what it takes and leaves).
// scan_kernel includes the same text inline instead of calling this: the call moved its register allocation (spills and
// scratch of seven of its ten instantiations - measured in commit f6cea70, "Exact range search: every stored vector at or above a
// cosine threshold"), while the included text compiles to the code the kernel had with the loop written out in it.
// kBTerms: the terms of the image (scan_pass.inc) - 2 for f32 queries, ScanElem<E>::kTerms for the self-join.
// ------------------------------------------------------------------------------------------
template <typename E, bool ALIGNED, int kBTerms = 2>
__device__ __forceinline__ void scan_pass(const typename ScanElem<E>::T* __restrict__ corpus, int64_t ldc, int dim, int nchunks,
                                          const int64_t* __restrict__ row_ids, const u32x4* __restrict__ bimg, u32x4* bl,
                                          int64_t base, int64_t row_begin, int64_t row_end, int tid, bool (&live)[2],
                                          int64_t (&row0)[2], f32x16 (&acc)[2][2], float (&nn)[2]) {
  using T = typename ScanElem<E>::T;
  constexpr bool kTwo = ScanElem<E>::kTerms == 2;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
#include "scan_pass.inc"
}

// ------------------------------------------------------------------------------------------
// what the two emitting kernels (range scan, self-join) do with a finished 32-row tile
// ------------------------------------------------------------------------------------------
// One column block: the dot products acc[i] (row rr = (i & 3) + 8 (i >> 2) + 4 h of the tile, this lane's query) become the
// approximate scores, in place; returns bit i for a live row whose score reaches `bar` (NaN reaches none) and - GAP, the
// self-join's diagonal tiles - whose offset in the tile lies beyond `gap`.
template <bool GAP>
__device__ __forceinline__ uint32_t scan_mark(f32x16& acc, float xn, float qn, float bar, uint32_t livemask, int h, int gap) {
  uint32_t hits = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int rr = (i & 3) + 8 * (i >> 2) + 4 * h;
    const float rn = __shfl(xn, rr);
    const float sc = acc[i] / (rn * qn);
    acc[i] = sc;
    if (((livemask >> rr) & 1u) && (!GAP || rr > gap) && sc >= bar) hits |= 1u << i;
  }
  return hits;
}

// The hits of a wave's tile (bit cb * 16 + i of `hits`) leave through the global cursor: the wave reserves their slots with
// one 64-bit atomicAdd on `total` (which counts every hit, also those beyond `capacity`: the caller then knows what to
// allocate) and writes those that fit - first column q0 / q1 (the lane's query of column block 0 / 1), the row, the score.
template <typename A>
__device__ __forceinline__ void scan_emit(uint32_t hits, int lane, int h, int64_t capacity, unsigned long long* __restrict__ total,
                                          A* __restrict__ out_q, A q0, A q1, int64_t* __restrict__ out_row, int64_t row0,
                                          float* __restrict__ out_approx, const f32x16 (&acc)[2]) {
  if (__ballot(hits != 0) == 0ull) return;          // (the common case: nothing of this tile reaches a bar)
  const int mine = __popc(hits);
  int incl = mine;                      // inclusive prefix sum of the lanes' hit counts
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  unsigned long long first = 0ull;
  if (lane == 63) first = atomicAdd(total, (unsigned long long)incl);       // (lane 63's sum is the wave's)
  int64_t slot = (int64_t)__shfl(first, 63) + (incl - mine);
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (hits & (1u << (cb * 16 + i))) {
        if (slot < capacity) {
          out_q[slot] = cb ? q1 : q0;
          out_row[slot] = row0 + (i & 3) + 8 * (i >> 2) + 4 * h;
          out_approx[slot] = acc[cb][i];
        }
        ++slot;
      }
}

// ------------------------------------------------------------------------------------------
// range scan: the same grid, image and pass; instead of a window per query, EVERY (query, live row) whose approximate score
// reaches the query's bar goes out (scan_mark, scan_emit).  Order unspecified.  LDS: the B chunk only.
// ------------------------------------------------------------------------------------------
template <typename E, bool ALIGNED>
__global__ __launch_bounds__(kScanThreads, 2) void scan_above_kernel(const typename ScanElem<E>::T* __restrict__ corpus, int64_t m,
                                                                  int64_t ldc, int dim, const int64_t* __restrict__ row_ids,
                                                                  const u32x4* __restrict__ image,
                                                                  const float* __restrict__ qnorm, const float* __restrict__ bars,
                                                                  int q, int64_t rows_per_slice, int64_t capacity,
                                                                  int32_t* __restrict__ out_query, int64_t* __restrict__ out_row,
                                                                  float* __restrict__ out_approx,
                                                                  unsigned long long* __restrict__ total,
                                                                  int32_t* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) unsigned char scan_lds[];
  u32x4* bl = reinterpret_cast<u32x4*>(scan_lds);

  const int tid = threadIdx.x, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int slice = blockIdx.x, qtile = blockIdx.y;
  const int nchunks = (dim + kScanKChunk - 1) / kScanKChunk;
  const int64_t row_begin = (int64_t)slice * rows_per_slice;
  const int64_t row_end = min(m, row_begin + rows_per_slice);
  const u32x4* bimg = image + (int64_t)qtile * nchunks * (kScanChunkBytes / 16);

  float qn[2], bar[2];
  int qi[2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    qi[cb] = qtile * kScanQTile + cb * 32 + r;
    qn[cb] = qnorm[qi[cb]];               // (padded to whole tiles)
    bar[cb] = qi[cb] < q ? bars[qi[cb]] : __builtin_inff();   // (nothing reaches the bar of a padding query, NaN reaches none)
  }

  for (int64_t base = row_begin; base < row_end; base += kScanPassRows) {
    bool live[2];
    int64_t row0[2];
    f32x16 acc[2][2];
    float nn[2];
    scan_pass<E, ALIGNED>(corpus, ldc, dim, nchunks, row_ids, bimg, bl, base, row_begin, row_end, tid, live, row0, acc, nn);

    // the finished 256 x 64 tile: acc[t][cb][i] is row (i & 3) + 8 (i >> 2) + 4 h of tile t, query cb * 32 + r
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      uint32_t livemask;
      const float xn = scan_tile_head(nn[t], live[t], h, err, livemask);
      uint32_t hits = 0;                  // bit cb * 16 + i
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) hits |= scan_mark<false>(acc[t][cb], xn, qn[cb], bar[cb], livemask, h, 0) << (cb * 16);
      scan_emit(hits, lane, h, capacity, total, out_query, qi[0], qi[1], out_row, row0[t], out_approx, acc[t]);
    }
  }
}

// ------------------------------------------------------------------------------------------
// self-join (scan_pairs_kernel, lshrs_scan_pairs_*): the queries are a block [qb, qb + qn) of the stored rows themselves.
// The image and the norms come straight from the rows, by the kernels that make them of f32 queries (scan_image_kernel,
// scan_norm_kernel), and a tile is scored and emitted by the range scan's own functions - so an approximate score is the one
// lshrs_scan_above_* gives the same rows as f32 queries.  The image of one-term rows holds no mid term, and the pass issues
// no MFMA for it (scan_pass.inc, kBTerms = 1).  A dead row is a padding query to the image and the norms; here it gets a bar
// of +inf.
// ------------------------------------------------------------------------------------------
// One workgroup per CU: at two, this kernel - like scan_above_kernel - fills 256 VGPRs and spills a few loop invariants to
// scratch; at one the accumulators live in AGPRs and nothing is spilled (self-join).
constexpr int kScanPairsPerCu = 1;

// grid (slices of the rows [qb, m), query tiles of the block).  A pair (a, b) goes out
// when a is a live row of the tile, b a live row with b > a (by position: every unordered pair once, no row against itself)
// and approx >= bar.  The workgroup starts at the pass that holds its tile's first row: no pass whose rows all lie before it.
template <typename E, bool ALIGNED>
__global__ __launch_bounds__(kScanThreads, kScanPairsPerCu) void scan_pairs_kernel(const typename ScanElem<E>::T* __restrict__ corpus, int64_t m,
                                                                  int64_t ldc, int dim, const int64_t* __restrict__ row_ids,
                                                                  const u32x4* __restrict__ image,
                                                                  const float* __restrict__ qnorm, float bar_all, int64_t qb,
                                                                  int qn, int64_t rows_per_slice, int64_t capacity,
                                                                  int64_t* __restrict__ out_a, int64_t* __restrict__ out_b,
                                                                  float* __restrict__ out_approx,
                                                                  unsigned long long* __restrict__ total,
                                                                  int32_t* __restrict__ err) {
  constexpr int kBTerms = ScanElem<E>::kTerms;
  extern __shared__ __attribute__((aligned(16))) unsigned char scan_lds[];
  u32x4* bl = reinterpret_cast<u32x4*>(scan_lds);

  const int tid = threadIdx.x, lane = tid & 63;
  const int r = lane & 31, h = lane >> 5;
  const int slice = blockIdx.x, qtile = blockIdx.y;
  const int nchunks = (dim + kScanKChunk - 1) / kScanKChunk;
  const int64_t row_begin = qb + (int64_t)slice * rows_per_slice;
  const int64_t row_end = min(m, row_begin + rows_per_slice);
  const int64_t tile_first = qb + (int64_t)qtile * kScanQTile;
  const int64_t first_base = tile_first <= row_begin ? row_begin
                                                     : row_begin + (tile_first - row_begin) / kScanPassRows * kScanPassRows;
  if (first_base >= row_end) return;      // (the whole slice lies before the tile; uniform, nothing was synchronised yet)
  const u32x4* bimg = image + (int64_t)qtile * nchunks * (kBTerms * 512);

  // the lane's query rows are tile_first + cb * 32 + r; which of them exist and are live, as wave masks (kept out of the
  // vector registers, as everything here that outlives a pass is: the pass needs them all)
  float qnv[2];
  uint64_t qlive[2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int qi = qtile * kScanQTile + cb * 32 + r;
    qnv[cb] = qnorm[qi];                  // (padded to whole tiles)
    qlive[cb] = __ballot(qi < qn && (row_ids == nullptr || row_ids[qb + qi] >= 0));
  }

  for (int64_t base = first_base; base < row_end; base += kScanPassRows) {
    bool live[2];
    int64_t row0[2];
    f32x16 acc[2][2];
    float nn[2];
    scan_pass<E, ALIGNED, kBTerms>(corpus, ldc, dim, nchunks, row_ids, bimg, bl, base, row_begin, row_end, tid, live, row0, acc,
                                   nn);

    // the finished 256 x 64 tile: acc[t][cb][i] is row (i & 3) + 8 (i >> 2) + 4 h of tile t, query row cb * 32 + r of the tile
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      uint32_t livemask;
      const float xn = scan_tile_head(nn[t], live[t], h, err, livemask);
      uint32_t hits = 0;                  // bit cb * 16 + i
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        // nothing reaches the bar of a dead or a padding row (NaN reaches none); rows of this tile at or before the lane's
        // query row are not its partners: b > a <=> the row's offset in the tile > gap (diagonal tiles; else -1: all are)
        const float bar = ((qlive[cb] >> lane) & 1ull) ? bar_all : __builtin_inff();
        const int64_t ahead = tile_first + cb * 32 - row0[t];          // (uniform)
        const int gap = ahead < -32 ? -1 : ahead > 32 ? 32 : (int)ahead + r;
        hits |= scan_mark<true>(acc[t][cb], xn, qnv[cb], bar, livemask, h, gap) << (cb * 16);
      }
      scan_emit(hits, lane, h, capacity, total, out_a, tile_first + r, tile_first + 32 + r, out_b, row0[t], out_approx, acc[t]);
    }
  }
}

// ------------------------------------------------------------------------------------------
// one workgroup per query: the slices' winners into LDS, bitonic network descending, the first `window` out
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void scan_merge_kernel(const uint64_t* __restrict__ parts, int n, int npad, int window,
                                                                  int64_t* __restrict__ out_rows, float* __restrict__ out_approx,
                                                                  int32_t* __restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) uint64_t merge_items[];
  __shared__ int total;
  const int qi = blockIdx.x;
  const uint64_t* src = parts + (int64_t)qi * n;
  if (threadIdx.x == 0) total = 0;
  for (int t = threadIdx.x; t < npad; t += kScanThreads) merge_items[t] = t < n ? src[t] : 0ull;
  __syncthreads();
  for (int size = 2; size <= npad; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (npad >> 1); t += kScanThreads) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const uint64_t a = merge_items[lo], b = merge_items[hi];
        if ((a < b) == up) {
          merge_items[lo] = b;
          merge_items[hi] = a;
        }
      }
      __syncthreads();
    }
  int have = 0;
  for (int t = threadIdx.x; t < window; t += kScanThreads) {     // (window <= n <= npad)
    const uint64_t v = merge_items[t];
    have += v != 0ull ? 1 : 0;
    out_rows[(int64_t)qi * window + t] = v != 0ull ? (int64_t)(0xffffffffu - (uint32_t)v) : -1;
    out_approx[(int64_t)qi * window + t] = v != 0ull ? asc_unkey((uint32_t)(v >> 32)) : -__builtin_inff();
  }
  if (have) atomicAdd(&total, have);
  __syncthreads();
  if (threadIdx.x == 0) out_count[qi] = total;
}

// ------------------------------------------------------------------------------------------
// host side: geometry of a launch, shared by the workspace size and the entries
// ------------------------------------------------------------------------------------------
struct ScanPlan {
  int qtiles, nchunks, slices, cap;
  int64_t rows_per_slice;
  int64_t image_bytes, qnorm_bytes, parts_bytes;
};

// slices: one round of the workgroups that are resident at a time - 256 CUs, two per CU while their LDS (`lds` bytes) fits twice
// into the CU's 160 KiB, else one - over all query tiles: a second, part-filled round costs a whole slice's time.  At least
// 1024 rows each, and no more than `limit` (scan_kernel: what one merge workgroup sorts in LDS).  `per_cu`: the workgroups per CU
// the kernel is compiled for (its __launch_bounds__).
inline void scan_slices(int64_t m, int qtiles, int64_t lds, int64_t limit, int64_t& rows_per_slice, int& slices, int per_cu = 2) {
  const int64_t resident = 256 * (per_cu >= 2 && 2 * lds <= 160 * 1024 ? 2 : 1);
  const int64_t qt = qtiles > 0 ? qtiles : 1;
  int64_t want = resident / qt;
  const int64_t by_rows = (m + 1023) / 1024;
  if (want > by_rows) want = by_rows;
  if (want > limit) want = limit;
  if (want < 1) want = 1;
  const int64_t passes = (m + kScanPassRows - 1) / kScanPassRows;
  const int64_t rps = (passes + want - 1) / want * kScanPassRows;
  rows_per_slice = rps;
  slices = (int)((m + rps - 1) / rps);
}

// what all three plans share: the ranges of m and dim and the chunks of k ...
inline int scan_rows_geometry(int64_t m, int32_t dim, ScanPlan& p) {
  if (m <= 0 || dim <= 0) return LSHRS_E_BADARG;
  if (dim > kScanMaxDim || m > 0x7fffffffLL) return LSHRS_E_TOOLARGE;
  p.nchunks = (dim + kScanKChunk - 1) / kScanKChunk;
  return 0;
}

// ... and the head of the workspace, for `qtiles` tiles of queries: the image (at two terms, whatever the queries hold: the
// workspace's size knows no element type) and the norms
inline int scan_front_bytes(int64_t qtiles, ScanPlan& p) {
  if (qtiles > 65535) return LSHRS_E_TOOLARGE;
  p.qtiles = (int)qtiles;
  p.image_bytes = qtiles * p.nchunks * kScanChunkBytes;
  p.qnorm_bytes = qtiles * kScanQTile * (int64_t)sizeof(float);
  return 0;
}

inline int scan_geometry(int32_t q, int64_t m, int32_t dim, ScanPlan& p) {
  if (q < 0) return LSHRS_E_BADARG;
  const int bad = scan_rows_geometry(m, dim, p);
  return bad ? bad : scan_front_bytes((q + kScanQTile - 1) / kScanQTile, p);
}

// the selection's window -> the per-query buffer (p.cap), and the LDS of a scan_kernel workgroup with it
inline int scan_window_cap(int32_t window, ScanPlan& p) {
  if (window <= 0 || window > kScanMaxWindow) return LSHRS_E_BADARG;
  p.cap = 64;
  while (p.cap < 2 * window) p.cap <<= 1;
  return 0;
}

inline int64_t scan_select_lds(int cap) { return (int64_t)kScanChunkBytes + (int64_t)kScanQTile * cap * 8 + kScanQTile * 12; }

inline int scan_plan(int32_t q, int64_t m, int32_t dim, int32_t window, ScanPlan& p) {
  int bad = scan_window_cap(window, p);
  if (bad) return bad;
  bad = scan_geometry(q, m, dim, p);
  if (bad) return bad;
  scan_slices(m, p.qtiles, scan_select_lds(p.cap), kScanMergeItems / window, p.rows_per_slice, p.slices);
  p.parts_bytes = (int64_t)q * p.slices * window * (int64_t)sizeof(uint64_t);
  return 0;
}

// range scan: no merge limit, residency from scan_above_kernel's own LDS (the B chunk)
inline int scan_above_plan(int32_t q, int64_t m, int32_t dim, ScanPlan& p) {
  const int bad = scan_geometry(q, m, dim, p);
  if (bad) return bad;
  p.cap = 0;
  scan_slices(m, p.qtiles, kScanChunkBytes, INT64_MAX, p.rows_per_slice, p.slices);
  p.parts_bytes = 0;
  return 0;
}

// self-join: the rows are taken as queries a block at a time.  The plan's block (p.qtiles): 128 query tiles - with the rows in
// two slices, one round of the 256 workgroups resident at a time, every slice's rows read by 128 of them in step - fewer where
// the image of that many would pass 256 MiB or the rows end.  A caller's block (a multiple of 64) is taken as it is.  The
// slices are each block's own (scan_pairs).
constexpr int kScanPairsBlock = 8192;
constexpr int64_t kScanPairsImageBytes = 256ll << 20;

inline int scan_pairs_plan(int64_t m, int32_t dim, int32_t qblock, ScanPlan& p) {
  if (qblock < 0 || qblock % kScanQTile) return LSHRS_E_BADARG;
  const int bad = scan_rows_geometry(m, dim, p);
  if (bad) return bad;
  int64_t tiles = qblock / kScanQTile;
  if (qblock == 0) {
    const int64_t tile_bytes = (int64_t)p.nchunks * kScanChunkBytes;
    tiles = kScanPairsBlock / kScanQTile;
    if (tiles > kScanPairsImageBytes / tile_bytes) tiles = kScanPairsImageBytes / tile_bytes;     // (at least 64: 4 MiB a tile)
    if (tiles > (m + kScanQTile - 1) / kScanQTile) tiles = (m + kScanQTile - 1) / kScanQTile;
  }
  p.cap = p.slices = 0;
  p.rows_per_slice = p.parts_bytes = 0;
  return scan_front_bytes(tiles, p);
}

// k-NN self-join: the rows [q_begin, q_begin + q_count) as queries in blocks as the self-join plans them, the range in place of
// the rows (scan_pairs_plan of q_count rows; a caller's block is taken as it is).  Every block scans all m rows in slices of
// its own (scan_knn_block); the slices' winners of the workspace are those of the block that has most: the first - a full one,
// or the only one - or the last, which has fewer rows and may have more slices.
inline void scan_knn_block(int64_t m, int32_t qn, int32_t window, ScanPlan& p) {
  p.qtiles = (qn + kScanQTile - 1) / kScanQTile;
  scan_slices(m, p.qtiles, scan_select_lds(p.cap), kScanMergeItems / window, p.rows_per_slice, p.slices, kScanKnnPerCu);
  p.parts_bytes = (int64_t)qn * p.slices * window * (int64_t)sizeof(uint64_t);
}

inline int scan_knn_plan(int32_t q_count, int64_t m, int32_t dim, int32_t window, int32_t qblock, ScanPlan& p) {
  if (q_count < 0 || q_count > m) return LSHRS_E_BADARG;
  int bad = scan_window_cap(window, p);
  if (bad) return bad;
  const int cap = p.cap;
  bad = scan_pairs_plan(q_count > 0 ? q_count : 1, dim, qblock, p);
  if (bad) return bad;
  bad = scan_rows_geometry(m, dim, p);
  if (bad) return bad;
  p.cap = cap;
  const int block_tiles = p.qtiles;
  const int64_t block_rows = (int64_t)block_tiles * kScanQTile;
  const int32_t first = (int32_t)(q_count < block_rows ? q_count : block_rows), last = (int32_t)(q_count % block_rows);
  int64_t parts = 0;
  for (const int32_t qn : {first, last})
    if (qn > 0) {
      scan_knn_block(m, qn, window, p);
      if (p.parts_bytes > parts) parts = p.parts_bytes;
    }
  p.qtiles = block_tiles;           // (image_bytes and qnorm_bytes are the block's: scan_front_bytes)
  p.parts_bytes = parts;
  return 0;
}

// the front of all four entries: the image and the norms at the head of the workspace, written by scan_image_kernel and
// scan_norm_kernel from `qn` queries - rows of Q at `qsrc` (stride qld), those from qb on, the dead ones by `qrow_ids` left
// out: f32 queries, or a block of the corpus itself - and whether the corpus takes the ALIGNED instantiation (16-byte vector
// loads of whole chunks).  p.qtiles covers qn; p.image_bytes may be a larger block's.
struct ScanFront {
  u32x4* image;
  float* qnorm;
  bool aligned;
};

template <typename E, typename Q>
ScanFront scan_front(const ScanPlan& p, const typename ScanElem<E>::T* corpus, int64_t ldc, int32_t dim,
                     const typename ScanElem<Q>::T* qsrc, int64_t qld, const int64_t* qrow_ids, int64_t qb, int32_t qn,
                     void* workspace, int32_t* err, hipStream_t s) {
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  ScanFront f;
  f.image = reinterpret_cast<u32x4*>(ws);
  f.qnorm = reinterpret_cast<float*>(ws + p.image_bytes);
  f.aligned = (ldc % ScanElem<E>::kAlign == 0) && ((reinterpret_cast<uintptr_t>(corpus) & 15) == 0);
  const int qpad = p.qtiles * kScanQTile;
  hipLaunchKernelGGL((scan_image_kernel<Q>), dim3((unsigned)p.nchunks, (unsigned)p.qtiles), dim3(kScanThreads), 0, s, qsrc, qld,
                     dim, qrow_ids, qb, qn, p.nchunks, f.image);
  hipLaunchKernelGGL((scan_norm_kernel<Q>), dim3((unsigned)(qpad / kScanWaves)), dim3(kScanThreads), 0, s, qsrc, qld, dim,
                     qrow_ids, qb, qn, qpad, f.qnorm, err);
  return f;
}

// ... with f32 queries (q, dim), all of them
template <typename E>
ScanFront scan_front(const ScanPlan& p, const typename ScanElem<E>::T* corpus, int64_t ldc, int32_t dim, const float* queries,
                     int32_t q, void* workspace, int32_t* err, hipStream_t s) {
  return scan_front<E, float>(p, corpus, ldc, dim, queries, dim, nullptr, 0, q, workspace, err, s);
}

// what the two emitting entries check alike, then the cursor's reset: the last thing before the launches
template <typename A>
int scan_emit_begin(const void* corpus, int64_t ldc, int32_t dim, int64_t capacity, const A* out_first, const int64_t* out_row,
                    const float* out_approx, uint64_t* total, const void* workspace, hipStream_t s) {
  const auto addr = [](const void* ptr) { return reinterpret_cast<uintptr_t>(ptr); };
  if (corpus == nullptr || total == nullptr || workspace == nullptr || capacity < 0 ||
      (capacity > 0 && (out_first == nullptr || out_row == nullptr || out_approx == nullptr)) || (addr(workspace) & 15) ||
      (addr(total) & 7) || (addr(out_first) & (sizeof(A) - 1)) || (addr(out_row) & 7) || (addr(out_approx) & 3) || ldc < dim)
    return LSHRS_E_BADARG;
  const hipError_t e = hipMemsetAsync(total, 0, sizeof(uint64_t), s);
  return e != hipSuccess ? -(int)e : 0;
}

// the selection of one launch, for both kinds of query: scan_kernel over the plan's grid - SELF: the queries are the rows
// [qb, qb + q) - then scan_merge_kernel of the slices' winners into the caller's arrays
template <typename E, bool ALIGNED, bool SELF>
int scan_launch(const ScanPlan& p, const typename ScanElem<E>::T* corpus, int64_t m, int64_t ldc, int32_t dim,
                const int64_t* row_ids, const u32x4* image, const float* qnorm, int32_t q, int32_t window, uint64_t* parts,
                int32_t* err, int64_t qb, hipStream_t s) {
  const size_t shmem = (size_t)scan_select_lds(p.cap);
  if (shmem > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(scan_kernel<E, ALIGNED, SELF>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return -(int)e;
  }
  hipLaunchKernelGGL((scan_kernel<E, ALIGNED, SELF>), dim3((unsigned)p.slices, (unsigned)p.qtiles), dim3(kScanThreads), shmem, s,
                     corpus, m, ldc, dim, row_ids, image, qnorm, q, window, p.cap, p.rows_per_slice, parts, err, qb);
  return -(int)hipGetLastError();
}

template <typename E, bool SELF>
int scan_select(const ScanPlan& p, const ScanFront& f, const typename ScanElem<E>::T* corpus, int64_t m, int64_t ldc, int32_t dim,
                const int64_t* row_ids, int32_t q, int32_t window, uint64_t* parts, int64_t* out_rows, float* out_approx,
                int32_t* out_count, int32_t* err, int64_t qb, hipStream_t s) {
  const int rc = f.aligned ? scan_launch<E, true, SELF>(p, corpus, m, ldc, dim, row_ids, f.image, f.qnorm, q, window, parts, err, qb, s)
                           : scan_launch<E, false, SELF>(p, corpus, m, ldc, dim, row_ids, f.image, f.qnorm, q, window, parts, err, qb, s);
  if (rc) return rc;
  const int n = p.slices * window;
  int npad = 2;
  while (npad < n) npad <<= 1;
  const size_t merge_lds = (size_t)npad * sizeof(uint64_t);
  if (merge_lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(scan_merge_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)merge_lds);
    if (e != hipSuccess) return -(int)e;
  }
  hipLaunchKernelGGL(scan_merge_kernel, dim3((unsigned)q), dim3(kScanThreads), merge_lds, s, parts, n, npad, window, out_rows,
                     out_approx, out_count);
  return -(int)hipGetLastError();
}

template <typename E>
int scan_topk(const typename ScanElem<E>::T* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids,
              const float* queries, int32_t q, int32_t window, int64_t* out_rows, float* out_approx, int32_t* out_count,
              void* workspace, int32_t* err, void* stream) {
  if (q == 0) return 0;
  ScanPlan p;
  const int bad = scan_plan(q, m, dim, window, p);
  if (bad) return bad;
  if (corpus == nullptr || queries == nullptr || out_rows == nullptr || out_approx == nullptr || out_count == nullptr ||
      workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 15) || ldc < dim)
    return LSHRS_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint64_t* parts = reinterpret_cast<uint64_t*>(static_cast<unsigned char*>(workspace) + p.image_bytes + p.qnorm_bytes);
  const ScanFront f = scan_front<E>(p, corpus, ldc, dim, queries, q, workspace, err, s);
  return scan_select<E, false>(p, f, corpus, m, ldc, dim, row_ids, q, window, parts, out_rows, out_approx, out_count, err, 0, s);
}

// k-NN self-join: the rows [q_begin, q_begin + q_count) as queries, a block at a time, one after the other on the stream; the
// blocks share the workspace (image | norms | the slices' winners) and each merges into the caller's arrays at its offset
template <typename E>
int scan_knn(const typename ScanElem<E>::T* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
             int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
             void* workspace, int32_t* err, void* stream) {
  ScanPlan p;
  const int bad = scan_knn_plan(q_count, m, dim, window, qblock, p);
  if (bad) return bad;
  const auto addr = [](const void* ptr) { return reinterpret_cast<uintptr_t>(ptr); };
  if (q_begin < 0 || q_begin > m - q_count || (addr(row_ids) & 7) || (addr(out_rows) & 7) || (addr(out_approx) & 3) ||
      (addr(out_count) & 3) || (addr(workspace) & 15) || (addr(err) & 3))
    return LSHRS_E_BADARG;
  if (q_count == 0) return 0;
  if (corpus == nullptr || out_rows == nullptr || out_approx == nullptr || out_count == nullptr || workspace == nullptr || ldc < dim)
    return LSHRS_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint64_t* parts = reinterpret_cast<uint64_t*>(static_cast<unsigned char*>(workspace) + p.image_bytes + p.qnorm_bytes);
  const int64_t block_rows = (int64_t)p.qtiles * kScanQTile;
  for (int64_t done = 0; done < q_count; done += block_rows) {
    const int qn = (int)(q_count - done < block_rows ? q_count - done : block_rows);
    scan_knn_block(m, qn, window, p);
    const ScanFront f = scan_front<E, E>(p, corpus, ldc, dim, corpus, ldc, row_ids, q_begin + done, qn, workspace, err, s);
    const int rc = scan_select<E, true>(p, f, corpus, m, ldc, dim, row_ids, qn, window, parts, out_rows + done * window,
                                        out_approx + done * window, out_count + done, err, q_begin + done, s);
    if (rc) return rc;
  }
  return 0;
}

template <typename E>
int scan_above(const typename ScanElem<E>::T* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids,
               const float* queries, int32_t q, const float* bars, int64_t capacity, int32_t* out_query, int64_t* out_row,
               float* out_approx, uint64_t* total, void* workspace, int32_t* err, void* stream) {
  if (q == 0) return 0;
  ScanPlan p;
  const int bad = scan_above_plan(q, m, dim, p);
  if (bad) return bad;
  if (queries == nullptr || bars == nullptr || (reinterpret_cast<uintptr_t>(bars) & 3) || (reinterpret_cast<uintptr_t>(queries) & 3))
    return LSHRS_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = scan_emit_begin(corpus, ldc, dim, capacity, out_query, out_row, out_approx, total, workspace, s);
  if (rc) return rc;
  const ScanFront f = scan_front<E>(p, corpus, ldc, dim, queries, q, workspace, err, s);
  const dim3 grid((unsigned)p.slices, (unsigned)p.qtiles), block(kScanThreads);
  unsigned long long* cursor = reinterpret_cast<unsigned long long*>(total);
  if (f.aligned)
    hipLaunchKernelGGL((scan_above_kernel<E, true>), grid, block, (size_t)kScanChunkBytes, s, corpus, m, ldc, dim, row_ids,
                       f.image, f.qnorm, bars, q, p.rows_per_slice, capacity, out_query, out_row, out_approx, cursor, err);
  else
    hipLaunchKernelGGL((scan_above_kernel<E, false>), grid, block, (size_t)kScanChunkBytes, s, corpus, m, ldc, dim, row_ids,
                       f.image, f.qnorm, bars, q, p.rows_per_slice, capacity, out_query, out_row, out_approx, cursor, err);
  return -(int)hipGetLastError();
}

template <typename E>
int scan_pairs(const typename ScanElem<E>::T* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, float bar,
               int32_t qblock, int64_t capacity, int64_t* out_a, int64_t* out_b, float* out_approx, uint64_t* total,
               void* workspace, int32_t* err, void* stream) {
  ScanPlan p;
  const int bad = scan_pairs_plan(m, dim, qblock, p);
  if (bad) return bad;
  if (reinterpret_cast<uintptr_t>(row_ids) & 7) return LSHRS_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = scan_emit_begin(corpus, ldc, dim, capacity, out_a, out_b, out_approx, total, workspace, s);
  if (rc) return rc;
  unsigned long long* cursor = reinterpret_cast<unsigned long long*>(total);
  const size_t lds = (size_t)ScanElem<E>::kTerms * (kScanChunkBytes / 2);
  const int64_t block_rows = (int64_t)p.qtiles * kScanQTile;
  // the blocks one after the other on the stream: they share the image, the norms and the cursor
  for (int64_t qb = 0; qb < m; qb += block_rows) {
    const int qn = (int)(m - qb < block_rows ? m - qb : block_rows);
    p.qtiles = (qn + kScanQTile - 1) / kScanQTile;
    scan_slices(m - qb, p.qtiles, (int64_t)lds, INT64_MAX, p.rows_per_slice, p.slices, kScanPairsPerCu);
    const ScanFront f = scan_front<E, E>(p, corpus, ldc, dim, corpus, ldc, row_ids, qb, qn, workspace, err, s);
    const dim3 grid((unsigned)p.slices, (unsigned)p.qtiles), block(kScanThreads);
    if (f.aligned)
      hipLaunchKernelGGL((scan_pairs_kernel<E, true>), grid, block, lds, s, corpus, m, ldc, dim, row_ids, f.image, f.qnorm, bar,
                         qb, qn, p.rows_per_slice, capacity, out_a, out_b, out_approx, cursor, err);
    else
      hipLaunchKernelGGL((scan_pairs_kernel<E, false>), grid, block, lds, s, corpus, m, ldc, dim, row_ids, f.image, f.qnorm, bar,
                         qb, qn, p.rows_per_slice, capacity, out_a, out_b, out_approx, cursor, err);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return -(int)le;
  }
  return 0;
}
}  // namespace

extern "C" {

int64_t lshrs_scan_workspace_bytes(int32_t q, int64_t m, int32_t dim, int32_t window) {
  ScanPlan p;
  const int bad = scan_plan(q, m, dim, window, p);
  if (bad) return bad;
  return p.image_bytes + p.qnorm_bytes + p.parts_bytes + 16;
}

int32_t lshrs_scan_max_window(void) { return kScanMaxWindow; }

// The bound DESIGN.md derives: split + f32 accumulation, carried through the norm arithmetic.
double lshrs_scan_epsilon(int32_t elem, int32_t dim) {
  if (elem < LSHRS_SCAN_F32 || elem > LSHRS_SCAN_F8E4M3 || dim <= 0 || dim > kScanMaxDim) return -1.0;
  const bool two = elem == LSHRS_SCAN_F32 || elem == LSHRS_SCAN_F16;
  const double split = (two ? 3.0 : 1.0) * 0x1p-14;
  const double products = (two ? 3.0 : 2.0) * kScanKChunk * ((dim + kScanKChunk - 1) / kScanKChunk);
  const double acc = (1.0 + 0x1p-7) * (1.0 + 0x1p-7) * products * 0x1p-23 / (1.0 - products * 0x1p-23);
  const double eta = (dim + 12.0) * 0x1p-24;
  return ((split + acc) * (1.0 + eta) + eta) * 1.0625;
}

int lshrs_scan_topk_f32(const float* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, const float* queries,
                        int32_t q, int32_t window, int64_t* out_rows, float* out_approx, int32_t* out_count, void* workspace,
                        int32_t* err, void* stream) {
  return scan_topk<float>(corpus, m, ldc, dim, row_ids, queries, q, window, out_rows, out_approx, out_count, workspace, err, stream);
}

int lshrs_scan_topk_bf16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, const float* queries,
                         int32_t q, int32_t window, int64_t* out_rows, float* out_approx, int32_t* out_count, void* workspace,
                         int32_t* err, void* stream) {
  return scan_topk<Bf16>(corpus, m, ldc, dim, row_ids, queries, q, window, out_rows, out_approx, out_count, workspace, err, stream);
}

int lshrs_scan_topk_f16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, const float* queries,
                        int32_t q, int32_t window, int64_t* out_rows, float* out_approx, int32_t* out_count, void* workspace,
                        int32_t* err, void* stream) {
  return scan_topk<F16>(corpus, m, ldc, dim, row_ids, queries, q, window, out_rows, out_approx, out_count, workspace, err, stream);
}

int lshrs_scan_topk_i8(const int8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, const float* queries,
                       int32_t q, int32_t window, int64_t* out_rows, float* out_approx, int32_t* out_count, void* workspace,
                       int32_t* err, void* stream) {
  return scan_topk<I8>(corpus, m, ldc, dim, row_ids, queries, q, window, out_rows, out_approx, out_count, workspace, err, stream);
}

int lshrs_scan_topk_f8e4m3(const uint8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids,
                           const float* queries, int32_t q, int32_t window, int64_t* out_rows, float* out_approx,
                           int32_t* out_count, void* workspace, int32_t* err, void* stream) {
  return scan_topk<F8E4M3>(corpus, m, ldc, dim, row_ids, queries, q, window, out_rows, out_approx, out_count, workspace, err, stream);
}

int64_t lshrs_scan_above_workspace_bytes(int32_t q, int64_t m, int32_t dim) {
  ScanPlan p;
  const int bad = scan_above_plan(q, m, dim, p);
  if (bad) return bad;
  return p.image_bytes + p.qnorm_bytes + 16;
}

int lshrs_scan_above_f32(const float* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, const float* queries,
                         int32_t q, const float* bars, int64_t capacity, int32_t* out_query, int64_t* out_row, float* out_approx,
                         uint64_t* total, void* workspace, int32_t* err, void* stream) {
  return scan_above<float>(corpus, m, ldc, dim, row_ids, queries, q, bars, capacity, out_query, out_row, out_approx, total, workspace,
                        err, stream);
}

int lshrs_scan_above_bf16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, const float* queries,
                         int32_t q, const float* bars, int64_t capacity, int32_t* out_query, int64_t* out_row, float* out_approx,
                         uint64_t* total, void* workspace, int32_t* err, void* stream) {
  return scan_above<Bf16>(corpus, m, ldc, dim, row_ids, queries, q, bars, capacity, out_query, out_row, out_approx, total, workspace,
                        err, stream);
}

int lshrs_scan_above_f16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, const float* queries,
                         int32_t q, const float* bars, int64_t capacity, int32_t* out_query, int64_t* out_row, float* out_approx,
                         uint64_t* total, void* workspace, int32_t* err, void* stream) {
  return scan_above<F16>(corpus, m, ldc, dim, row_ids, queries, q, bars, capacity, out_query, out_row, out_approx, total, workspace,
                        err, stream);
}

int lshrs_scan_above_i8(const int8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, const float* queries,
                         int32_t q, const float* bars, int64_t capacity, int32_t* out_query, int64_t* out_row, float* out_approx,
                         uint64_t* total, void* workspace, int32_t* err, void* stream) {
  return scan_above<I8>(corpus, m, ldc, dim, row_ids, queries, q, bars, capacity, out_query, out_row, out_approx, total, workspace,
                        err, stream);
}

int lshrs_scan_above_f8e4m3(const uint8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, const float* queries,
                         int32_t q, const float* bars, int64_t capacity, int32_t* out_query, int64_t* out_row, float* out_approx,
                         uint64_t* total, void* workspace, int32_t* err, void* stream) {
  return scan_above<F8E4M3>(corpus, m, ldc, dim, row_ids, queries, q, bars, capacity, out_query, out_row, out_approx, total, workspace,
                        err, stream);
}

int64_t lshrs_scan_pairs_workspace_bytes(int64_t m, int32_t dim, int32_t qblock) {
  ScanPlan p;
  const int bad = scan_pairs_plan(m, dim, qblock, p);
  if (bad) return bad;
  return p.image_bytes + p.qnorm_bytes + 16;
}

int lshrs_scan_pairs_f32(const float* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, float bar,
                          int32_t qblock, int64_t capacity, int64_t* out_a, int64_t* out_b, float* out_approx, uint64_t* total,
                          void* workspace, int32_t* err, void* stream) {
  return scan_pairs<float>(corpus, m, ldc, dim, row_ids, bar, qblock, capacity, out_a, out_b, out_approx, total, workspace, err,
                         stream);
}

int lshrs_scan_pairs_bf16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, float bar,
                          int32_t qblock, int64_t capacity, int64_t* out_a, int64_t* out_b, float* out_approx, uint64_t* total,
                          void* workspace, int32_t* err, void* stream) {
  return scan_pairs<Bf16>(corpus, m, ldc, dim, row_ids, bar, qblock, capacity, out_a, out_b, out_approx, total, workspace, err,
                         stream);
}

int lshrs_scan_pairs_f16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, float bar,
                          int32_t qblock, int64_t capacity, int64_t* out_a, int64_t* out_b, float* out_approx, uint64_t* total,
                          void* workspace, int32_t* err, void* stream) {
  return scan_pairs<F16>(corpus, m, ldc, dim, row_ids, bar, qblock, capacity, out_a, out_b, out_approx, total, workspace, err,
                         stream);
}

int lshrs_scan_pairs_i8(const int8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, float bar,
                          int32_t qblock, int64_t capacity, int64_t* out_a, int64_t* out_b, float* out_approx, uint64_t* total,
                          void* workspace, int32_t* err, void* stream) {
  return scan_pairs<I8>(corpus, m, ldc, dim, row_ids, bar, qblock, capacity, out_a, out_b, out_approx, total, workspace, err,
                         stream);
}

int lshrs_scan_pairs_f8e4m3(const uint8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, float bar,
                          int32_t qblock, int64_t capacity, int64_t* out_a, int64_t* out_b, float* out_approx, uint64_t* total,
                          void* workspace, int32_t* err, void* stream) {
  return scan_pairs<F8E4M3>(corpus, m, ldc, dim, row_ids, bar, qblock, capacity, out_a, out_b, out_approx, total, workspace, err,
                         stream);
}

int64_t lshrs_scan_knn_workspace_bytes(int32_t q_count, int64_t m, int32_t dim, int32_t window, int32_t qblock) {
  ScanPlan p;
  const int bad = scan_knn_plan(q_count, m, dim, window, qblock, p);
  if (bad) return bad;
  return p.image_bytes + p.qnorm_bytes + p.parts_bytes + 16;
}

int lshrs_scan_knn_f32(const float* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream) {
  return scan_knn<float>(corpus, m, ldc, dim, row_ids, q_begin, q_count, window, qblock, out_rows, out_approx, out_count, workspace,
                       err, stream);
}

int lshrs_scan_knn_bf16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream) {
  return scan_knn<Bf16>(corpus, m, ldc, dim, row_ids, q_begin, q_count, window, qblock, out_rows, out_approx, out_count, workspace,
                       err, stream);
}

int lshrs_scan_knn_f16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream) {
  return scan_knn<F16>(corpus, m, ldc, dim, row_ids, q_begin, q_count, window, qblock, out_rows, out_approx, out_count, workspace,
                       err, stream);
}

int lshrs_scan_knn_i8(const int8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream) {
  return scan_knn<I8>(corpus, m, ldc, dim, row_ids, q_begin, q_count, window, qblock, out_rows, out_approx, out_count, workspace,
                       err, stream);
}

int lshrs_scan_knn_f8e4m3(const uint8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream) {
  return scan_knn<F8E4M3>(corpus, m, ldc, dim, row_ids, q_begin, q_count, window, qblock, out_rows, out_approx, out_count, workspace,
                       err, stream);
}

}  // extern "C"
