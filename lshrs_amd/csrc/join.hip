// join.hip - the LSH self-join (include/lshrs_join.h; lshrs_amd/_join.py): the candidate pairs of a banded index - two members
// that share a bucket in at least `min_collisions` bands - out of ONE bucket segment (codes ascending, offsets, members), every
// pair once and with its collision count, nothing sorted.
//
//   row map   int32 [n_rows][num_bands]: the counted bucket (2 .. max_bucket entries) a row is a member of in each band, -1 where
//             there is none.  join_rowmap_kernel: one lane per entry of the member list, its bucket by bisection on `offsets`, the
//             cell by a compare-and-swap from -1 - a second, DIFFERENT bucket for one (row, band) is an id indexed under two
//             signatures: error bit 0, the join is refused.
//   emit      the raw pairs - len (len - 1) / 2 per counted bucket - are numbered through an exclusive prefix sum the caller
//             makes.  join_emit_kernel: one lane per raw pair, whatever the largest bucket is: its bucket by bisection on the
//             prefix, its two entries from the triangular index, the two rows of the map compared band by band.  The map says in
//             which bands the pair collides; the pair leaves only from the FIRST of them, so it leaves once, and the count of what
//             left is the number of distinct candidate pairs.  Hits leave as scan.hip's do (scan_emit): one 64-bit add per wave
//             on the cursor, plain stores.
// Every loop is bounded by its iteration count; no workgroup waits for another.
#include "lshrs_common.h"
#include "lshrs_join.h"
#include "lshrs_lists.h"

namespace {

using lshrs::blocks_for;
using lshrs::places_of;
using lshrs::Places;
using lshrs::report;
using lshrs::usable;

constexpr int kJoinThreads = 256;
constexpr int64_t kJoinMaxLanes = 0x7fffffffLL * kJoinThreads;      // what a one-dimensional grid of 256-lane workgroups covers
constexpr int64_t kJoinMaxBuckets = 0x7fffffffLL;                   // a bucket is an int32 in the map
constexpr int64_t kJoinMaxCells = (int64_t)1 << 40;
constexpr int64_t kJoinMaxRaw = (int64_t)1 << 31;                   // raw pairs of one launch
constexpr int kErrTwoBuckets = 1, kErrBand = 2, kErrMissing = 256, kErrBeyond = 512;

typedef int32_t i32x2 __attribute__((ext_vector_type(2)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
template <int W> struct MapVec;
template <> struct MapVec<1> { typedef int32_t T; };
template <> struct MapVec<2> { typedef i32x2 T; };
template <> struct MapVec<4> { typedef i32x4 T; };
template <int W> __device__ __forceinline__ int32_t map_elem(const typename MapVec<W>::T& v, int e) { return v[e]; }
template <> __device__ __forceinline__ int32_t map_elem<1>(const int32_t& v, int) { return v; }

// the largest g of [0, n) with a[g] <= v, for a[0 .. n] ascending and a[0] <= v; n < 2^31: at most 31 halvings
__device__ __forceinline__ int64_t last_at_or_below(const int64_t* __restrict__ a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  for (int it = 0; it < 32 && hi - lo > 1; ++it) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kJoinThreads) void join_rowmap_kernel(const int64_t* __restrict__ codes, const int64_t* __restrict__ offsets,
                                                                   int64_t n_codes, int shift, int num_bands,
                                                                   const int64_t* __restrict__ member_rows, int64_t n_members,
                                                                   int64_t n_rows, int64_t max_bucket, int32_t* rowmap, int32_t* err) {
  const int64_t e = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x;
  int bad = 0;
  if (e < n_members) {
    const int64_t row = member_rows[e];
    if (row < 0) {
      bad = kErrMissing;
    } else if (row >= n_rows) {
      bad = kErrBeyond;
    } else {
      const int64_t g = last_at_or_below(offsets, n_codes, e);
      const int64_t first = offsets[g], end = offsets[g + 1], len = end - first;
      if (e >= first && e < end && len >= 2 && len <= max_bucket) {
        const int64_t band = codes[g] >> shift;
        if (band < 0 || band >= num_bands) {
          bad = kErrBand;
        } else {
          const int old = atomicCAS(rowmap + row * num_bands + band, -1, (int)g);
          if (old != -1 && old != (int)g) bad = kErrTwoBuckets;
        }
      }
    }
  }
  report(err, bad);
}

// W: int32 per load of a map row - 4 where num_bands is a multiple of 4 (every row then starts at a 16-byte boundary), 2
// where it is even, else 1
template <int W>
__global__ __launch_bounds__(kJoinThreads) void join_emit_kernel(const int64_t* __restrict__ offsets, const int64_t* __restrict__ prefix,
                                                                 int64_t n_codes, const int64_t* __restrict__ member_rows,
                                                                 int64_t n_rows, int num_bands, const int32_t* __restrict__ rowmap,
                                                                 int64_t raw_begin, int64_t raw_count, int min_collisions,
                                                                 int64_t capacity, int64_t* __restrict__ out_a,
                                                                 int64_t* __restrict__ out_b, int32_t* __restrict__ out_hits,
                                                                 unsigned long long* __restrict__ total) {
  typedef typename MapVec<W>::T V;
  const int64_t idx = (int64_t)blockIdx.x * kJoinThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool hit = false;
  int64_t a = 0, b = 0;
  int collisions = 0;
  if (idx < raw_count) {
    const int64_t p = raw_begin + idx;
    const int64_t g = last_at_or_below(prefix, n_codes, p);
    const int64_t t = p - prefix[g], count = prefix[g + 1] - prefix[g];
    const int64_t base = offsets[g], len = offsets[g + 1] - base;
    if (t >= 0 && t < count) {
      // pair t of the bucket is its entries (i, j), i < j, with t = j (j - 1) / 2 + i: the root, then integer steps make it exact
      int64_t j = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
      if (j < 1) j = 1;
      for (int s = 0; s < 2 && j * (j - 1) / 2 > t; ++s) --j;
      for (int s = 0; s < 2 && (j + 1) * j / 2 <= t; ++s) ++j;
      const int64_t i = t - j * (j - 1) / 2;
      if (i >= 0 && i < j && j < len) {
        const int64_t ra = member_rows[base + i], rb = member_rows[base + j];
        if (ra >= 0 && rb >= 0 && ra < n_rows && rb < n_rows && ra != rb) {
          a = ra < rb ? ra : rb;
          b = ra < rb ? rb : ra;
          const V* __restrict__ ma = reinterpret_cast<const V*>(rowmap + a * num_bands);
          const V* __restrict__ mb = reinterpret_cast<const V*>(rowmap + b * num_bands);
          int first = -1;
          for (int v = 0; v < num_bands / W; ++v) {
            const V va = ma[v], vb = mb[v];
#pragma unroll
            for (int e = 0; e < W; ++e) {
              const int32_t x = map_elem<W>(va, e);
              const bool same = x >= 0 && x == map_elem<W>(vb, e);
              collisions += same ? 1 : 0;
              first = (same && first < 0) ? x : first;
            }
          }
          hit = collisions >= min_collisions && first == (int)g;
        }
      }
    }
  }
  // the wave reserves the slots of its hits with one add on the cursor (which counts what does not fit, too)
  const Places hits = places_of(hit);
  if (hits.flagged == 0ull) return;
  const int leader = hits.leader();
  unsigned long long first_slot = 0ull;
  if (lane == leader) first_slot = atomicAdd(total, (unsigned long long)hits.count());
  first_slot = __shfl(first_slot, leader);
  const int64_t slot = (int64_t)first_slot + hits.rank();
  if (hit && slot < capacity) {
    out_a[slot] = a;
    out_b[slot] = b;
    out_hits[slot] = collisions;
  }
}


}  // namespace

extern "C" {

int64_t lshrs_join_workspace_bytes(int64_t n_rows, int32_t num_bands) {
  if (n_rows < 0 || num_bands < 1) return LSHRS_E_BADARG;
  if (n_rows > kJoinMaxBuckets || n_rows * (int64_t)num_bands > kJoinMaxCells) return LSHRS_E_TOOLARGE;
  const int64_t bytes = (n_rows * (int64_t)num_bands * 4 + 15) & ~(int64_t)15;
  return bytes < 16 ? 16 : bytes;
}

int lshrs_join_rowmap_i64(const int64_t* codes, const int64_t* offsets, int64_t n_codes, int32_t band_bytes, int32_t num_bands,
                          const int64_t* member_rows, int64_t n_members, int64_t n_rows, int64_t max_bucket, void* workspace,
                          int32_t* err, void* stream) {
  if (n_codes < 0 || n_members < 0 || n_rows < 0 || band_bytes < 1 || band_bytes > 6 || num_bands < 1 || max_bucket < 2)
    return LSHRS_E_BADARG;
  if (!usable(workspace, 16) || !usable(err, 4)) return LSHRS_E_BADARG;
  if (n_codes > 0 && n_members > 0 && (!usable(codes, 8) || !usable(offsets, 8) || !usable(member_rows, 8))) return LSHRS_E_BADARG;
  if (n_codes > kJoinMaxBuckets || n_rows > kJoinMaxBuckets || n_rows * (int64_t)num_bands > kJoinMaxCells || n_members > kJoinMaxLanes)
    return LSHRS_E_TOOLARGE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t cells = n_rows * (int64_t)num_bands;
  if (cells > 0) {
    const hipError_t rc = hipMemsetAsync(workspace, 0xff, (size_t)cells * 4, s);
    if (rc != hipSuccess) return -(int)rc;
  }
  if (n_codes == 0 || n_members == 0) return 0;
  hipLaunchKernelGGL(join_rowmap_kernel, dim3(blocks_for(n_members, kJoinThreads)), dim3(kJoinThreads), 0, s, codes, offsets, n_codes,
                     8 * band_bytes, (int)num_bands, member_rows, n_members, n_rows, max_bucket, static_cast<int32_t*>(workspace), err);
  return -(int)hipGetLastError();
}

int lshrs_join_emit_i64(const int64_t* offsets, const int64_t* pair_prefix, int64_t n_codes, const int64_t* member_rows,
                        int64_t n_rows, int32_t num_bands, const void* workspace, int64_t raw_begin, int64_t raw_count,
                        int32_t min_collisions, int64_t capacity, int64_t* out_a, int64_t* out_b, int32_t* out_hits,
                        uint64_t* total, void* stream) {
  if (n_codes < 0 || n_rows < 0 || num_bands < 1 || raw_begin < 0 || raw_count < 0 || capacity < 0 || min_collisions < 1 ||
      min_collisions > num_bands)
    return LSHRS_E_BADARG;
  if (!usable(total, 8)) return LSHRS_E_BADARG;
  if (capacity > 0 && (!usable(out_a, 8) || !usable(out_b, 8) || !usable(out_hits, 4))) return LSHRS_E_BADARG;
  if (n_codes > kJoinMaxBuckets || n_rows > kJoinMaxBuckets || n_rows * (int64_t)num_bands > kJoinMaxCells || raw_count > kJoinMaxRaw)
    return LSHRS_E_TOOLARGE;
  if (n_codes == 0 || raw_count == 0) return 0;
  if (!usable(offsets, 8) || !usable(pair_prefix, 8) || !usable(member_rows, 8) || !usable(workspace, 16)) return LSHRS_E_BADARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(blocks_for(raw_count, kJoinThreads)), block(kJoinThreads);
  const int32_t* map = static_cast<const int32_t*>(workspace);
  unsigned long long* cursor = reinterpret_cast<unsigned long long*>(total);
  if (num_bands % 4 == 0)
    hipLaunchKernelGGL(join_emit_kernel<4>, grid, block, 0, s, offsets, pair_prefix, n_codes, member_rows, n_rows, (int)num_bands, map,
                       raw_begin, raw_count, (int)min_collisions, capacity, out_a, out_b, out_hits, cursor);
  else if (num_bands % 2 == 0)
    hipLaunchKernelGGL(join_emit_kernel<2>, grid, block, 0, s, offsets, pair_prefix, n_codes, member_rows, n_rows, (int)num_bands, map,
                       raw_begin, raw_count, (int)min_collisions, capacity, out_a, out_b, out_hits, cursor);
  else
    hipLaunchKernelGGL(join_emit_kernel<1>, grid, block, 0, s, offsets, pair_prefix, n_codes, member_rows, n_rows, (int)num_bands, map,
                       raw_begin, raw_count, (int)min_collisions, capacity, out_a, out_b, out_hits, cursor);
  return -(int)hipGetLastError();
}

}  // extern "C"
