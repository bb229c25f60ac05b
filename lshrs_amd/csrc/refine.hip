// refine.hip - one local-join round over a k-NN graph (include/lshrs_refine.h; lshrs_amd/_refine.py): what stands between a
// neighbour table and the candidate lists of its refinement.
//
//   edges     one lane per entry of the table: kept when it is the first of its row to name that row and, of a mutual pair, the
//             lower row's - every undirected pair once.
//   expand    per row the rows at distance one or two over an adjacency, each once: an open-addressing set of int32 in LDS,
//             filled by compare-and-swap - one WAVE per row whose bound U is at most kWaveSet, one WORKGROUP per row up to
//             kMaxSet.  Run twice over the same rows: to count, and - behind the caller's prefix sum - to write.  A lane that
//             wins a slot of the set has found a NEW row and counts / writes it there and then: the order of a list is the order
//             the lanes won in.
//
// The library stands alone: no symbol of liblshrs_hip.so, liblshrs_groups.so or liblshrs_graph.so.
#include "lshrs_lists.h"
#include "lshrs_refine.h"

namespace {

using namespace lshrs;                             // (lshrs_lists.h: the layers shared with graph, groups and join)

constexpr int64_t kMaxCount = 0x7fffffffLL;        // rows, and entries of a table: a member of a set is an int32
constexpr int kWaveSet = 1024;                     // the largest bound one wave takes: 2048 slots, 8 KiB per wave, 32 KiB per workgroup
constexpr int kMaxSet = 8192;                      // the largest bound a workgroup takes: 16384 slots, 64 KiB, two workgroups per CU
constexpr int kWaveSlots = 2 * kWaveSet;
constexpr int kMaxSlots = 2 * kMaxSet;
constexpr int kMinSlots = 64;
constexpr int kSub = 16;                           // the lanes that share one midpoint's list: four midpoints per wave at a time
constexpr int kLongBlocksPerCu = 2;
constexpr int kEmpty = -1;                         // (no row is negative)

__global__ __launch_bounds__(kThreads) void edges_kernel(const int64_t* __restrict__ graph, int64_t n_rows, int k_in,
                                                         uint8_t* __restrict__ keep, int32_t* err) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int bad = 0;
  if (e < n_rows * k_in) {
    const int64_t r = e / k_in;
    const int c = (int)(e - r * k_in);
    const int64_t* mine = graph + r * k_in;
    const int64_t g = mine[c];
    bool kept = false;
    if (g < -1 || g >= n_rows) {
      bad |= LSHRS_REFINE_ERR_OUTSIDE;
    } else if (g == r) {
      bad |= LSHRS_REFINE_ERR_SELF;
    } else if (g >= 0) {
      kept = true;
      for (int j = 0; j < c; ++j) kept = kept && mine[j] != g;                  // the first occurrence counts
      if (kept && g < r) {                                                      // of a mutual pair the lower row's entry
        const int64_t* theirs = graph + g * k_in;
        for (int j = 0; j < k_in; ++j) kept = kept && theirs[j] != r;
      }
    }
    keep[e] = kept ? 1 : 0;
  }
  report(err, bad);
}

// ------------------------------------------------------------------------------------------
// expand
// ------------------------------------------------------------------------------------------
struct ExpandArgs {
  const int64_t* nbr;
  const int64_t* row_off;
  int64_t n_rows, total;
  int max_degree;
  int32_t* cand_count;        // the count launch: where |C(r)| goes; the write launch: null
  const int64_t* cand_off;    // the write launch: the lists of cand; the count launch: null
  int64_t* cand;
  int64_t cand_total;
  int32_t* err;
};

// What the entry m of a list adds to its row's bound: the length of m's own list where m is a midpoint - a row, with a list
// inside nbr, at or under the cap - and where that list begins; else 0.
__device__ __forceinline__ int64_t midpoint_of(const ExpandArgs& s, int64_t m, int64_t& begin, int& bad) {
  begin = 0;
  if ((uint64_t)m >= (uint64_t)s.n_rows) {
    bad |= LSHRS_REFINE_ERR_ENTRY;
    return 0;
  }
  const int64_t len = list_of(s, m, begin, bad, LSHRS_REFINE_ERR_RANGE);
  return (s.max_degree > 0 && len > s.max_degree) ? 0 : len;
}

// U(row) = deg + the lists of its midpoints, by ONE LANE: entries are added while the sum is within kMaxSet - a row beyond that
// is beyond every tier, by how much decides nothing.
__device__ __forceinline__ int64_t bound_by_lane(const ExpandArgs& s, int64_t begin, int64_t deg) {
  int64_t bound = deg, unused_begin;
  int unused = 0;                     // (what is wrong with a list is the wave kernel's to report)
  for (int64_t i = 0; i < deg && bound <= kMaxSet; ++i) bound += midpoint_of(s, s.nbr[begin + i], unused_begin, unused);
  return bound;
}

// The same by the 64 lanes of a wave, every one of which calls it and gets the sum; deg <= kWaveSet.
__device__ __forceinline__ int64_t bound_by_wave(const ExpandArgs& s, int64_t begin, int64_t deg, int lane, int& bad) {
  int64_t sum = 0, unused_begin;
  for (int64_t i = lane; i < deg; i += 64) sum += midpoint_of(s, s.nbr[begin + i], unused_begin, bad);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) sum += __shfl_xor(sum, off);
  return deg + sum;
}

// v into the set of mask + 1 slots: true where THIS lane put it there, false where it was there already.  At most
// (mask + 1) / 2 different rows ever arrive (the bound), so an empty slot is met before the probes run out.
__device__ __forceinline__ bool insert(int* table, uint32_t mask, int v) {
  uint32_t at = ((uint32_t)v * 2654435761u >> 7) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const int old = atomicCAS(table + at, kEmpty, v);
    if (old == kEmpty) return true;
    if (old == v) return false;
    at = (at + 1) & mask;
  }
  return false;
}

// One row whose bound is within the tier's, by THREADS threads (this one: t): the set cleared, A(row) put in, then the lists
// of its midpoints - kSub lanes to a midpoint.  Every loop runs the same number of times in all lanes of a wave, so that the
// new rows of a step can be counted by a ballot.
template <int THREADS, bool WAVE>
__device__ __forceinline__ void expand_row(const ExpandArgs& s, int* table, int* counter, int64_t row, int64_t begin, int deg,
                                           int bound, int t, int& bad) {
  const bool writing = s.cand_off != nullptr;
  const int lane = t & 63;
  int64_t out = 0, room = 0;
  if (writing) {                      // (uniform in the row's threads)
    out = s.cand_off[row];
    const int64_t end = s.cand_off[row + 1];
    if (out < 0 || end < out || end > s.cand_total) {
      bad |= LSHRS_REFINE_ERR_RANGE;
      return;
    }
    room = end - out;
  }
  if (deg == 0) {
    if (!writing && t == 0) s.cand_count[row] = 0;
    return;
  }
  int slots = kMinSlots;
  while (slots < 2 * bound) slots <<= 1;
  const uint32_t mask = (uint32_t)slots - 1u;
  for (int i = t; i < slots; i += THREADS) table[i] = kEmpty;
  if (!WAVE && t == 0) *counter = 0;
  pass_done<WAVE>();

  int found = 0;                      // WAVE: the rows found so far, the same in every lane
  // the lanes of this wave whose v is new: each gets a place in the list, and writes v there in the write launch
  auto emit = [&](bool fresh, int64_t v) {
    const Places won = places_of(fresh);
    if (!won.flagged) return;
    const int before = won.rank();
    int base = found;
    if (WAVE) {
      found += won.count();
    } else {
      if (lane == won.leader()) base = atomicAdd(counter, won.count());
      base = __shfl(base, won.leader());
    }
    if (fresh && writing) {
      if (base + before < room) s.cand[out + base + before] = v;
      else bad |= LSHRS_REFINE_ERR_RANGE;
    }
  };
  auto take = [&](bool has, int64_t v) {
    if (has && (uint64_t)v >= (uint64_t)s.n_rows) bad |= LSHRS_REFINE_ERR_ENTRY;
    const bool ok = has && (uint64_t)v < (uint64_t)s.n_rows && v != row;
    emit(ok && insert(table, mask, (int)v), v);
  };

  for (int i0 = 0; i0 < deg; i0 += THREADS) {
    const int i = i0 + t;
    take(i < deg, i < deg ? s.nbr[begin + i] : -1);
  }
  constexpr int kGroups = THREADS / kSub;
  const int group = t / kSub, sub = t % kSub;
  for (int i0 = 0; i0 < deg; i0 += kGroups) {
    const int i = i0 + group;
    int64_t mb = 0;
    int unused = 0;                   // (the entry was judged above, its list by the bound)
    const int dm = i < deg ? (int)midpoint_of(s, s.nbr[begin + i], mb, unused) : 0;
    int widest = dm;                  // ... of the four midpoints of this wave
    for (int off = kSub; off < 64; off <<= 1) {
      const int other = __shfl_xor(widest, off);
      widest = other > widest ? other : widest;
    }
    for (int j0 = 0; j0 < widest; j0 += kSub) {
      const int j = j0 + sub;
      take(j < dm, j < dm ? s.nbr[mb + j] : -1);
    }
  }
  pass_done<WAVE>();
  if (!writing && t == 0) s.cand_count[row] = WAVE ? found : *counter;
  pass_done<WAVE>();                  // (the set and the counter are read: they may be cleared again)
}

// Rows whose bound is at most kWaveSet: one wave per row, four rows per workgroup, no workgroup barrier.
__global__ __launch_bounds__(kThreads) void expand_wave_kernel(ExpandArgs s) {
  __shared__ int slices[kWavesPerGroup][kWaveSlots];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWavesPerGroup + wave;
  int bad = 0;
  if (row < s.n_rows) {               // (uniform in the wave)
    int64_t begin;
    const int64_t deg = list_of(s, row, begin, bad, LSHRS_REFINE_ERR_RANGE);
    if (deg <= kWaveSet) {
      const int64_t bound = bound_by_wave(s, begin, deg, lane, bad);
      if (bound <= kWaveSet) expand_row<64, true>(s, slices[wave], nullptr, row, begin, (int)deg, (int)bound, lane, bad);
    }
  }
  report(s.err, bad);
}

// Rows beyond: the workgroups walk the rows (walk_rows) - a thread bounds one row and notes it, with its bound, where it is the
// workgroup's - and expand the noted rows one after the other.  A row beyond kMaxSet gets its -1 in the count launch and
// nothing else.
__global__ __launch_bounds__(kThreads) void expand_long_kernel(ExpandArgs s) {
  extern __shared__ __attribute__((aligned(16))) unsigned char refine_lds[];
  int* noted = reinterpret_cast<int*>(refine_lds) + kMaxSlots;     // behind the table: walk_rows' noted rows and their bounds,
  int bad = 0;                                                     // and behind them the counter of a row
  walk_rows<kThreads, true>(
      s, noted,
      [](const ExpandArgs& s, int64_t row, int& bound_of) {
        int64_t begin;
        int unused = 0;               // (a list out of range is the wave kernel's to report)
        const int64_t deg = list_of(s, row, begin, unused, LSHRS_REFINE_ERR_RANGE);
        const int64_t bound = deg > kMaxSet ? deg : bound_by_lane(s, begin, deg);
        if (bound > kMaxSet) {
          if (s.cand_off == nullptr) s.cand_count[row] = -1;
          return false;
        }
        bound_of = (int)bound;
        return bound > kWaveSet;
      },
      [&bad](const ExpandArgs& s, int64_t row, int bound) {
        int* table = reinterpret_cast<int*>(refine_lds);
        int64_t begin;
        int unused = 0;
        const int64_t deg = list_of(s, row, begin, unused, LSHRS_REFINE_ERR_RANGE);
        expand_row<kThreads, false>(s, table, table + kMaxSlots + kWalkInts<kThreads, true>, row, begin, (int)deg, bound,
                                    threadIdx.x, bad);
      });
  report(s.err, bad);
}

constexpr size_t kLongLds = (size_t)kMaxSlots * sizeof(int) + (kWalkInts<kThreads, true> + 3) * sizeof(int);

}  // namespace

extern "C" {

int lshrs_refine_abi_version(void) { return LSHRS_REFINE_ABI_VERSION; }
int32_t lshrs_refine_wave_set(void) { return kWaveSet; }
int32_t lshrs_refine_max_set(void) { return kMaxSet; }

int lshrs_refine_edges_i64(const int64_t* graph, int64_t n_rows, int32_t k_in, uint8_t* keep, int32_t* err, void* stream) {
  if (n_rows < 0 || k_in < 0) return LSHRS_E_BADARG;
  if (n_rows > kMaxCount || n_rows * (int64_t)k_in > kMaxCount) return LSHRS_E_TOOLARGE;
  if (n_rows == 0 || k_in == 0) return 0;
  if (!usable(graph, 8) || keep == nullptr || !usable(err, 4)) return LSHRS_E_BADARG;
  hipLaunchKernelGGL(edges_kernel, dim3(blocks_for(n_rows * k_in, kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     graph, n_rows, (int)k_in, keep, err);
  return -(int)hipGetLastError();
}

int lshrs_refine_expand_count_i64(const int64_t* nbr, const int64_t* row_off, int64_t n_rows, int64_t total, int32_t max_degree,
                                  int32_t* cand_count, int32_t* err, void* stream) {
  if (n_rows < 0 || total < 0) return LSHRS_E_BADARG;
  if (n_rows > kMaxCount) return LSHRS_E_TOOLARGE;
  if (n_rows == 0) return 0;
  if (!usable(row_off, 8) || !usable(cand_count, 4) || !usable(err, 4)) return LSHRS_E_BADARG;
  if (total > 0 && !usable(nbr, 8)) return LSHRS_E_BADARG;
  const ExpandArgs args{nbr, row_off, n_rows, total, max_degree, cand_count, nullptr, nullptr, 0, err};
  return launch_tiers(expand_wave_kernel, expand_long_kernel, args, n_rows, kLongLds, kLongBlocksPerCu, stream);
}

int lshrs_refine_expand_write_i64(const int64_t* nbr, const int64_t* row_off, int64_t n_rows, int64_t total, int32_t max_degree,
                                  const int64_t* cand_off, int64_t* cand, int64_t cand_total, int32_t* err, void* stream) {
  if (n_rows < 0 || total < 0 || cand_total < 0) return LSHRS_E_BADARG;
  if (n_rows > kMaxCount) return LSHRS_E_TOOLARGE;
  if (n_rows == 0) return 0;
  if (!usable(row_off, 8) || !usable(cand_off, 8) || !usable(err, 4)) return LSHRS_E_BADARG;
  if (total > 0 && !usable(nbr, 8)) return LSHRS_E_BADARG;
  if (cand_total > 0 && !usable(cand, 8)) return LSHRS_E_BADARG;
  const ExpandArgs args{nbr, row_off, n_rows, total, max_degree, nullptr, cand_off, cand, cand_total, err};
  return launch_tiers(expand_wave_kernel, expand_long_kernel, args, n_rows, kLongLds, kLongBlocksPerCu, stream);
}

}  // extern "C"
