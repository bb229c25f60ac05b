// graph.hip - from an unordered list of undirected pairs to per-row neighbour lists, and the best k of every list
// (include/lshrs_graph.h; lshrs_amd/_knn_join.py): what stands between the LSH self-join's candidate pairs and a k-NN graph.
//
//   degree    one lane per pair: degree[a] += 1, degree[b] += 1.
//   fill      one lane per pair: b into a slot of a's list that an add on cursor[a] reserves, a into b's likewise.  The order
//             inside a list is the order the lanes arrived in.
//   select    per row the best k entries of its list by (key of the score, id): a bitonic network over 16-byte items in LDS -
//             one WAVE per list of at most kWaveList entries, one WORKGROUP per longer list.  The id breaks every tie, so the
//             answer does not depend on the order fill left.
//
// The library stands alone: no symbol of liblshrs_hip.so or liblshrs_groups.so.
#include "lshrs_graph.h"
#include "lshrs_lists.h"
#include "lshrs_rows.h"

namespace {

using namespace lshrs;                             // (lshrs_lists.h: the layers shared with refine, groups and join; desc_key)

constexpr int64_t kMaxCount = 0x7fffffffLL;        // rows and pairs: a degree is an int32
constexpr int kWaveList = 256;                     // the longest list one wave sorts: 4 KiB of LDS per wave, 16 KiB per workgroup
constexpr int kMaxList = 4096;                     // the longest list a workgroup sorts: 64 KiB, two workgroups per CU
constexpr int kLongBlocksPerCu = 2;
constexpr uint32_t kNanBits = 0x7fc00000u;
#ifndef LSHRS_GRAPH_COMBINE
#define LSHRS_GRAPH_COMBINE 0
#endif
constexpr bool kCombine = LSHRS_GRAPH_COMBINE != 0;   // equal addresses of a wave combined before the atomic (see reserve)

// One unit added to counter[row] for every lane that is `active`; each such lane gets the value its own unit found there.
// Every lane of the wave calls it.  Plain: one atomicAdd per lane.  COMBINE: the lanes that name the same row are found round
// by round - the first lane still waiting is the leader, its row is broadcast, the lanes that hold it are counted by a
// ballot - and the leader adds their number once; a round retires at least its leader, so 64 rounds bound the loop.
template <bool COMBINE>
__device__ __forceinline__ int reserve(int32_t* counter, int64_t row, bool active) {
  if (!COMBINE) return active ? atomicAdd(counter + row, 1) : 0;
  const int lane = threadIdx.x & 63;
  int slot = 0;
  uint64_t todo = __ballot(active);
  for (int round = 0; round < 64 && todo; ++round) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int64_t named = __shfl(row, leader);
    const bool mine = active && row == named;
    const Places group = places_of(mine);         // (its leader is `leader`: the first lane waiting holds the row it names)
    int base = 0;
    if (lane == leader) base = atomicAdd(counter + row, group.count());
    base = __shfl(base, leader);
    if (mine) slot = base + group.rank();
    todo &= ~group.flagged;
  }
  return slot;
}

__device__ __forceinline__ bool pair_ok(int64_t ea, int64_t eb, int64_t n_rows, int& bad) {
  if ((uint64_t)ea >= (uint64_t)n_rows || (uint64_t)eb >= (uint64_t)n_rows) {
    bad |= LSHRS_GRAPH_ERR_ENDPOINT;
    return false;
  }
  if (ea == eb) {
    bad |= LSHRS_GRAPH_ERR_LOOP;
    return false;
  }
  return true;
}

__global__ __launch_bounds__(kThreads) void degree_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b,
                                                          int64_t n_pairs, int64_t n_rows, int32_t* degree, int32_t* err) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int bad = 0;
  int64_t ea = 0, eb = 0;
  bool ok = false;
  if (p < n_pairs) {
    ea = a[p];
    eb = b[p];
    ok = pair_ok(ea, eb, n_rows, bad);
  }
  reserve<kCombine>(degree, ea, ok);
  reserve<kCombine>(degree, eb, ok);
  report(err, bad);
}

__global__ __launch_bounds__(kThreads) void fill_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b,
                                                        int64_t n_pairs, int64_t n_rows, const int64_t* __restrict__ row_off,
                                                        int32_t* cursor, int64_t* __restrict__ nbr) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int bad = 0;
  int64_t ea = 0, eb = 0;
  bool ok = false;
  if (p < n_pairs) {
    ea = a[p];
    eb = b[p];
    ok = pair_ok(ea, eb, n_rows, bad);
  }
  const int at_a = reserve<kCombine>(cursor, ea, ok);
  const int at_b = reserve<kCombine>(cursor, eb, ok);
  if (ok) {
    // a slot inside its row's list AND inside nbr's 2 n_pairs entries, or no store
    const int64_t sa = row_off[ea] + at_a, sb = row_off[eb] + at_b;
    if (sa >= row_off[ea] && sa < row_off[ea + 1] && (uint64_t)sa < (uint64_t)(2 * n_pairs)) nbr[sa] = eb;
    if (sb >= row_off[eb] && sb < row_off[eb + 1] && (uint64_t)sb < (uint64_t)(2 * n_pairs)) nbr[sb] = ea;
  }
}

// ------------------------------------------------------------------------------------------
// select: the sort item and the network
// ------------------------------------------------------------------------------------------
// An item, compared as the 128-bit number {hi, lo}: the descending key of the score, then the id (its sign bit flipped, so that
// the unsigned order is the signed one), then the position in the list - which decides nothing between entries of different
// ids and is what the score is read back through.  The padding of a list to the network's size is all ones: behind every
// real item, whose position is below 2^32 - 1.
struct __attribute__((aligned(16))) Item {
  uint64_t hi, lo;
};
__device__ __forceinline__ Item make_item(float score, int64_t id, uint32_t pos) {
  const uint64_t uid = (uint64_t)id ^ 0x8000000000000000ull;
  return Item{((uint64_t)desc_key(score) << 32) | (uid >> 32), (uid << 32) | pos};
}
__device__ __forceinline__ Item pad_item() { return Item{~0ull, ~0ull}; }
__device__ __forceinline__ int64_t item_id(const Item& x) {
  return (int64_t)((((x.hi & 0xffffffffull) << 32) | (x.lo >> 32)) ^ 0x8000000000000000ull);
}
__device__ __forceinline__ bool behind(const Item& x, const Item& y) { return x.hi > y.hi || (x.hi == y.hi && x.lo > y.lo); }

// The ascending bitonic network over items[0, n), n a power of two, by THREADS threads of which this is thread t.
template <int THREADS, bool WAVE>
__device__ __forceinline__ void sort_items(Item* items, int n, int t) {
  for (int size = 2; size <= n; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < (n >> 1); i += THREADS) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const Item x = items[lo], y = items[hi];
        if (behind(x, y) == up) {
          items[lo] = y;
          items[hi] = x;
        }
      }
      pass_done<WAVE>();
    }
}

struct SelectArgs {
  const int64_t* nbr;
  const float* scores;
  const int64_t* row_off;
  int64_t n_rows, total;
  const int64_t* row_ids;
  int64_t n_ids;
  int k;
  int64_t* out_ids;
  float* out_scores;
  int32_t* out_count;
  int32_t* err;
};


// One list of `len` <= the network's capacity, by THREADS threads (this one: t): loaded as items, sorted, the best
// min(k, len) written out and the tail padded.
template <int THREADS, bool WAVE>
__device__ __forceinline__ void select_list(const SelectArgs& s, Item* items, int64_t row, int64_t begin, int len, int t,
                                            int& bad) {
  int n = 1;
  while (n < len) n <<= 1;
  for (int i = t; i < n; i += THREADS) {
    Item it = pad_item();
    if (i < len) {
      const int64_t nb = s.nbr[begin + i];
      int64_t id = nb;
      if (s.row_ids != nullptr) {
        if ((uint64_t)nb < (uint64_t)s.n_ids) {
          id = s.row_ids[nb];
        } else {
          id = -1;
          bad |= LSHRS_GRAPH_ERR_ENTRY;
        }
      }
      it = make_item(s.scores[begin + i], id, (uint32_t)i);
    }
    items[i] = it;
  }
  pass_done<WAVE>();
  sort_items<THREADS, WAVE>(items, n, t);
  const int count = len < s.k ? len : s.k;
  int64_t* oi = s.out_ids + row * s.k;
  float* os = s.out_scores + row * s.k;
  for (int i = t; i < s.k; i += THREADS) {
    if (i < count) {
      const Item it = items[i];
      oi[i] = item_id(it);
      os[i] = s.scores[begin + (uint32_t)it.lo];
    } else {
      oi[i] = -1;
      os[i] = __uint_as_float(kNanBits);
    }
  }
  if (t == 0) s.out_count[row] = count;
  pass_done<WAVE>();                  // (the items are read: the slice may be loaded again)
}

// Lists of at most kWaveList entries: one wave per row, four rows per workgroup, no workgroup barrier.
__global__ __launch_bounds__(kThreads) void select_wave_kernel(SelectArgs s) {
  __shared__ Item slices[kWavesPerGroup][kWaveList];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kWavesPerGroup + wave;
  int bad = 0;
  if (row < s.n_rows) {               // (uniform in the wave)
    int64_t begin;
    const int64_t len = list_of(s, row, begin, bad, LSHRS_GRAPH_ERR_RANGE);
    if (len <= kWaveList) select_list<64, true>(s, slices[wave], row, begin, (int)len, lane, bad);
  }
  report(s.err, bad);
}

// Longer lists: the workgroups walk the rows (walk_rows) - a thread notes its row where its list is long - and sort the noted
// rows one after the other.  A list beyond kMaxList gets its -1 and nothing else.
__global__ __launch_bounds__(kThreads) void select_long_kernel(SelectArgs s) {
  extern __shared__ __attribute__((aligned(16))) unsigned char graph_lds[];
  int* noted = reinterpret_cast<int*>(graph_lds + (size_t)kMaxList * sizeof(Item));     // (walk_rows: the noted rows)
  int bad = 0;
  walk_rows<kThreads, false>(
      s, noted,
      [](const SelectArgs& s, int64_t row, int&) {
        int64_t begin;
        int unused = 0;               // (a list out of range is the wave kernel's to report)
        return list_of(s, row, begin, unused, LSHRS_GRAPH_ERR_RANGE) > kWaveList;
      },
      [&bad](const SelectArgs& s, int64_t row, int) {
        int64_t begin;
        int unused = 0;
        const int64_t len = list_of(s, row, begin, unused, LSHRS_GRAPH_ERR_RANGE);
        if (len > kMaxList) {
          if (threadIdx.x == 0) s.out_count[row] = -1;
        } else {
          select_list<kThreads, false>(s, reinterpret_cast<Item*>(graph_lds), row, begin, (int)len, threadIdx.x, bad);
        }
      });
  report(s.err, bad);
}

constexpr size_t kLongLds = (size_t)kMaxList * sizeof(Item) + (kWalkInts<kThreads, false> + 3) * sizeof(int);

}  // namespace

extern "C" {

int lshrs_graph_abi_version(void) { return LSHRS_GRAPH_ABI_VERSION; }
int32_t lshrs_graph_max_list(void) { return kMaxList; }
int32_t lshrs_graph_wave_list(void) { return kWaveList; }

int lshrs_graph_degree_i64(const int64_t* a, const int64_t* b, int64_t n_pairs, int64_t n_rows, int32_t* degree, int32_t* err,
                           void* stream) {
  if (n_pairs < 0 || n_rows < 0) return LSHRS_E_BADARG;
  if (n_pairs > kMaxCount || n_rows > kMaxCount) return LSHRS_E_TOOLARGE;
  if (n_pairs == 0 || n_rows == 0) return 0;
  if (!usable(a, 8) || !usable(b, 8) || !usable(degree, 4) || !usable(err, 4)) return LSHRS_E_BADARG;
  hipLaunchKernelGGL(degree_kernel, dim3(blocks_for(n_pairs, kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a,
                     b, n_pairs, n_rows, degree, err);
  return -(int)hipGetLastError();
}

int lshrs_graph_fill_i64(const int64_t* a, const int64_t* b, int64_t n_pairs, int64_t n_rows, const int64_t* row_off,
                         int32_t* cursor, int64_t* nbr, void* stream) {
  if (n_pairs < 0 || n_rows < 0) return LSHRS_E_BADARG;
  if (n_pairs > kMaxCount || n_rows > kMaxCount) return LSHRS_E_TOOLARGE;
  if (n_pairs == 0 || n_rows == 0) return 0;
  if (!usable(a, 8) || !usable(b, 8) || !usable(row_off, 8) || !usable(cursor, 4) || !usable(nbr, 8)) return LSHRS_E_BADARG;
  hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(n_pairs, kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a, b,
                     n_pairs, n_rows, row_off, cursor, nbr);
  return -(int)hipGetLastError();
}

int lshrs_graph_select_f32(const int64_t* nbr, const float* scores, const int64_t* row_off, int64_t n_rows, int64_t total,
                           const int64_t* row_ids, int64_t n_ids, int32_t k, int64_t* out_ids, float* out_scores,
                           int32_t* out_count, int32_t* err, void* stream) {
  if (n_rows < 0 || total < 0 || k < 1 || (row_ids != nullptr && n_ids < 0)) return LSHRS_E_BADARG;
  if (n_rows > kMaxCount) return LSHRS_E_TOOLARGE;
  if (n_rows == 0) return 0;
  if (!usable(row_off, 8) || !usable(out_ids, 8) || !usable(out_scores, 4) || !usable(out_count, 4) || !usable(err, 4))
    return LSHRS_E_BADARG;
  if (total > 0 && (!usable(nbr, 8) || !usable(scores, 4))) return LSHRS_E_BADARG;
  if (row_ids != nullptr && !usable(row_ids, 8)) return LSHRS_E_BADARG;
  const SelectArgs args{nbr, scores, row_off, n_rows, total, row_ids, n_ids, k, out_ids, out_scores, out_count, err};
  return launch_tiers(select_wave_kernel, select_long_kernel, args, n_rows, kLongLds, kLongBlocksPerCu, stream);
}

}  // extern "C"
