// idmap.hip - the id -> row table of a device-resident vector store (lshrs_amd/vectors.py: DeviceVectors).
//
// An open-addressing hash table in device memory from non-negative int64 ids to row numbers of the store's row block.  One
// slot is 16 bytes {int64 id, int64 row}, so a probe is one 16-byte load; an empty slot has id = -1 (and row = -1: the
// caller fills a new table with 0xff bytes); `slots` is a power of two; probing is linear from lshrs::idmap_home(id).
//   * ids are never taken out of their slots: erase only sets the row to -1, a later insert of the id raises it again;
//   * rows only grow (atomicMax), so an id inserted several times - in one launch or across launches on one stream - ends
//     at its LATEST row in whatever order the lanes run;
//   * every probe loop runs at most `slots` steps and then answers "full" / "absent": no table makes a kernel spin.
// Lookups run behind the inserts of their stream (plain 16-byte loads); inserts, erases and rehashes use 64-bit atomics.
#include "lshrs_common.h"

namespace {

using namespace lshrs;

struct alignas(16) Slot {
  long long id;
  long long row;
};
static_assert(sizeof(Slot) == 16, "one probe = one 16-byte load");
typedef long long i64x2 __attribute__((ext_vector_type(2)));

constexpr int kIdmapThreads = 256;
constexpr int kErrMissing = 256;         // bit 8 of the rerank's error word: a candidate id without a stored vector

// 1 = the id took a free slot, 0 = it had one already, -1 = no slot left; *old_row: the row it had (-1: none / erased)
__device__ __forceinline__ int insert_one(Slot* table, int64_t slots, long long id, long long row, long long* old_row) {
  int64_t s = idmap_home(id, slots);
  for (int64_t p = 0; p < slots; ++p, s = (s + 1) & (slots - 1)) {
    long long cur = __hip_atomic_load(&table[s].id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int fresh = 0;
    if (cur == -1) {
      cur = (long long)atomicCAS(reinterpret_cast<unsigned long long*>(&table[s].id), ~0ULL, (unsigned long long)id);
      if (cur == -1) {
        fresh = 1;
        cur = id;
      }
    }
    if (cur == id) {
      *old_row = atomicMax(&table[s].row, row);
      return fresh;
    }
  }
  return -1;
}

__device__ __forceinline__ Slot* find_slot(Slot* table, int64_t slots, long long id) {
  if (id < 0) return nullptr;
  int64_t s = idmap_home(id, slots);
  for (int64_t p = 0; p < slots; ++p, s = (s + 1) & (slots - 1)) {
    const long long cur = __hip_atomic_load(&table[s].id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == id) return table + s;
    if (cur == -1) return nullptr;
  }
  return nullptr;
}

__device__ __forceinline__ long long find_row(const Slot* __restrict__ table, int64_t slots, long long id) {
  if (id < 0) return -1;
  int64_t s = idmap_home(id, slots);
  for (int64_t p = 0; p < slots; ++p, s = (s + 1) & (slots - 1)) {
    const i64x2 v = *reinterpret_cast<const i64x2*>(table + s);      // one 16-byte load: {id, row}
    if (v.x == id) return v.y;            // (-1: erased)
    if (v.x == -1) return -1;
  }
  return -1;
}

// the number of lanes of this workgroup for which `flag` holds, added to *counter by one lane
__device__ __forceinline__ void block_count(int flag, int32_t* counter) {
  const int n = __syncthreads_count(flag);
  if (threadIdx.x == 0 && n) atomicAdd(counter, n);
}

// report int32[4]: [0] += slots taken, [1] += ids that became live, [2] |= a negative id, [3] |= no free slot
__global__ __launch_bounds__(kIdmapThreads) void idmap_insert_kernel(Slot* table, int64_t slots, const int64_t* __restrict__ ids,
                                                                     int64_t n, int64_t first_row, int32_t* report) {
  const int64_t i = (int64_t)blockIdx.x * kIdmapThreads + threadIdx.x;
  int fresh = 0, live = 0, neg = 0, full = 0;
  if (i < n) {
    const long long id = ids[i];
    if (id < 0) {
      neg = 1;
    } else {
      long long old_row = 0;
      const int got = insert_one(table, slots, id, first_row + i, &old_row);
      fresh = got == 1;
      full = got < 0;
      live = got >= 0 && old_row < 0;
    }
  }
  block_count(fresh, report);
  block_count(live, report + 1);
  if (__syncthreads_or(neg) && threadIdx.x == 0) atomicOr(report + 2, 1);
  if (__syncthreads_or(full) && threadIdx.x == 0) atomicOr(report + 3, 1);
}

__global__ __launch_bounds__(kIdmapThreads) void idmap_erase_kernel(Slot* table, int64_t slots, const int64_t* __restrict__ ids,
                                                                    int64_t n, int32_t* live_count) {
  const int64_t i = (int64_t)blockIdx.x * kIdmapThreads + threadIdx.x;
  int was_live = 0;
  if (i < n) {
    Slot* s = find_slot(table, slots, ids[i]);
    if (s != nullptr) was_live = atomicExch(reinterpret_cast<unsigned long long*>(&s->row), ~0ULL) != ~0ULL;
  }
  block_count(was_live, live_count);
}

__global__ __launch_bounds__(kIdmapThreads) void idmap_lookup_kernel(const Slot* __restrict__ table, int64_t slots,
                                                                     const int64_t* __restrict__ ids, int64_t n,
                                                                     int64_t* __restrict__ rows, int32_t* err) {
  const int64_t i = (int64_t)blockIdx.x * kIdmapThreads + threadIdx.x;
  int miss = 0;
  if (i < n) {
    const long long r = find_row(table, slots, ids[i]);
    rows[i] = r;
    miss = r < 0;
  }
  if (err != nullptr && __syncthreads_or(miss) && threadIdx.x == 0) atomicOr(err, kErrMissing);
}

// grid (x, y): the workgroups of column y take queries y, y + gridDim.y, ...; those of one query stride over its list
__global__ __launch_bounds__(kIdmapThreads) void idmap_lookup_ragged_kernel(const Slot* __restrict__ table, int64_t slots,
                                                                            const int64_t* __restrict__ cand_ids,
                                                                            const int64_t* __restrict__ pair_off,
                                                                            const int32_t* __restrict__ ucount, int32_t q,
                                                                            int64_t* __restrict__ rows, int32_t* err) {
  int miss = 0;
  for (int32_t qi = blockIdx.y; qi < q; qi += gridDim.y) {
    const int32_t cnt = ucount[qi];
    if (cnt <= 0) continue;               // (< 0: a list beyond the collide step's capacity - nothing of it is there)
    const int64_t off = pair_off[qi];
    for (int64_t j = (int64_t)blockIdx.x * kIdmapThreads + threadIdx.x; j < cnt; j += (int64_t)gridDim.x * kIdmapThreads) {
      const long long r = find_row(table, slots, cand_ids[off + j]);
      rows[off + j] = r;
      miss |= r < 0;
    }
  }
  if (err != nullptr && __syncthreads_or(miss) && threadIdx.x == 0) atomicOr(err, kErrMissing);
}

// report as idmap_insert_kernel's ([1]: entries moved)
__global__ __launch_bounds__(kIdmapThreads) void idmap_rehash_kernel(const Slot* __restrict__ src, int64_t src_slots, Slot* dst,
                                                                     int64_t dst_slots, int32_t* report) {
  const int64_t i = (int64_t)blockIdx.x * kIdmapThreads + threadIdx.x;
  int fresh = 0, moved = 0, full = 0;
  if (i < src_slots) {
    const Slot v = src[i];
    if (v.id >= 0 && v.row >= 0) {
      long long old_row = 0;
      const int got = insert_one(dst, dst_slots, v.id, v.row, &old_row);
      fresh = got == 1;
      full = got < 0;
      moved = got >= 0;
    }
  }
  block_count(fresh, report);
  block_count(moved, report + 1);
  if (__syncthreads_or(full) && threadIdx.x == 0) atomicOr(report + 3, 1);
}

inline bool table_ok(const void* table, int64_t slots) {
  return table != nullptr && (reinterpret_cast<uintptr_t>(table) & 15) == 0 && idmap_slots_ok(slots);
}
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kIdmapThreads - 1) / kIdmapThreads); }
constexpr int64_t kIdmapMaxN = 0x7fffffffLL * kIdmapThreads;      // what a one-dimensional grid of 256-lane workgroups covers

}  // namespace

extern "C" {

int64_t lshrs_idmap_bytes(int64_t slots) {
  if (!idmap_slots_ok(slots) || slots > (INT64_MAX >> 4)) return LSHRS_E_BADARG;
  return 16 * slots;
}

int64_t lshrs_idmap_home_slot(int64_t id, int64_t slots) {
  if (id < 0 || !idmap_slots_ok(slots)) return LSHRS_E_BADARG;
  return idmap_home(id, slots);
}

int lshrs_idmap_insert_i64(void* table, int64_t slots, const int64_t* ids, int64_t n, int64_t first_row, int32_t* report,
                           void* stream) {
  if (!table_ok(table, slots) || ids == nullptr || report == nullptr || n < 0 || first_row < 0) return LSHRS_E_BADARG;
  if (n > kIdmapMaxN || first_row > INT64_MAX - n) return LSHRS_E_TOOLARGE;
  if (n == 0) return 0;
  hipLaunchKernelGGL(idmap_insert_kernel, dim3(blocks_for(n)), dim3(kIdmapThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<Slot*>(table), slots, ids, n, first_row, report);
  return -(int)hipGetLastError();
}

int lshrs_idmap_erase_i64(void* table, int64_t slots, const int64_t* ids, int64_t n, int32_t* live_count, void* stream) {
  if (!table_ok(table, slots) || ids == nullptr || live_count == nullptr || n < 0) return LSHRS_E_BADARG;
  if (n > kIdmapMaxN) return LSHRS_E_TOOLARGE;
  if (n == 0) return 0;
  hipLaunchKernelGGL(idmap_erase_kernel, dim3(blocks_for(n)), dim3(kIdmapThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<Slot*>(table), slots, ids, n, live_count);
  return -(int)hipGetLastError();
}

int lshrs_idmap_lookup_i64(const void* table, int64_t slots, const int64_t* ids, int64_t n, int64_t* rows, int32_t* err,
                           void* stream) {
  if (!table_ok(table, slots) || ids == nullptr || rows == nullptr || n < 0) return LSHRS_E_BADARG;
  if (n > kIdmapMaxN) return LSHRS_E_TOOLARGE;
  if (n == 0) return 0;
  hipLaunchKernelGGL(idmap_lookup_kernel, dim3(blocks_for(n)), dim3(kIdmapThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const Slot*>(table), slots, ids, n, rows, err);
  return -(int)hipGetLastError();
}

int lshrs_idmap_lookup_ragged_i64(const void* table, int64_t slots, const int64_t* cand_ids, const int64_t* pair_off,
                                  const int32_t* ucount, int32_t q, int64_t total, int64_t* rows, int32_t* err,
                                  void* stream) {
  if (!table_ok(table, slots) || cand_ids == nullptr || pair_off == nullptr || ucount == nullptr || rows == nullptr ||
      q < 0 || total < 0)
    return LSHRS_E_BADARG;
  if (q == 0 || total == 0) return 0;
  // workgroups per query from the AVERAGE list (as lshrs_cosine_ragged_*: `total` sizes the launch only); a longer list is
  // walked in strides
  const int64_t avg = (total + q - 1) / q;
  int64_t bx = (avg + kIdmapThreads - 1) / kIdmapThreads;
  bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
  const dim3 grid((unsigned)bx, (unsigned)(q < 65535 ? q : 65535));
  hipLaunchKernelGGL(idmap_lookup_ragged_kernel, grid, dim3(kIdmapThreads), 0, static_cast<hipStream_t>(stream),
                     static_cast<const Slot*>(table), slots, cand_ids, pair_off, ucount, q, rows, err);
  return -(int)hipGetLastError();
}

int lshrs_idmap_rehash(const void* src, int64_t src_slots, void* dst, int64_t dst_slots, int32_t* report, void* stream) {
  if (!table_ok(src, src_slots) || !table_ok(dst, dst_slots) || src == dst || report == nullptr) return LSHRS_E_BADARG;
  if (src_slots > kIdmapMaxN) return LSHRS_E_TOOLARGE;
  hipLaunchKernelGGL(idmap_rehash_kernel, dim3(blocks_for(src_slots)), dim3(kIdmapThreads), 0,
                     static_cast<hipStream_t>(stream), static_cast<const Slot*>(src), src_slots, static_cast<Slot*>(dst),
                     dst_slots, report);
  return -(int)hipGetLastError();
}

}  // extern "C"
