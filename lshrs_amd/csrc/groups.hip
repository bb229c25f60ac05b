// groups.hip - connected components of an edge list (include/lshrs_groups.h; lshrs_amd/_groups.py): a union-find forest over
// dense vertices, built by lanes that race and still end in ONE result - the smallest vertex of every component.
//
//   init      parent[x] = x.
//   hook      one lane per edge (grid-stride, the grid sized to the device): the two roots by walks with path halving, the
//             larger root hung under the smaller by a compare-and-swap of its own entry from itself; a lost race goes on from
//             what the swap returned.
//   flatten   lane x alone writes parent[x], two levels up at a time, until it names a root.
//
// parent[x] <= x at every moment, so every walk descends strictly and its steps are bounded by where it started: the caps below
// are those bounds plus a constant, and a lane that passes one reports it (err bit 1) and leaves.  Inside hook and flatten
// every access to `parent` is an agent-scope relaxed atomic: the L2 of an XCD is not coherent with the others', and a stale
// value - an earlier ancestor - costs steps, never the result.  The library stands alone: no symbol of liblshrs_hip.so.
#include "lshrs_groups.h"
#include "lshrs_lists.h"

namespace {

using namespace lshrs;                             // (lshrs_lists.h: the layers shared with graph, refine and join)

constexpr int kBlocksPerCu = 8;                    // 2048 lanes per CU: every wave slot of its SIMDs
constexpr int64_t kMaxVertices = 0x7fffffffLL;     // a vertex is an int32
constexpr int64_t kCapSlack = 16;
constexpr int kErrEndpoint = LSHRS_CC_ERR_ENDPOINT, kErrCap = LSHRS_CC_ERR_CAP;

__device__ __forceinline__ int32_t ld(const int32_t* parent, int64_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st(int32_t* parent, int64_t x, int32_t v) {
  __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A vertex that was the root of x's tree when its entry was read, by a walk with path halving: parent[x] = its grandparent,
// then on from there.  x descends strictly; every step is taken off `budget`, and -1 comes back when that is used up - or when
// an entry is not in [0, its index], which no forest of init and hook holds: nothing is ever read outside [0, x].
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x, int64_t& budget) {
  for (;;) {
    const int32_t p = ld(parent, x);
    if (p == x) return x;
    if ((uint32_t)p > (uint32_t)x) return -1;
    const int32_t gp = ld(parent, p);
    if (gp == p) return p;
    if ((uint32_t)gp > (uint32_t)p || --budget < 0) return -1;
    st(parent, x, gp);            // (x is no root and never will be again: only an ancestor is stored)
    x = gp;
  }
}

__global__ __launch_bounds__(kThreads) void cc_init_kernel(int32_t* __restrict__ parent, int64_t n) {
  const int64_t x = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (x < n) parent[x] = (int32_t)x;
}

__global__ __launch_bounds__(kThreads) void cc_hook_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b,
                                                           int64_t n_edges, int32_t* parent, int64_t n, int32_t* err) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int bad = 0;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n_edges; e += stride) {
    const int64_t ea = a[e], eb = b[e];
    if ((uint64_t)ea >= (uint64_t)n || (uint64_t)eb >= (uint64_t)n) {
      bad |= kErrEndpoint;
      continue;
    }
    // u and v only ever descend - by the steps of a walk, or to what a lost swap returned - and each descent is one unit
    // of the budget: u + v < 2 n bounds them all
    int32_t u = (int32_t)ea, v = (int32_t)eb;
    int64_t budget = 2 * n + kCapSlack;
    for (;;) {
      u = find_root(parent, u, budget);
      if (u < 0) break;
      v = find_root(parent, v, budget);
      if (v < 0 || u == v) break;
      const int32_t hi = u > v ? u : v, lo = u > v ? v : u;
      int32_t seen = hi;
      if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        break;
      // hi has been hung under `seen` meanwhile (seen < hi): on from there
      if (--budget < 0 || seen >= hi) {
        u = -1;
        break;
      }
      if (u == hi) u = seen;
      else v = seen;
    }
    if (u < 0 || v < 0) bad |= kErrCap;
  }
  report(err, bad);
}

__global__ __launch_bounds__(kThreads) void cc_flatten_kernel(int32_t* parent, int64_t n, int32_t* err) {
  const int64_t x = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int bad = 0;
  if (x < n) {
    int32_t p = ld(parent, x);
    bool done = false;
    // (an entry outside [0, its index] is in no forest of init and hook: such a walk is given up before it reads outside)
    for (int64_t it = 0; it < n + kCapSlack && (uint32_t)p <= (uint32_t)x; ++it) {
      const int32_t gp = ld(parent, p);
      if (gp == p) {
        done = true;
        break;
      }
      if ((uint32_t)gp > (uint32_t)p) break;
      st(parent, x, gp);
      p = gp;
    }
    if (!done) bad = kErrCap;
  }
  report(err, bad);
}

}  // namespace

extern "C" {

int lshrs_groups_abi_version(void) { return LSHRS_GROUPS_ABI_VERSION; }

int lshrs_cc_init_i32(int32_t* parent, int64_t n, void* stream) {
  if (n < 0) return LSHRS_E_BADARG;
  if (n > kMaxVertices) return LSHRS_E_TOOLARGE;
  if (n == 0) return 0;
  if (!usable(parent, 4)) return LSHRS_E_BADARG;
  hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), parent, n);
  return -(int)hipGetLastError();
}

int lshrs_cc_hook_i64(const int64_t* a, const int64_t* b, int64_t n_edges, int32_t* parent, int64_t n, int32_t* err,
                      void* stream) {
  if (n < 0 || n_edges < 0) return LSHRS_E_BADARG;
  if (n > kMaxVertices) return LSHRS_E_TOOLARGE;
  if (n == 0 || n_edges == 0) return 0;
  if (!usable(a, 8) || !usable(b, 8) || !usable(parent, 4) || !usable(err, 4)) return LSHRS_E_BADARG;
  unsigned blocks = 0;
  const hipError_t rc = resident_grid(blocks_for(n_edges, kThreads), kBlocksPerCu, blocks);
  if (rc != hipSuccess) return -(int)rc;
  hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a, b, n_edges, parent, n,
                     err);
  return -(int)hipGetLastError();
}

int lshrs_cc_flatten_i32(int32_t* parent, int64_t n, int32_t* err, void* stream) {
  if (n < 0) return LSHRS_E_BADARG;
  if (n > kMaxVertices) return LSHRS_E_TOOLARGE;
  if (n == 0) return 0;
  if (!usable(parent, 4) || !usable(err, 4)) return LSHRS_E_BADARG;
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, static_cast<hipStream_t>(stream), parent, n, err);
  return -(int)hipGetLastError();
}

}  // extern "C"
