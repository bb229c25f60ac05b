// lshrs_lists.h - what the kernels over per-row lists share (graph.hip, refine.hip, groups.hip, join.hip), each layer stated once:
// the wave's error report, the wait between two passes over LDS, a row's list out of its offsets, the places a wave's flagged
// lanes get behind one add, the workgroup tier's walk over the rows - and on the host the pointer check, the grid sizes and
// the launch of the two tiers.  What a kernel DOES with a list - the network, the hash set, the forest - stays in its file.
// Everything is inline (no state, nothing exported) and needs nothing but the HIP runtime: a library that includes this
// still stands alone.
#ifndef LSHRS_LISTS_H
#define LSHRS_LISTS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lshrs {

constexpr int kThreads = 256;                      // four wave64 per workgroup
constexpr int kWavesPerGroup = kThreads / 64;

// the bits of a wave's lanes or-ed into err by one lane; every lane of the wave calls it
__device__ __forceinline__ void report(int32_t* err, int bad) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) bad |= __shfl_xor(bad, off);
  if ((threadIdx.x & 63) == 0 && bad) atomicOr(err, bad);
}

// What the threads that share a piece of LDS wait with between two passes over it.  A wave on its own slice of LDS needs no
// barrier: its LDS instructions execute in order; the fences keep the compiler from moving a pass's reads above the stores
// before it.
template <bool WAVE>
__device__ __forceinline__ void pass_done() {
  if (WAVE) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  } else {
    __syncthreads();
  }
}

// The list of a row of s (its row_off, its total): where it begins and how long it is; a list that does not lie within
// [0, total] is empty and reported with `bit`.
template <class Args>
__device__ __forceinline__ int64_t list_of(const Args& s, int64_t row, int64_t& begin, int& bad, int bit) {
  begin = s.row_off[row];
  const int64_t end = s.row_off[row + 1];
  if (begin < 0 || end < begin || end > s.total) {
    bad |= bit;
    begin = 0;
    return 0;
  }
  return end - begin;
}

// The flagged lanes of a wave get consecutive places behind ONE add by their leader: who is flagged, the first of them, how
// many they are, and how many of them stand below this lane.  Every lane of the wave calls places_of; the add - its target,
// its width - is the caller's.
struct Places {
  uint64_t flagged;
  __device__ __forceinline__ int leader() const { return __ffsll((unsigned long long)flagged) - 1; }
  __device__ __forceinline__ int count() const { return (int)__popcll(flagged); }
  __device__ __forceinline__ int rank() const { return (int)__popcll(flagged & ((1ull << (threadIdx.x & 63)) - 1ull)); }
};
__device__ __forceinline__ Places places_of(bool flag) { return Places{__ballot(flag)}; }

// The workgroup tier of a kernel over the rows of s (its n_rows): the workgroups walk the rows THREADS at a time.  A thread looks
// at one row and notes it where classify(s, row, keep) says it is the workgroup's - with KEEP, together with the int classify
// left in `keep`; the noted rows are then worked one after the other, work(s, row, kept) by all threads, in the order the
// notes arrived in.  `noted` is LDS of the caller's: [THREADS] rows, with KEEP [THREADS] ints behind them, then their number -
// kWalkInts<THREADS, KEEP> ints.  Every thread of the workgroup calls it.
// s goes through by value and the callables name it as their parameter, LDS by its symbol and nothing by a pointer they
// captured: the walk is optimised on its own before it is inlined, and so what it hoists out of the loop is what - and in
// the order - a kernel with the loop written out hoists.
template <int THREADS, bool KEEP>
constexpr int kWalkInts = THREADS * (KEEP ? 2 : 1) + 1;

template <int THREADS, bool KEEP, class Args, class Classify, class Work>
__device__ __forceinline__ void walk_rows(const Args s, int* noted, Classify classify, Work work) {
  int* kept = noted + THREADS;
  int* n_noted = noted + kWalkInts<THREADS, KEEP> - 1;
  for (int64_t base = (int64_t)blockIdx.x * THREADS; base < s.n_rows; base += (int64_t)gridDim.x * THREADS) {
    if (threadIdx.x == 0) *n_noted = 0;
    __syncthreads();
    const int64_t mine = base + threadIdx.x;
    int keep = 0;
    if (mine < s.n_rows && classify(s, mine, keep)) {
      const int at = atomicAdd(n_noted, 1);
      noted[at] = threadIdx.x;
      if (KEEP) kept[at] = keep;
    }
    __syncthreads();
    const int todo = *n_noted;
    for (int j = 0; j < todo; ++j) work(s, base + noted[j], KEEP ? kept[j] : 0);
    __syncthreads();                  // (noted[] is read: the next THREADS rows may be noted)
  }
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
inline bool usable(const void* p, uintptr_t align) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & (align - 1)) == 0; }
inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// The grid of a kernel whose workgroups stride: min(wanted, CUs x per_cu), all of it resident at once.
inline hipError_t resident_grid(int64_t wanted, int per_cu, unsigned& blocks) {
  int device = 0, cus = 0;
  hipError_t rc = hipGetDevice(&device);
  if (rc == hipSuccess) rc = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  const int64_t resident = (int64_t)(cus > 0 ? cus : 1) * per_cu;
  blocks = (unsigned)(wanted < resident ? wanted : resident);
  return rc;
}

// Both launches of a kernel family over rows: the wave kernel over all rows, one row per wave, and the workgroup kernel - with
// long_lds bytes of dynamic LDS - on a resident grid of at most blocks_per_cu workgroups per CU.
template <class Args>
inline int launch_tiers(void (*wave_kernel)(Args), void (*long_kernel)(Args), const Args& args, int64_t n_rows, size_t long_lds,
                        int blocks_per_cu, void* stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long_blocks = 0;
  hipError_t rc = resident_grid(blocks_for(n_rows, kThreads), blocks_per_cu, long_blocks);
  if (rc == hipSuccess)
    rc = hipFuncSetAttribute(reinterpret_cast<const void*>(long_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)long_lds);
  if (rc != hipSuccess) return -(int)rc;
  hipLaunchKernelGGL(wave_kernel, dim3(blocks_for(n_rows, kWavesPerGroup)), dim3(kThreads), 0, s, args);
  hipLaunchKernelGGL(long_kernel, dim3(long_blocks), dim3(kThreads), long_lds, s, args);
  return -(int)hipGetLastError();
}

}  // namespace lshrs

#endif  // LSHRS_LISTS_H
