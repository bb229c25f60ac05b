// bitonic_pass.inc - the one text of a compare-exchange pass of the ASCENDING bitonic network over 64-bit items in LDS: every
// pair at distance `stride` of merge size `size`, by all threads of the workgroup, and the barrier behind it.  Not a translation
// unit and not a header: statements, #included where they run - topk_kernel and topk_local_kernel (rerank.hip), the fall-through
// of bitonic_sort_lds (query.hip).  Included, not called, for scan_pass.inc's reason: as a function the pass compiled to other
// instructions in every kernel that runs it (the function is canonicalised on its own before it is inlined).
// The including scope provides: uint64_t* items (LDS), n (their number, a power of two), size, stride, base and kPassThreads
// (the workgroup's threads).  The direction of a pair follows its GLOBAL index base + lo: base is where these n items stand in
// a longer array (a chunk of the global network), else a constant 0.
for (int t = threadIdx.x; t < (n >> 1); t += kPassThreads) {
  const int lo = 2 * t - (t & (stride - 1));
  const int hi = lo + stride;
  const bool up = (((base + lo) & size) == 0);
  const uint64_t a = items[lo], b = items[hi];
  if ((a > b) == up) {
    items[lo] = b;
    items[hi] = a;
  }
}
__syncthreads();
