// scan_pass.inc - the one text of a workgroup's pass in scan.hip: 256 rows from `base` (64 per wave, two 32-row tiles) against
// the query tile's image, all chunks of k.  Not a translation unit and not a header: statements, #included where they run
// (inline in scan_kernel's row loop, and as the body of scan_pass()).
// The including scope provides: E, ALIGNED, T, kTwo, kBTerms; corpus, ldc, dim, nchunks, row_ids, bimg, bl; base, row_begin,
// row_end; tid, lane, wave, r, h; and, declared but not set, bool live[2], int64_t row0[2], f32x16 acc[2][2], float nn[2].
// kBTerms: the terms the image holds per query element - 2 (hi and mid: f32 queries), or 1 (hi only: the self-join of a
// one-term corpus, whose queries are exact in bf16; their mid term is zero and its MFMA is not issued).
// It leaves acc[t][cb] (the dot products of tile t with column block cb), nn[t] (this lane's half of ||row||^2), live[t] and
// row0[t] (the tile's first row).  Every thread of the workgroup runs it (it synchronises on the B chunk in LDS, `bl`).
const T* rowp[2];
#pragma unroll
for (int t = 0; t < 2; ++t) {
  row0[t] = base + wave * 64 + t * 32;
  const int64_t row = row0[t] + r;
  const bool valid = row < row_end;
  live[t] = valid && (row_ids == nullptr || row_ids[row] >= 0);
  rowp[t] = corpus + (valid ? row : row_begin) * ldc;      // (a row past the end reads the slice's first row, unused)
}
#pragma unroll
for (int t = 0; t < 2; ++t)
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][cb][i] = 0.f;
nn[0] = nn[1] = 0.f;

// chunk c + 1's rows and B fragments are asked for before chunk c is multiplied, so that the loads fly under the MFMAs
constexpr int kBVecs = 2 * kBTerms;                        // 16-byte vectors of a B chunk a thread stages
constexpr int kBChunkVecs = kBVecs * kScanThreads;         // ... and the chunk holds
auto load_chunk = [&](int c, ScanRaw<E> (&raw)[2], u32x4 (&bst)[kBVecs]) {
  const int k0 = c * kScanKChunk + 32 * h;
  if (ALIGNED && (c + 1) * kScanKChunk <= dim) {
#pragma unroll
    for (int t = 0; t < 2; ++t) raw[t] = scan_load_vec<E>(rowp[t] + k0);
  } else {
#pragma unroll
    for (int t = 0; t < 2; ++t) raw[t] = scan_load_elems<E>(rowp[t], k0, dim);
  }
#pragma unroll
  for (int i = 0; i < kBVecs; ++i) bst[i] = bimg[(int64_t)c * kBChunkVecs + i * kScanThreads + tid];
};
// (one-term rows only: a two-term row's fragments leave no registers for a second chunk)
constexpr bool kAhead = !kTwo;
ScanRaw<E> nraw[2];
u32x4 nbst[kBVecs];
if constexpr (kAhead) load_chunk(0, nraw, nbst);
for (int c = 0; c < nchunks; ++c) {
  if constexpr (!kAhead) load_chunk(c, nraw, nbst);
  ScanRaw<E> raw[2] = {nraw[0], nraw[1]};
  __syncthreads();                    // the last chunk's fragments have been read
#pragma unroll
  for (int i = 0; i < kBVecs; ++i) bl[i * kScanThreads + tid] = nbst[i];
  __syncthreads();
  if constexpr (kAhead)
    if (c + 1 < nchunks) load_chunk(c + 1, nraw, nbst);

  u32x4 ahi[2][4], amid[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t) scan_fragments<E>(raw[t], ahi[t], amid[t], nn[t]);
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const bf16x8 bh = __builtin_bit_cast(bf16x8, bl[((0 * 4 + s) * 2 + cb) * 64 + lane]);
      bf16x8 bm;
      if constexpr (kBTerms == 2) bm = __builtin_bit_cast(bf16x8, bl[((1 * 4 + s) * 2 + cb) * 64 + lane]);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8 ah = __builtin_bit_cast(bf16x8, ahi[t][s]);
        acc[t][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t][cb], 0, 0, 0);
        if constexpr (kBTerms == 2) acc[t][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[t][cb], 0, 0, 0);
        if constexpr (kTwo)
          acc[t][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, amid[t][s]), bh, acc[t][cb], 0, 0, 0);
      }
    }
}
