// sig_split.hip - part of liblshrs_hip.so, the gfx950 (MI355X / CDNA4) implementation of the lshrs hot path.
// The split-precision signature pass as the C ABI offers it: stage 1 (sig16.hip / sig16r.hip) + stage 2 (sig_replay.hip) on
// one stream, with the tie replay; the library's version and build flags.
// One translation unit per kernel family (round 5): what is shared lives in lshrs_common.h, measurement switches (-DLSHRS_AB_*,
// tools/ab_build.py) are local to the unit whose kernel they alter and reported through lshrs_build_flags().
// ABI and reference citations: include/lshrs_hip.h.  Design notes: DESIGN.md.
#include "lshrs_common.h"

#include <chrono>
#include <cstdlib>

using namespace lshrs;

extern "C" {

int lshrs_abi_version(void) { return LSHRS_ABI_VERSION; }

// Which measurement switches this build was compiled with (include/lshrs_hip.h, LSHRS_BUILD_*): every translation unit
// reports its own; the product build returns 0.
// LSHRS_SIG16_HALF_MAX_TILES (sig16_half_rows below) is no compile-time switch, but a set variable changes which workgroup
// shape every measurement of the process is taken on: reported as LSHRS_BUILD_TUNED with bit 25.
static int sig16_half_forced() {
  static const int forced = [] {
    const char* e = std::getenv("LSHRS_SIG16_HALF_MAX_TILES");
    return e != nullptr ? std::atoi(e) : -1;
  }();
  return forced;
}

uint32_t lshrs_build_flags(void) {
  return lshrs_flags_sig16() | lshrs_flags_sig16r() | lshrs_flags_replay() | lshrs_flags_query() |
         (sig16_half_forced() >= 0 ? LSHRS_BUILD_TUNED | (1u << 25) : 0u);
}

int lshrs_stream_synchronize(void* stream) { return -(int)hipStreamSynchronize(static_cast<hipStream_t>(stream)); }

int lshrs_wait_done(const int32_t* done_host, int32_t epoch, int64_t spin_ns, void* stream) {
  if (done_host != nullptr && spin_ns > 0) {
    const volatile int32_t* word = done_host;
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t spins = 0;; ++spins) {
      if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == epoch) return 0;
#if !defined(__HIP_DEVICE_COMPILE__)
      __builtin_ia32_pause();
#endif
      if ((spins & 255) == 255 &&
          std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() > spin_ns)
        break;
    }
  }
  return -(int)hipStreamSynchronize(static_cast<hipStream_t>(stream));
}

// blas_model 0: ties are reported in tie_list (the caller resolves them on the host); > 0: stage 2 resolves them itself
// by replaying that summation order of the host BLAS (sig_fix8_kernel<true>), tie_list is not used.
// counters (replay only): the LSHRS_SIG_DEVICE_COUNTERS block; flag_y: the stage-1 value of every list entry (may be NULL).
// Which workgroup of sig16_kernel a launch takes: 128 rows, two per CU (sig16.hip), for vectors of up to kHalfMaxTiles k-tiles
// (measured, 1 M rows of 16 x 16: stage 1 +2 .. +5 % from 5 to 11 k-tiles, -1 .. -3 % from 12 on) and for batches whose
// 256-row workgroups would leave half of the CUs without one (up to 32 768 rows per column block: stage 1 59 -> 47 us at 768-d).
// LSHRS_SIG16_HALF_MAX_TILES (environment, read once; a measurement switch: tools/half_rows_ab.py) replaces both rules by a
// k-tile limit: 0 = never, 64 = always; lshrs_build_flags() says when it is set.
static bool sig16_half_rows(int ktiles, int64_t groups_of_256) {
  const int forced = sig16_half_forced();
  if (forced >= 0) return ktiles <= forced;
  return ktiles <= kHalfMaxTiles || groups_of_256 <= kHalfMaxGroups;
}

// What lshrs_sig_hash_batch_split_replay_f32 refuses before split_pass sees the call (and lshrs_split_stage2_args with it)
static int split_replay_refusal(int32_t num_bands, int32_t rows_per_band, int32_t dim, int32_t blas_model, const int32_t* counters) {
  const bool resident = sig_resident(num_bands, rows_per_band, dim).on;
  // dim % 4 elements of scalar tail: modelled from 9 elements up, model 1 / 2 = how the build compiles them (sig_fixany_kernel);
  // whole groups of four: both builds sum alike, model 1
  const bool tail_ok = dim % 4 != 0 && dim >= 9 && rows_per_band >= 2 && (blas_model == 1 || blas_model == 2);
  // bands of ONE row: the host calls sdot - modelled for both builds at every length (stage 2: sig_fixany_kernel)
  const bool one_row_ok = rows_per_band == 1 && (blas_model == 1 || blas_model == 2);
  if (!tail_ok && !one_row_ok && (blas_model != 1 || dim % 4 != 0)) return LSHRS_E_BADARG;
  const int body = dim & ~3;
  if ((dim < 32 && !resident) || (body % 8 != 0 && body > 4096) || counters == nullptr) return LSHRS_E_BADARG;
  return 0;
}

// What a split pass of this shape is: its geometry, whether stage 1 is the resident-image kernel, whether the pass takes the
// input itself (`aligned`) - and what it refuses.  split_pass and lshrs_split_stage2_args (stage 2 alone, for the tests' entry).
struct SplitPlan { SigGeom g; int row_bytes; bool narrow; SigResident rs; bool aligned; };
static int split_plan(const float* X, int64_t n, int64_t ldx, const void* workspace, int32_t num_bands, int32_t rows_per_band, int32_t dim,
                      const uint8_t* keys, const int64_t* tie_list, int32_t tie_cap, const int32_t* tie_count, const int64_t* flag_list,
                      int32_t flag_cap, const int32_t* flag_count, int blas_model, SplitPlan* p) {
  if (X == nullptr || workspace == nullptr || keys == nullptr || n < 0 || ldx < dim || flag_list == nullptr ||
      flag_count == nullptr || flag_cap <= 0 || !sig_shape_ok(num_bands, rows_per_band, dim))
    return LSHRS_E_BADARG;
  if (tie_list != nullptr && (tie_count == nullptr || tie_cap < 0)) return LSHRS_E_BADARG;
  const SigGeom g = sig_geom(num_bands, rows_per_band, dim);
  // (the second stage patches key bits with 32-bit atomics on the ALIGNED word around the byte: a word that straddles two
  //  rows, or the end of the buffer, shares its page with a byte that is ours, and the bits that are not ours go back as
  //  they came - key rows of any width, keys at any address)
  const bool narrow = sig_has_narrow_split(g);
  // short vectors of narrow hashers: the resident-image kernel (whole rows in registers: any dim % 4 == 0 with the replay)
  SigResident rs = sig_resident(num_bands, rows_per_band, dim);
  if (rs.on && dim % kKTile != 0 && blas_model == 0) rs.on = false;   // (only the replaying stage 2 masks a row's end)
  if (!sig_has_split(g) && !narrow && !rs.on) return LSHRS_E_TOOLARGE;
  const int64_t wgs = ((n + 127) / 128 + 7) / 8 * 8 * g.cb;          // (the most any launch below makes)
  if (n >= ((int64_t)1 << 42) || wgs > 0x7fffffffLL || g.cb > 65535) return LSHRS_E_TOOLARGE;
  // (a partial last k-tile - dim % 32 != 0 - only with the replay: its stage 2 is the one that reads the chunks past a row's end as zero)
  // With the replaying stage 2 rows of any length (from 9 elements) at any 4-byte address: both stage-1 kernels fetch the row's
  // last dim % 4 elements with its last four and shift them into place; stage 2 adds the library's scalar tail behind its tiles
  // (sig_fix8_kernel<., GENERAL>); the LDS-DMA takes 4-byte aligned addresses.  (Without the replay - blas_model 0 - as
  // before: 16-byte chunks of 16-byte aligned rows.)
  const bool aligned = ldx < (1 << 20) &&
                       (blas_model != 0 ? (dim % 4 == 0 || dim >= 9) && (dim >= 32 || rs.on)
                                        : dim % 32 == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0);
  *p = SplitPlan{g, num_bands * g.bb, narrow, rs, aligned};
  return 0;
}

// BUCKETS (lshrs_sig_sort mode 1): sig16_kernel appends flagged and sampled projections by key column (sig_replay.hip takes
// them from there): long rows, at most 1024 padded key columns, the replaying stage 2, the caller's scratch given
static bool split_buckets(const SplitPlan& p, int blas_model, int rows_per_band, const lshrs_sig_sort* sort) {
  const int padcols_all = p.row_bytes * 8;
  return !p.rs.on && blas_model != 0 && rows_per_band != 1 && sort != nullptr && sort->mode == 1 && sort->thr != nullptr &&
         padcols_all <= kSortMaxCols && p.g.ktiles > kFixSlabShort && sort->cap / padcols_all >= 64;
}

// What stage 2 of a split pass is handed.  sort: the bucket scratch where stage 1 filled it (split_buckets), else NULL.
static FixArgs split_stage2_args(const float* X, int64_t ldx, int dim, const float* base, const SplitPlan& p, int rows_per_band, uint8_t* keys,
                                 int64_t* tie_list, int32_t tie_cap, int32_t* tie_count, float tau, const int64_t* flag_list, float* flag_y,
                                 int32_t flag_cap, const int32_t* flag_count, int blas_model, int32_t* counters, const lshrs_sig_sort* sort,
                                 const int64_t* audit_list, const float* audit_vals, int audit_n) {
  const SigGeom& g = p.g;
  FixArgs f = fix_args_base(X, ldx, dim, base, g, rows_per_band, keys, p.row_bytes, flag_list, flag_count, flag_cap, tau, blas_model);
  if (p.narrow && !p.rs.on) {      // (the narrow block's own copy of the norms: the same values for every valid column)
    f.norms = base + sig_narrow_offset_floats(g) + sig_narrow_image_floats(g);
    if (tau > 0.f) f.tie_coef = f.norms;
  }
  f.tie_list = tie_list;
  f.tie_cap = tie_cap;
  f.tie_count = tie_count;
  if (sort != nullptr) {
    f.sorted_list = sort->list;
    f.sorted_y = sort->y;
    f.flag_thr = sort->thr;
    f.col_count = sort->hist + (size_t)(sort->parity & 1) * kSortMaxCols;
    f.col_cap = sort->cap / (p.row_bytes * 8);
  }
  if (blas_model != 0) {
    f.tail_model = blas_model;
    f.tie_list = nullptr;
    f.flag_y = flag_y;
    f.partials = counters + LSHRS_SIG_COUNTERS;
    f.count_ties = 1;
    f.audit_list = audit_n > 0 ? audit_list : nullptr;
    f.audit_vals = audit_vals;
    f.audit_n = audit_n;
  }
  return f;
}

static int split_pass(const float* X, int64_t n, int64_t ldx, const void* workspace, int32_t num_bands,
                      int32_t rows_per_band, int32_t dim, uint8_t* keys, int64_t* tie_list, int32_t tie_cap,
                      int32_t* tie_count, float tau, uint8_t* row_flags, int64_t* flag_list, float* flag_y,
                      int32_t flag_cap, int32_t* flag_count, float tau1, int blas_model, int32_t* counters,
                      int32_t* host_counts, const lshrs_sig_audit* audit, const lshrs_sig_opts* opts, void* stream) {
  if (n == 0) return 0;
  SplitPlan plan;
  const int rc0 = split_plan(X, n, ldx, workspace, num_bands, rows_per_band, dim, keys, tie_list, tie_cap, tie_count, flag_list, flag_cap,
                             flag_count, blas_model, &plan);
  if (rc0 != 0) return rc0;
  const SigGeom g = plan.g;
  const int row_bytes = plan.row_bytes;
  const bool narrow = plan.narrow, aligned = plan.aligned;
  const SigResident rs = plan.rs;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Opts o = read_opts(opts);
  const float* base = static_cast<const float*>(workspace);
  if (!aligned) {  // the split pass is built for 16-byte chunks of 16-byte aligned rows; anything else takes the f32 pass (same keys)
    if (blas_model != 0) return LSHRS_E_BADARG;   // (the f32 kernel reports ties, it does not resolve them)
    return lshrs_sig_hash_batch_f32(X, n, ldx, workspace, num_bands, rows_per_band, dim, keys, tie_list, tie_cap,
                                    tie_count, tau, row_flags, opts, stream);
  }
  // stage 1: bf16 x 3 projections -> keys + list of the projections inside the stage-1 window (+ their values)
  SigArgs a{};
  a.X = X;
  a.n = n;
  a.ldx = ldx;
  a.dim = dim;
  a.ktiles = g.ktiles;
  // its tables, for exactly one of four layouts: the resident image (sig16r_kernel) or compact column blocks (sig_compact) - list
  // entries and keys leave through padcol / bytetab -, the narrow hasher's zero-padded 256-column block, the padded layout
  const SigCompact cp = sig_compact(g, num_bands, rows_per_band);
  if (rs.on || cp.on) {
    float* wbase = const_cast<float*>(base);
    const SigCompactWs t = rs.on ? sig_resident_ws(wbase, g, num_bands, rows_per_band, rs) : sig_compact_ws(wbase, g, cp);
    a.ncb = rs.on ? 1 : cp.ncb;
    a.image = t.image;
    a.norms = t.norms;
    a.norm_max = t.norm_max;
    a.wa = t.wa;
    a.wb = t.wb;
    a.wamax = t.wamax;
    a.wbmax = t.wbmax;
    a.compact = 1;
    a.padcol = t.padcol;
    a.bytetab = t.bytetab;
    a.bpb = rs.on ? num_bands : cp.bpb;
    a.band_bytes = g.bb;
    a.num_bands = num_bands;
  } else {
    const SigWindow w = sig_window(base, g);
    a.ncb = narrow ? 1 : g.cb;
    a.image = base + (narrow ? sig_narrow_offset_floats(g) : sig_t16_offset_floats(g));
    a.norms = narrow ? a.image + sig_narrow_image_floats(g) : base + sig_image_floats(g);
    a.norm_max = a.norms + (narrow ? 256 : sig_norm_floats(g));
    a.wa = w.wa;
    a.wb = w.wb;
    a.wamax = narrow ? w.wamax + kNarrowMaxSlot : w.wamax;
    a.wbmax = narrow ? w.wbmax + kNarrowMaxSlot : w.wbmax;
  }
  // the window: LSHRS_WINDOW_PROVEN - ||x_hi|| wa + ||x_mid|| wb (lshrs_sig_set_window) -, or tau1 units of ||x|| ||p|| (the caller's)
  a.tau = a.tau_b = 1.0f;
  if (tau1 > 0.f) {
    a.tau = tau1;
    a.tau_b = 0.f;
    a.wa = a.wb = a.norms;
    a.wamax = a.wbmax = a.norm_max;
  }
  a.keys = keys;
  a.row_bytes = row_bytes;
  const int key_align = rs.on ? 4 : 16;                 // (sig16r_kernel stores 32-bit words, sig16_kernel pairs of them)
  a.vec_store = (row_bytes % key_align == 0) && ((reinterpret_cast<uintptr_t>(keys) % key_align) == 0);
  a.row_base = 0;
  a.tie_list = flag_list;
  a.flag_y = flag_y;
  a.tie_cap = flag_cap;
  a.tie_count = flag_count;
  a.row_flags = row_flags;
  a.clock_probe = o.clock_probe;
  // sig16_kernel's workgroup: 256 rows, or 128 (two per CU) - sig16_half_rows
  const bool half = !rs.on && sig16_half_rows(g.ktiles, (n + 255) / 256 * a.ncb);
  const int wg_rows = half ? 128 : 256, wg_waves = half ? 4 : 8;
  const int64_t row_tiles = (n + wg_rows - 1) / wg_rows;
  // the audit sample (lshrs_sig_audit): one unit in `div` - a wave of sig16_kernel, a 32-row tile of sig16r_kernel
  int audit_n = 0;
  if (audit != nullptr && audit->struct_bytes >= sizeof(lshrs_sig_audit) && audit->list != nullptr && audit->vals != nullptr &&
      audit->slots > 0 && audit->target > 0 && blas_model != 0) {
    const int res_rows = 16 * res_rt(rs.nct, rs.kt);
    const int64_t units = rs.on ? (n + res_rows - 1) / res_rows : (row_tiles + 7) / 8 * 8 * a.ncb * wg_waves;
    int64_t div = units / audit->target;
    if (div < 1) div = 1;
    if ((units + div - 1) / div > audit->slots) div = (units + audit->slots - 1) / audit->slots;
    if (div <= 0x7fffffffLL) {
      a.audit_list = audit->list;
      a.audit_vals = audit->vals;
      a.audit_div = (int)div;
      a.audit_phase = (int)(audit->seed % (uint32_t)div);
      a.audit_seed = audit->seed;
      audit_n = (int)((units - 1 - a.audit_phase) / div + 1);           // units u < `units` with u % div == phase: every slot is written
    }
  }
  const int padcols_all = row_bytes * 8;
  const bool buckets = split_buckets(plan, blas_model, rows_per_band, o.sort);
  if (buckets) {
    a.tie_list = o.sort->list;
    a.flag_y = o.sort->y;
    a.flag_thr = o.sort->thr;
    a.col_count = o.sort->hist + (size_t)(o.sort->parity & 1) * kSortMaxCols;
    a.col_cap = o.sort->cap / padcols_all;
  }
  if (rs.on) {
    const int res_rows = 16 * res_rt(rs.nct, rs.kt);
    const int64_t tiles = (n + res_rows - 1) / res_rows;
    const int rwaves = res_waves(rs.nct, rs.kt);
#ifndef LSHRS_RES_GRID
#define LSHRS_RES_GRID 256        // workgroups of a full launch: one per CU (A/B builds: more, shorter ones - the hardware hands them to the CUs that finish first)
#endif
    const unsigned grid = (unsigned)(tiles < (int64_t)LSHRS_RES_GRID * rwaves ? (tiles + rwaves - 1) / rwaves : LSHRS_RES_GRID);
    const int rc = lshrs_launch_sig16r(a, rs.nct, rs.kt, grid, 64u * (unsigned)rwaves, s, o.ev[0], o.ev[1]);
    if (rc != 0) return rc;
  } else {
    const int rc = lshrs_launch_sig16(a, (unsigned)((row_tiles + 7) / 8 * 8 * a.ncb), cp.on, dim % kKTile != 0, half, s, o.ev[0], o.ev[1]);
    if (rc != 0) return rc;
  }
  // stage 2: the flagged projections, one by one
  const FixArgs f = split_stage2_args(X, ldx, dim, base, plan, rows_per_band, keys, tie_list, tie_cap, tie_count, tau, flag_list, flag_y,
                                      flag_cap, flag_count, blas_model, counters, buckets ? o.sort : nullptr, a.audit_list, a.audit_vals, audit_n);
  const int rc2 = lshrs_replay_stage2(f, counters, host_counts, o, s);
  if (rc2 != 0) return rc2;
  return -(int)hipGetLastError();
}

int lshrs_sig_hash_batch_split_f32(const float* X, int64_t n, int64_t ldx, const void* workspace, int32_t num_bands,
                                   int32_t rows_per_band, int32_t dim, uint8_t* keys, int64_t* tie_list,
                                   int32_t tie_cap, int32_t* tie_count, float tau, uint8_t* row_flags,
                                   int64_t* flag_list, int32_t flag_cap, int32_t* flag_count, float tau1,
                                   const lshrs_sig_opts* opts, void* stream) {
  return split_pass(X, n, ldx, workspace, num_bands, rows_per_band, dim, keys, tie_list, tie_cap, tie_count, tau,
                    row_flags, flag_list, nullptr, flag_cap, flag_count, tau1, 0, nullptr, nullptr, nullptr, opts, stream);
}

int lshrs_sig_hash_batch_split_replay_f32(const float* X, int64_t n, int64_t ldx, const void* workspace,
                                          int32_t num_bands, int32_t rows_per_band, int32_t dim, uint8_t* keys,
                                          int32_t* counters, float tau, uint8_t* row_flags, int64_t* flag_list,
                                          float* flag_y, int32_t flag_cap, float tau1, int32_t blas_model,
                                          int32_t* host_counts, const lshrs_sig_audit* audit, const lshrs_sig_opts* opts,
                                          void* stream) {
  const int rc = split_replay_refusal(num_bands, rows_per_band, dim, blas_model, counters);
  if (rc != 0) return rc;
  return split_pass(X, n, ldx, workspace, num_bands, rows_per_band, dim, keys, nullptr, 0, counters + 0, tau, row_flags,
                    flag_list, flag_y, flag_cap, counters + 1, tau1, blas_model, counters, host_counts, audit, opts, stream);
}

}  // extern "C"

// Stage 2 of a split replay pass WITHOUT its stage 1, for lshrs_sig_replay_values_f32 (sig_replay.hip): the refusals of
// lshrs_sig_hash_batch_split_replay_f32 and of split_pass, and the FixArgs split_pass would hand to lshrs_replay_stage2 for a list
// the caller filled (counters[1]: its length) - or, want_buckets, for the column segments of o.sort, which must then be what
// split_pass itself would let stage 1 fill (split_buckets), else LSHRS_E_BADARG.  No audit sample.
int lshrs_split_stage2_args(const float* X, int64_t n, int64_t ldx, const void* workspace, int32_t num_bands, int32_t rows_per_band,
                            int32_t dim, uint8_t* keys, int32_t* counters, float tau, int64_t* flag_list, float* flag_y, int32_t flag_cap,
                            int32_t blas_model, const Opts& o, bool want_buckets, FixArgs* out) {
  const int rc = split_replay_refusal(num_bands, rows_per_band, dim, blas_model, counters);
  if (rc != 0) return rc;
  SplitPlan plan;
  const int rc0 = split_plan(X, n, ldx, workspace, num_bands, rows_per_band, dim, keys, nullptr, 0, counters + 0, flag_list, flag_cap,
                             counters + 1, blas_model, &plan);
  if (rc0 != 0) return rc0;
  if (!plan.aligned) return LSHRS_E_BADARG;
  const bool buckets = split_buckets(plan, blas_model, rows_per_band, o.sort);
  if (buckets != want_buckets) return LSHRS_E_BADARG;
  *out = split_stage2_args(X, ldx, dim, static_cast<const float*>(workspace), plan, rows_per_band, keys, nullptr, 0, counters + 0, tau, flag_list,
                           flag_y, flag_cap, counters + 1, blas_model, counters, buckets ? o.sort : nullptr, nullptr, nullptr, 0);
  return 0;
}
