// sig16.hip - part of liblshrs_hip.so, the gfx950 (MI355X / CDNA4) implementation of the lshrs hot path.
// K1: stage 1 of the split-precision signature pass - bf16 x 3 on v_mfma_f32_16x16x32_bf16, proven window, audit sample.
// One translation unit per kernel family (round 5): what is shared lives in lshrs_common.h, measurement switches (-DLSHRS_AB_*,
// tools/ab_build.py) are local to the unit whose kernel they alter and reported through lshrs_build_flags().
// ABI and reference citations: include/lshrs_hip.h.  Design notes: DESIGN.md.
#include "lshrs_common.h"

using namespace lshrs;

namespace {
// Grid: one dimension, blockIdx.x -> (row tile, column block) with the column blocks of one row tile eight workgroup
// ids apart: workgroups are dealt round-robin over the 8 XCDs, so the `cb` passes over the same 256 rows run on the
// SAME XCD at about the same time and the second one reads x from that XCD's L2 instead of HBM (config 5: 512 key
// columns = two column blocks).
#ifndef LSHRS_X_AUX
#define LSHRS_X_AUX 0              // cache policy of stage 1's x loads (A/B builds: 2 = nt)
#endif
// flagged projections a workgroup stages in LDS before its ONE global append: 8192 for the 256-row workgroup, 4096 for the 128-row one
// COMPACT: the column blocks hold the bands' key columns side by side (sig_compact) - list entries and keys leave through
// the tables; a template parameter so that the padded layout's kernel is instruction for instruction what it was.
// PARTIAL: vectors that are not whole 32-element k-tiles (300-d, 100-d; round 5: any length, 301-d, 767-d) - in the last k-tile
// the 16-byte chunks that reach past a row's end are fetched from the row's last four elements instead (never a byte past the
// row): the chunk that holds the row's last dim % 4 elements is shifted into place when it is read back, the ones behind it
// read as zero.  Rows may start at any 4-byte address (the LDS-DMA takes it: tools/probes/lds_dma_align_probe.hip).
// W: waves of a workgroup = 32 W rows.  W = 8: one workgroup per CU (the ring is 144 KiB).  W = 4 (round 6, vectors of up to
// ~512 elements): TWO workgroups of 128 rows per CU, each with its own fragment ring and a two-deep x ring (80 KiB: the x
// tile a k-tile's second stage reads into registers is free again two stages before the tile after next lands in its place) -
// independent barriers, so one workgroup's prologue, epilogue and dispatch run under the other one's k-tiles, which at ten
// to sixteen k-tiles is 20-28 % of a 256-row workgroup's time.  Twice the fragment traffic from L2, the same x traffic, the
// same instruction schedule per wave, the same accumulation.
template <bool COMPACT, bool PARTIAL = false, int W = 8>
__global__ __launch_bounds__(64 * W, 8 / W) void sig16_kernel(const SigArgs args) {
  constexpr int RT = 2;
  constexpr int kRows = 32 * W;                   // rows of a workgroup
  constexpr int kXDepth = W == 8 ? 3 : 2;         // x tiles in the ring
  constexpr int kS1ListCap = W == 8 ? 8192 : 4096;
  constexpr int kWaveRows = 16 * RT;
  constexpr int kPP = 16 / W;                     // fragment pieces a wave stages per stage
  constexpr int kXPS = RT;                        // x pieces a wave stages per stage (2 RT per k-tile)
  constexpr int kE = 6 * RT;                      // MFMAs per eighth: 2 column tiles x 3 terms x RT row tiles
  constexpr int kSlices = 12 * RT;                // split slices per k-tile: 4 RT pairs x 3 steps
  constexpr int kPHalf = 16 * kFragFloats;        // floats of one fragment stage (16 blocks of 1 KiB)
  constexpr int kXTile = kRows * kKTile;          // floats of one x tile of the workgroup
  constexpr int kXWave = kWaveRows * kKTile;
  constexpr int kRingFloats = 3 * kPHalf + kXDepth * kXTile;
  constexpr int kIssues = (kPP + kXPS) / 2;       // DMA instructions a wave issues under each of a stage's last two eighths
  constexpr int kIssueStep = kE / kIssues;
  static_assert((kPP + kXPS) % 2 == 0 && kE % kIssues == 0, "DMA issue slots");
  static_assert(3 * kS1ListCap <= kRingFloats, "the epilogue's list stage reuses the ring");
  // the epilogue's tables: behind the list stage in the ring; the list counters behind the ring where one workgroup owns the
  // CU, inside it (behind the sign words) where two share it: 80 KiB each, to the byte
  constexpr int kTabOff = 3 * kS1ListCap;
  constexpr int kCntOff = W == 8 ? kRingFloats : kTabOff + 768 + kRows * 8;
  static_assert(kCntOff + 4 <= (W == 8 ? kRingFloats + 4 : kRingFloats), "list counters");
  __shared__ __attribute__((aligned(16))) float lds[W == 8 ? kRingFloats + 4 : kRingFloats];
  struct Bf16Pairs { bf16x2 p[4]; };

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g = lane >> 4;
  // blockIdx.x = ((group * ncb + cb) * 8 + xcd slot): row tile = group * 8 + slot
  const int ncb = args.ncb;
  const int bid = blockIdx.x;
  const int cb = (bid >> 3) % ncb;
  const int row_tile = ((bid >> 3) / ncb) * 8 + (bid & 7);
  // the audit sample of this wave (SigArgs::audit_list): slot au_slot (-1: not sampled), accumulator word au_rw = 8 rt + w,
  // lane au_lane, slot au_q of that word's eight values
  int au_slot = -1, au_rw = -1, au_lane = 0, au_q = 0;
  if (args.audit_list != nullptr) {
    const unsigned u = (unsigned)bid * (unsigned)W + (unsigned)wave;
    if ((int)(u % (unsigned)args.audit_div) == args.audit_phase) {
      const unsigned h = audit_hash(u, args.audit_seed);
      au_slot = (int)(u / (unsigned)args.audit_div);
      au_rw = (int)(h & 15u);
      au_q = (int)((h >> 4) & 7u);
      au_lane = (int)((h >> 7) & 63u);
    }
  }
  if ((int64_t)row_tile * kRows >= args.n) {           // (whole workgroup: the grid is padded to a multiple of 8 row tiles)
    if (au_slot >= 0 && lane == 0) args.audit_list[au_slot] = -1;
    return;
  }
  const int ktiles = args.ktiles;
  const int stages = 2 * ktiles, lasts = stages - 1;
  const char* img = reinterpret_cast<const char*>(args.image) + (size_t)cb * ktiles * 32768;
  const int64_t blk_row0 = (int64_t)row_tile * kRows;
  const int64_t row0 = blk_row0 + wave * kWaveRows;
  const char* xblk = reinterpret_cast<const char*>(args.X + blk_row0 * args.ldx);

  // DMA offsets.  x is staged in FULL 128-byte lines: piece j (0..3) of a wave = rows 8j..8j+7 of its 32; lane
  // l = (r = l>>3, q = l&7) fetches 16-byte chunk q ^ r ^ (j&1) of row 8j + r, so an 8-lane group covers one whole
  // line (in permuted order) and the read-back (each lane: its row's two chunks of the k-tile quarter it feeds) is
  // conflict-free for ds_read_b128's 16-lane groups.
  // (fragments: one lane offset in a register, piece d is W d KiB behind it on both sides - the scalar offset of the piece carries it)
  unsigned xfo[2 * RT], xrd[2];
  const unsigned poff = (unsigned)((wave * 64 + lane) * 16);
  {
    const int r8 = lane >> 3, q8 = lane & 7;
#pragma unroll
    for (int j = 0; j < 2 * RT; ++j) {
      const int64_t r = row0 + 8 * j + r8;
      const int64_t rl = (r < args.n ? r : args.n - 1) - blk_row0;   // clamp: loads stay in bounds, stores are masked
      xfo[j] = (unsigned)((rl * args.ldx + 4 * (q8 ^ r8 ^ (j & 1))) * 4);
    }
    {
      const int j = r16 >> 3, r = r16 & 7;       // this lane's row of row tile 0: chunks 2g, 2g+1; row tile rt is 2048 rt bytes behind
#pragma unroll
      for (int c = 0; c < 2; ++c) xrd[c] = (unsigned)(wave * (kXWave * 4) + j * 1024 + (r * 8 + ((2 * g + c) ^ r ^ (j & 1))) * 16);
    }
  }

  f32x4 acc[RT][16];
  float ss[RT], sm[RT], amax[RT];      // ||x_hi||^2, ||x_mid||^2 (both from the bf16 pieces the MFMAs consume), max |x|
  auto zero_tile_state = [&]() {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < 16; ++ct) {
        acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        // pin the zeroing HERE: the MFMAs below are inline asm, so hipcc pads no hazard for them - a v_accvgpr_write
        // rematerialised right in front of the first accumulation would be read too early
        asm volatile("" : "+a"(acc[rt][ct]));
      }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { ss[rt] = 0.f; sm[rt] = 0.f; amax[rt] = 0.f; }
  };
  unsigned long long t_shader = 0, t_real = 0;
  if (args.clock_probe != nullptr) {
    t_shader = __builtin_amdgcn_s_memtime();
    t_real = __builtin_amdgcn_s_memrealtime();
  }

  const int last_valid_chunks = PARTIAL ? (args.dim - (ktiles - 1) * kKTile) / 4 : 8;   // WHOLE 16-byte chunks of a row in the last k-tile
  const int rem = PARTIAL ? (args.dim & 3) : 0;                                          // elements of the chunk behind them
  const int tail_off = PARTIAL ? (args.dim - 4 - (ktiles - 1) * kKTile) * 4 : 0;         // the row's last four elements, from the last k-tile's start (bytes)
  // The LDS-DMA goes through two buffer descriptors, built once from wave-uniform values: a piece is then
  // `buffer_load_dwordx4 v_lane_offset, s[descriptor], s_uniform_offset offen lds` - the lane offsets stay the 32-bit values
  // they are, the stage / k-tile advance is a scalar, and no vector instruction forms an address per piece (the global form
  // costs one 64-bit vector add per piece and a 64-bit register pair per lane offset).  The fragment image of this column
  // block; x: exactly what this workgroup may touch (the row clamp above is the mechanism, the range check returns zeros
  // and is only the net under it; < 2^31: 256 rows of < 2^20 elements).  Rows at any 4-byte address go through it like
  // aligned ones.  PARTIAL keeps the global form for its x pieces (the chunk redirection below is as it was); its
  // fragments take the descriptor.
  const int rows_here = (int)(args.n - blk_row0 < (int64_t)kRows ? args.n - blk_row0 : (int64_t)kRows);
  const __amdgpu_buffer_rsrc_t rs_img = uniform_buffer(img, (unsigned)ktiles * 32768u);
  const __amdgpu_buffer_rsrc_t rs_x = uniform_buffer(xblk, (unsigned)(((int64_t)(rows_here - 1) * args.ldx + args.dim) * 4));
  LDS_AS char* const lds_b = (LDS_AS char*)lds;
  // Ring positions are counters that rotate in scalar registers (no `% 3` of the stage number): the LDS byte offsets of the
  // fragment slots of stages s, s + 1, s + 2 and of the x slots of k-tiles t, t + 1, t + 2 (two-deep x ring: t + 2 is t's)
  unsigned fr0 = 0u, fr1 = (unsigned)kPHalf * 4u, fr2 = 2u * (unsigned)kPHalf * 4u;
  unsigned xq0 = 3u * kPHalf * 4u, xq1 = xq0 + (unsigned)kXTile * 4u, xq2 = kXDepth == 3 ? xq1 + (unsigned)kXTile * 4u : xq0;
  const unsigned wave_f = (unsigned)wave * (kFragFloats * 4u), wave_x = (unsigned)wave * (kXWave * 4u);
  // fragment piece d of stage c (clamped by the caller) into the slot at LDS byte `slot`
  auto issue_frag = [&](int d, int c, unsigned slot) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_img, (LDS_AS void*)(lds_b + (slot + wave_f + (unsigned)(W * d * 1024))), 16, (int)poff,
                                             c * 16384 + W * d * 1024, 0, 0);
  };
  // x piece j (0 .. 2 RT - 1) of k-tile t (clamped by the caller) into the x slot at LDS byte `slot`
  auto issue_x = [&](int j, int t, unsigned slot) {
    LDS_AS void* dst = (LDS_AS void*)(lds_b + (slot + wave_x + (unsigned)(j * 1024)));
    if constexpr (!PARTIAL) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, dst, 16, (int)xfo[j], t * (kKTile * 4), 0, LSHRS_X_AUX);
    } else {
      // branch-free (a branch here changes where hipcc joins the accumulator tiles around the inline-asm MFMAs): in the last
      // k-tile a chunk that is not wholly inside the row is fetched from the row's last four elements instead; this lane's
      // chunk of the line, as in xfo
      const unsigned off = xfo[j];
      const int lim = t == ktiles - 1 ? last_valid_chunks : 8;
      const int chunk = (int)((lane & 7) ^ (lane >> 3) ^ (j & 1));
      const int o2 = chunk >= lim ? (int)off - 16 * chunk + tail_off : (int)off;      // (off < 2^30: 256 rows of < 2^20 elements)
      __builtin_amdgcn_global_load_lds((const GLOBAL_AS void*)(xblk + (size_t)t * (kKTile * 4) + o2), dst, 16, 0, LSHRS_X_AUX);
    }
  };
  // what stage s issues: fragments of stage s + 2, x pieces kXPS (s & 1) .. of tile (s >> 1) + 2; piece d of the kPP + kXPS
  auto issue = [&](int s, int ch, int d) {
    if (d < kPP) {
      const int ns = s + 2;
      issue_frag(d, ns < lasts ? ns : lasts, fr2);
    } else {
      const int nt = (s >> 1) + 2;
      issue_x(kXPS * ch + d - kPP, nt < ktiles ? nt : ktiles - 1, xq2);
    }
  };
  f32x4 xr[RT][2];                           // raw f32 x of one k-tile: [row tile][chunk]
  auto read_x = [&](int t, unsigned slot) {   // k-tile t from the x slot at LDS byte `slot`: two vector adds, row tile 1 is an immediate
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      unsigned at = xrd[c] + slot;
      asm volatile("" : "+v"(at));            // (opaque: hipcc otherwise keeps an address register per read and ring position)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) xr[rt][c] = *reinterpret_cast<const LDS_AS f32x4*>(lds_b + (at + 2048u * rt));
    }
    if constexpr (PARTIAL) {                // chunks 2 g, 2 g + 1 of the last k-tile: past the row's end they read as zero (selects, no branch)
      const int lim = t >= ktiles - 1 ? last_valid_chunks : 8;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const bool part = rem != 0 && 2 * g + c == lim;      // the chunk with the row's last dim % 4 elements
          xr[rt][c] = tail_chunk(xr[rt][c], rem, part, 2 * g + c >= lim && !part);
        }
    }
  };
  float r0 = 0.f, r1 = 0.f;
  auto split_step = [&](int q, Bf16Pairs (&hi)[RT], Bf16Pairs (&mid)[RT]) {   // slice q (0..kSlices-1) of one k-tile's split
    const int pair = q / 3, step = q % 3, rt = pair >> 2, pr = pair & 3, c = pr >> 1, e = 2 * (pr & 1);
    const float v0 = xr[rt][c][e], v1 = xr[rt][c][e + 1];
    // ONE conversion per pair, as an asm statement (the instruction hipcc selects for the cast; left to it, in four pairs of
    // a k-tile it converts the two elements separately and packs them again)
    if (step == 0) {
      bf16x2 hp;
      asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(hp) : "v"(v0), "v"(v1));
      hi[rt].p[pr] = hp;
      r0 = v0 - (float)hp[0];
      r1 = v1 - (float)hp[1];
    } else if (step == 1) {
      bf16x2 mp;
      asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(mp) : "v"(r0), "v"(r1));
      mid[rt].p[pr] = mp;
    } else {
      ss[rt] = __builtin_amdgcn_fdot2_f32_bf16(hi[rt].p[pr], hi[rt].p[pr], ss[rt], false);
#ifndef LSHRS_AB_NO_XMID_NORM          // (A/B builds only, tools/ab_build.py: what ||x_mid||^2 costs stage 1; keys are wrong without it)
      sm[rt] = __builtin_amdgcn_fdot2_f32_bf16(mid[rt].p[pr], mid[rt].p[pr], sm[rt], false);
#endif
      asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(amax[rt]) : "v"(v0), "v"(v1));
    }
  };
  // Fragments travel in EIGHTHS of a stage: 2 column tiles x {hi, mid} = 4 ds_read_b128 = 16 VGPRs, two buffers.
  // (Quarters, as in sig_kernel, push this kernel over 256 VGPRs next to its 256 accumulator AGPRs: hipcc then
  // shuffles accumulators through v_accvgpr moves inside the loop.)
  // `base`: this lane's address in the stage's slot (ONE vector add per stage), the eighths are immediate offsets
  auto read_eighth = [&](unsigned base, int e, f32x4 (&f)[2][2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f[j][0] = *reinterpret_cast<const LDS_AS f32x4*>(lds_b + (base + (unsigned)(((2 * e + j) * 2 + 0) * 1024)));
      f[j][1] = *reinterpret_cast<const LDS_AS f32x4*>(lds_b + (base + (unsigned)(((2 * e + j) * 2 + 1) * 1024)));
    }
  };
  const unsigned lane16 = (unsigned)lane * 16u;
  // MFMA k (0..11) of an eighth: term k / 4 of xh*ph + xh*pm + xm*ph, column tile ct0 + (k / 2) % 2, row tile k % 2: the
  // four accumulator tiles of the eighth take turns, so two MFMAs on the same tile are four instructions (64 cycles)
  // apart.  (Two apart - tile order (j, term, rt) - the result of a 4-pass MFMA is not back in time and hipcc pads every
  // other MFMA with an s_nop: 33 per k-tile and wave.)  Every tile still sees its terms in the order 0, 1, 2.
  auto mfma_one = [&](int ct0, int k, const f32x4 (&f)[2][2], const Bf16Pairs (&hi)[RT], const Bf16Pairs (&mid)[RT], const bool drain = false) {
    const int term = k / (2 * RT), j = (k / RT) % 2, rt = k % RT;
    const bf16x8 a = __builtin_bit_cast(bf16x8, term == 2 ? mid[rt] : hi[rt]);
    const bf16x8 b = __builtin_bit_cast(bf16x8, f[j][term == 1 ? 1 : 0]);
    // D = P X^T (the fragments are the instruction's first operand, x its second - both operands have the same register layout):
    // lane (r16, g) ends with columns 16 ct + 4 g + e of ITS row r16, as in sig16r_kernel - the epilogue needs one row's window per
    // lane and one v_alignbit per sign.  The products and their order of accumulation are what they were.
    // Inline asm pins the accumulator to AGPRs and to in-place accumulation: left to the builtin, hipcc renames
    // accumulator tiles between MFMAs (vDst != SrcC) and parks some in VGPRs, i.e. hundreds of v_accvgpr moves and
    // s_nops per loop body.  Dependent MFMAs are four instructions (64 cycles) apart, beyond the 4-pass hazard window.
#ifdef LSHRS_T16_BUILTIN
    acc[rt][ct0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, acc[rt][ct0 + j], 0, 0, 0);
#else
    // drain (behind the last barrier, where the two ends of the tile loop join): the wait states are PART of the statement -
    // hipcc may move accumulator tiles between registers at the join, and as two statements it put those moves between
    // the MFMA and its wait states (round 6, odd k-tile counts: the live audit fired; tools/check_mfma_hazards.py looks for it)
    if (drain) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %2, %1, %0\n\ts_nop 7\n\ts_nop 4" : "+a"(acc[rt][ct0 + j]) : "v"(a), "v"(b));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %2, %1, %0" : "+a"(acc[rt][ct0 + j]) : "v"(a), "v"(b));
#endif
  };

  f32x4 fa[2][2], fb[2][2];
  Bf16Pairs hs0[RT], ms0[RT], hs1[RT], ms1[RT];   // bf16 x of the k-tiles, ping-pong by tile parity

  // One k-tile = two stages (column halves ch), one stage = four eighths E0..E3 of 24 MFMAs.  Every eighth's MFMAs
  // run while the next eighth's fragments are read; the last eighth of a stage is consumed after the barrier:
  //   barrier(s) | read E0(s) | MFMA E3(s-1) | read E1(s) [+ raw x of the next tile, ch = 1] | MFMA E0(s) |
  //              | read E2(s) | MFMA E1(s) + DMA | read E3(s) | MFMA E2(s) + DMA | barrier(s+1)
  // The next tile's x is read in the second stage of a tile and split (48 slices) under that stage's last two
  // eighths and the first eighth after the tile boundary: it must be complete before E0 of the new tile.
  auto stage = [&](int s, const int ch, const bool first, const Bf16Pairs (&hc)[RT], const Bf16Pairs (&mc)[RT],
                   const Bf16Pairs (&hp)[RT], const Bf16Pairs (&mp)[RT], Bf16Pairs (&hn)[RT], Bf16Pairs (&mn)[RT]) {
    // hc/mc: this stage's tile; hp/mp: the tile E3(s-1) belongs to; hn/mn: where the split in flight writes
    unsigned st = lane16 + fr0;
    asm volatile("" : "+v"(st));
    read_eighth(st, 0, fa);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < kE; ++k) {
      if (!first) mfma_one(8 * (1 - ch) + 6, k, fb, hp, mp);        // E3 of the previous stage (the other column half)
      if (ch == 0) {                                                  // the last third of this tile's split (2 slices per 3 MFMAs)
        if (k % 3 != 2) split_step(2 * kSlices / 3 + (k / 3) * 2 + k % 3, hn, mn);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    wait_vmcnt<kXPS>();                                               // own fragments of stage s+1 and every older x piece
    read_eighth(st, 1, fb);
    if (ch == 1) read_x((s >> 1) + 1, xq1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < kE; ++k) {
      mfma_one(8 * ch + 0, k, fa, hc, mc);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    read_eighth(st, 2, fa);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < kE; ++k) {
      mfma_one(8 * ch + 2, k, fb, hc, mc);
      if (ch == 1 && k % 3 != 2) split_step((k / 3) * 2 + k % 3, hn, mn);          // first third of the next tile's split
      if (k % kIssueStep == 0) issue(s, ch, k / kIssueStep);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    read_eighth(st, 3, fb);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < kE; ++k) {
      mfma_one(8 * ch + 4, k, fa, hc, mc);
      if (ch == 1 && k % 3 != 2) split_step(kSlices / 3 + (k / 3) * 2 + k % 3, hn, mn);   // second third
      if (k % kIssueStep == 0) issue(s, ch, kIssues + k / kIssueStep);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    {                                       // the rings turn: a stage on, and behind a tile's second stage a k-tile on
      const unsigned f = fr0;
      fr0 = fr1; fr1 = fr2; fr2 = f;
      if (ch == 1) {
        const unsigned x = xq0;
        xq0 = xq1;
        if (kXDepth == 3) { xq1 = xq2; xq2 = x; } else { xq1 = x; xq2 = xq0; }
      }
    }
  };
  // tile t with its sets (hc, mc); the previous tile's (hp, mp) double as the target of the next tile's split
  auto tile = [&](int t, const bool first, Bf16Pairs (&hc)[RT], Bf16Pairs (&mc)[RT], Bf16Pairs (&hp)[RT], Bf16Pairs (&mp)[RT]) {
    stage(2 * t, 0, first, hc, mc, hp, mp, hc, mc);       // ch 0: E3(s-1) is the previous tile's; the split in flight is this tile's
    stage(2 * t + 1, 1, false, hc, mc, hc, mc, hp, mp);   // ch 1: E3(s-1) is this tile's; the next tile's split starts (into the other set)
  };

  auto issue_prologue = [&]() {     // the first two stages' fragments and the first two x tiles of the row tile entered
    const int t1 = ktiles > 1 ? 1 : 0;
#pragma unroll
    for (int d = 0; d < kPP; ++d) issue_frag(d, 0, fr0);                                    // fragments of stage 0
#pragma unroll
    for (int d = 0; d < kXPS; ++d) { issue_x(d, 0, xq0); issue_x(kXPS + d, 0, xq0); }       // x tile 0
#pragma unroll
    for (int d = 0; d < kPP; ++d) issue_frag(d, 1, fr1);                                    // fragments of stage 1
#pragma unroll
    for (int d = 0; d < kXPS; ++d) { issue_x(d, t1, xq1); issue_x(kXPS + d, t1, xq1); }     // x tile 1
  };
  // Static priority for the second-dispatched half of the workgroup: of the two waves of a SIMD the younger one loses the
  // VALU arbitration (priority, then age) on every stage; one s_setprio for that half, no flips (MI355X_MICROARCH.md, "Two
  // waves per SIMD", item 4).  Same box, interleaved, four pairs: +0.2 .. +0.9 % (profiles/r03_static_prio_ab.log).
#ifndef LSHRS_AB_NO_STATIC_PRIO
  if (W == 8 && wave >= 4) __builtin_amdgcn_s_setprio(1);
#endif
  issue_prologue();
  zero_tile_state();
  wait_vmcnt<kPP + 2 * kXPS>();
  __builtin_amdgcn_s_barrier();
  read_x(0, xq0);
#pragma unroll
  for (int q = 0; q < 2 * kSlices / 3; ++q) split_step(q, hs0, ms0);   // tile 0 only: the last third rides in stage 0 as for every tile
  tile(0, true, hs0, ms0, hs1, ms1);
  int t = 1;
  for (; t + 1 < ktiles; t += 2) {
    tile(t, false, hs1, ms1, hs0, ms0);
    tile(t + 1, false, hs0, ms0, hs1, ms1);
  }
  Bf16Pairs hd[RT], md[RT];                                              // the last tile's set: ONE drain behind the join
  if (t < ktiles) {                                                      // even number of k-tiles: one more, then drain with its set
    tile(t, false, hs1, ms1, hs0, ms0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { hd[rt] = hs1[rt]; md[rt] = ms1[rt]; }
  } else {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { hd[rt] = hs0[rt]; md[rt] = ms0[rt]; }
  }
#pragma unroll
  for (int k = 0; k < kE; ++k) mfma_one(14, k, fb, hd, md, true);
  // (the wait states after every MFMA of the drain: where the two branches join hipcc may copy accumulator tiles, and
  //  it does not know that the asm in front of such a copy is an MFMA whose result takes passes to arrive)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped prefetches past the last stage must land before exit
  __builtin_amdgcn_s_barrier();
  // Landing point of the accumulators.  hipcc does not know that the asm statements above are MFMAs whose results
  // take passes to arrive: without this it hoists the epilogue's v_accvgpr_reads to a few instructions behind the
  // last MFMA (observed: one register of one tile read before its final accumulation).  Volatile asms keep their
  // order, and every read below depends on the empty asm that follows the wait states.
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < 16; ++ct) asm volatile("" : "+a"(acc[rt][ct]));

  if (args.clock_probe != nullptr && tid == 0) {
    const unsigned long long slot = (unsigned long long)blockIdx.x;
    args.clock_probe[2 * slot] = __builtin_amdgcn_s_memtime() - t_shader;
    args.clock_probe[2 * slot + 1] = __builtin_amdgcn_s_memrealtime() - t_real;
  }

  // The ring is free (every wave is past the barrier above, every prefetch has landed): the epilogue stages the
  // workgroup's flagged projections in it - list entries and their stage-1 values - and appends them to the global
  // list with ONE atomic per workgroup.  (One atomic per flagged projection on the single global counter serialises:
  // at a 870-unit window - 300 k flagged projections per 1M rows - it tripled the kernel's time.)
  // Everything the epilogue derives from the lane index is loop-invariant: left alone, hipcc computes it in front of
  // the main loop and carries (or spills) it across.  These copies are opaque: the epilogue's addressing starts here.
  int r16e = r16, ge = g, lanee = lane;
  asm volatile("" : "+v"(r16e), "+v"(ge), "+v"(lanee));
  int64_t* l_list = reinterpret_cast<int64_t*>(lds);
  float* l_y = lds + 2 * kS1ListCap;
  int* l_count = reinterpret_cast<int*>(lds + kCntOff);   // [0] staged + overflowed entries, [1] global base
  if (tid == 0) l_count[0] = 0;

  // ---- the block's tables, staged once behind the list stage (which owns the first 3 x kS1ListCap floats of the ring) ----
  // The window coefficients: with the proven window the exact test below runs on a third of the 32-column words, and a global
  // load in front of each of its compares is latency two waves per SIMD cannot hide.  In IMAGE order (t16_colmap: position
  // 16 ct + m holds the block's column the map names), so a lane reads the coefficients of its four columns of a column tile as
  // one 16-byte word.
  float* coef_lds = lds + kTabOff;
  static_assert(kTabOff + 512 <= kRingFloats, "coefficients behind the list stage");
#pragma unroll
  for (int i = tid; i < 512; i += 64 * W) {
    const int src = cb * 256 + t16_colmap((i & 255) >> 4, i & 15);
    coef_lds[i] = i < 256 ? args.wa[src] : args.wb[src];
  }
  // compact column blocks (sig_compact): the padded id of every column of this block, in image order too, and room for the
  // block's sign words.  Padded blocks: which bits of the block's sign string are key columns (a band's padding columns and the
  // block's tail have no hyperplane - norm 0, y = +0 - and their key bits are 0)
  int* padcol_lds = reinterpret_cast<int*>(lds + kTabOff + 512);
  uint32_t* live_lds = reinterpret_cast<uint32_t*>(lds + kTabOff + 512);
  uint32_t* cw_lds = reinterpret_cast<uint32_t*>(lds + kTabOff + 768);
  static_assert(kTabOff + 768 + kRows * 8 <= kRingFloats, "compact tables behind the coefficients");
  if (tid < 256) {                                     // (whole waves: the first four)
    if (COMPACT) {
      padcol_lds[tid] = args.padcol[cb * 256 + t16_colmap(tid >> 4, tid & 15)];
    } else {
      const unsigned long long live = __builtin_amdgcn_ballot_w64(args.norms[cb * 256 + tid] > 0.f);
      if (lane == 0) *reinterpret_cast<u32x2*>(live_lds + 2 * wave) = u32x2{(uint32_t)live, (uint32_t)(live >> 32)};
    }
  }

  // ---- row statistics -> the two factors of the stage-1 window and the screen, per lane for ITS row (in registers) ------
  // (window_hi: a row outside the guarded range gets +inf - NOT(|y| > +inf) holds for every y: all of its projections are
  // re-evaluated.  A true zero row gives y = 0 in both passes.)
  const float amax_cb = args.wamax[cb], bmax_cb = args.wbmax[cb];
  float wnd[RT], wnb[RT], tsmax[RT];
  bool zrow[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const float s2 = row_lanes_sum(ss[rt]), m2 = row_lanes_sum(sm[rt]), am = row_lanes_max(amax[rt]);
    const int64_t myrow = row0 + 16 * rt + r16e;
    wnd[rt] = window_hi<false>(s2, am, args.tau);
    wnb[rt] = window_mid<false>(m2, args.tau_b);
    tsmax[rt] = row_screen(wnd[rt], wnb[rt], amax_cb, bmax_cb);
    zrow[rt] = am == 0.f;                  // every projection of the row is +0: all bits 0 (a NaN row is flagged wholesale)
    if (ge == 0 && cb == 0 && args.row_flags != nullptr && myrow < args.n) args.row_flags[myrow] = row_flag_byte(am, s2);
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();

  // ---- sign bits, window test, list.  A lane's 64 values of a row are 64 consecutive bits of the row's sign string (the
  // image is packed in that order): shift_sign_in per value, words 2 g and 2 g + 1 of the block's eight per row.
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t grow = row0 + 16 * rt + r16e;
    uint32_t word[2] = {0u, 0u};
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      float m = __builtin_inff();                     // min |y| over the 2 tiles x 4 registers of this word (NaN dropped:
                                                      // a NaN y only comes from a row whose window is non-finite)
#pragma unroll
      for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int reg = 0; reg < 4; reg += 2) {
          const float y0 = acc[rt][2 * w + half][reg], y1 = acc[rt][2 * w + half][reg + 1];
          word[w >> 2] = shift_sign_in(word[w >> 2], y0);
          word[w >> 2] = shift_sign_in(word[w >> 2], y1);
          asm("v_min3_f32 %0, |%1|, |%2|, %0" : "+v"(m) : "v"(y0), "v"(y1));
        }
      const bool aud = au_rw == 8 * rt + w;                   // (wave-uniform: this word holds the wave's audit sample)
      if (__builtin_amdgcn_ballot_w64(!(m > tsmax[rt])) != 0 || aud) {   // wave-uniform: the exact per-element test
        // With the proven window this runs on a fraction of the words: first the eight comparisons, branch-free, into a
        // mask; only the lane that holds a flagged projection (one, seldom two of the wave) enters the append.
        unsigned hits = 0u;
        float ys[8], thrs[8];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int ct = 2 * w + half;
          const f32x4 pa = *reinterpret_cast<const f32x4*>(coef_lds + 16 * ct + 4 * ge);
          const f32x4 pb = *reinterpret_cast<const f32x4*>(coef_lds + 256 + 16 * ct + 4 * ge);
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            float thr = wnd[rt] * pa[reg] + wnb[rt] * pb[reg];
            thr = thr > 0.f ? thr : -1.f;                               // zero row / zero-padded column: y is exactly 0
            ys[4 * half + reg] = acc[rt][ct][reg];
            thrs[4 * half + reg] = thr;
            hits |= (!(__builtin_fabsf(ys[4 * half + reg]) > thr) ? 1u : 0u) << (4 * half + reg);
          }
        }
        if (aud && lanee == au_lane) {
          // the sample: value au_q of this lane - left for stage 2 with the window it has just been compared with, unless
          // it is flagged anyway (then stage 2 decides it), sits in a padding column or past the last row
          float yq = ys[0], tq = thrs[0];
#pragma unroll
          for (int q = 1; q < 8; ++q) {
            yq = au_q == q ? ys[q] : yq;
            tq = au_q == q ? thrs[q] : tq;
          }
          const int ct = 2 * w + (au_q >> 2), mpos = 4 * ge + (au_q & 3);
          const int colid = COMPACT ? padcol_lds[16 * ct + mpos] : cb * 256 + t16_colmap(ct, mpos);
          const bool keep = ((hits >> au_q) & 1u) == 0u && grow < args.n && colid >= 0 && colid < args.row_bytes * 8 &&
                            tq < __builtin_inff();
          if (args.col_cap > 0) {           // buckets: the sample rides in its column's segment, marked
            if (keep) {
              const int slot = atomicAdd(args.col_count + colid, 1);
              if (slot < args.col_cap) {
                const size_t at = (size_t)colid * args.col_cap + slot;
                args.tie_list[at] = flag_entry(grow, colid) | kAuditBit;
                args.flag_y[at] = yq;
                args.flag_thr[at] = tq;
              }
            }
          } else {
            args.audit_list[au_slot] = keep ? flag_entry(grow, colid) : (int64_t)-1;
            args.audit_vals[2 * au_slot] = yq;
            args.audit_vals[2 * au_slot + 1] = tq;
          }
        }
        if (hits != 0u) {
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int reg = q & 3, ct = 2 * w + (q >> 2);
            const int colid = COMPACT ? padcol_lds[16 * ct + 4 * ge + reg] : cb * 256 + t16_colmap(ct, 4 * ge + reg);
            // (a NaN / Inf row also "flags" the zero-padded columns behind the last key column: the plain list carries
            //  them to stage 2, which skips them; a bucket launch has no segment for them)
            if (((hits >> q) & 1u) != 0u && grow < args.n && (!COMPACT || colid >= 0) &&
                (args.col_cap == 0 || colid < args.row_bytes * 8)) {
              const int64_t entry = flag_entry(grow, colid);
              const float yk = ykeep(wnd[rt], ys[q]);
              const int pos = atomicAdd(l_count, 1);                    // LDS atomic
              if (pos < kS1ListCap) {
                l_list[pos] = entry;
                l_y[pos] = yk;
              } else if (args.col_cap > 0) {                            // LDS stage full, buckets: straight to the column's segment
                atomicAdd(args.tie_count, 1);
                const int slot = atomicAdd(args.col_count + colid, 1);
                if (slot < args.col_cap) {
                  args.tie_list[(size_t)colid * args.col_cap + slot] = entry;
                  args.flag_y[(size_t)colid * args.col_cap + slot] = yk;
                }
              } else {                                                  // LDS stage full (rows flagged wholesale): straight out
                const int slot = atomicAdd(args.tie_count, 1);
                if (slot < args.tie_cap) {
                  args.tie_list[slot] = entry;
                  if (args.flag_y != nullptr) args.flag_y[slot] = yk;
                }
              }
            }
          }
        }
      }
    }
    // the lane's 64 bits of row 16 rt + r16: words 2 g, 2 g + 1 of the block's part of the row's sign string
    uint32_t w0 = zrow[rt] ? 0u : ~word[0], w1 = zrow[rt] ? 0u : ~word[1];
    const int byte0 = (cb * 8 + 2 * ge) * 4;
    if (COMPACT) {                  // the block's sign string of this row: to LDS, the key bytes are cut from it below
      *reinterpret_cast<u32x2*>(cw_lds + (wave * kWaveRows + 16 * rt + r16e) * 8 + 2 * ge) = u32x2{w0, w1};
    } else {
      const u32x2 live = *reinterpret_cast<const u32x2*>(live_lds + 2 * ge);
      w0 &= live[0];
      w1 &= live[1];
      if (grow < args.n) {
        uint8_t* dst = args.keys + grow * (int64_t)args.row_bytes + byte0;
        if (args.vec_store && byte0 + 8 <= args.row_bytes) {
          *reinterpret_cast<u32x2*>(dst) = u32x2{w0, w1};
        } else {
#pragma unroll
          for (int bsel = 0; bsel < 4; ++bsel) {
            if (byte0 + bsel < args.row_bytes) dst[bsel] = (uint8_t)(w0 >> (8 * bsel));
            if (byte0 + 4 + bsel < args.row_bytes) dst[4 + bsel] = (uint8_t)(w1 >> (8 * bsel));
          }
        }
      }
    }
  }

  // ---- the workgroup's flagged projections: one global append ------------------------------------------------------
  __syncthreads();
  if (COMPACT) {
    // key byte o of this block = bits [src, src + 8) of the row's 256-bit sign string, masked to the band's live rows
    const int bands_here = args.num_bands - cb * args.bpb < args.bpb ? args.num_bands - cb * args.bpb : args.bpb;
    const int nby = bands_here * args.band_bytes;
    const int byte_base = cb * args.bpb * args.band_bytes;
    const int* tab = args.bytetab + cb * 512;
    for (int idx = tid; idx < kRows * nby; idx += 64 * W) {
      const int rl = idx / nby, o = idx - rl * nby;
      const int64_t grow = blk_row0 + rl;
      if (grow < args.n) {
        const int src = tab[2 * o], w = src >> 5;
        const uint32_t lo = cw_lds[rl * 8 + w], hi = cw_lds[rl * 8 + (w < 7 ? w + 1 : 7)];
        args.keys[grow * (int64_t)args.row_bytes + byte_base + o] = (uint8_t)key_byte<false>(lo, hi, src, (uint32_t)tab[2 * o + 1]);
      }
    }
  }
  const int staged = l_count[0] < kS1ListCap ? l_count[0] : kS1ListCap;
  if (staged > 0 && args.col_cap > 0) {                 // buckets: every staged entry to its column's segment (one atomic on
    if (tid == 0) atomicAdd(args.tie_count, staged);    // one of <= 1024 addresses each: ~30 per workgroup at 768-d, ~60 at 1536-d)
    for (int e = tid; e < staged; e += 64 * W) {
      const int64_t entry = l_list[e];
      const int col = entry_col(entry);
      const int slot = atomicAdd(args.col_count + col, 1);
      if (slot < args.col_cap) {
        args.tie_list[(size_t)col * args.col_cap + slot] = entry;
        args.flag_y[(size_t)col * args.col_cap + slot] = l_y[e];
      }
    }
  } else if (staged > 0) {                              // (workgroup-uniform)
    if (tid == 0) l_count[1] = atomicAdd(args.tie_count, staged);
    __syncthreads();
    const int base = l_count[1];
    for (int e = tid; e < staged; e += 64 * W) {
      const int slot = base + e;
      if (slot < args.tie_cap) {
        args.tie_list[slot] = l_list[e];
        if (args.flag_y != nullptr) args.flag_y[slot] = l_y[e];
      }
    }
  }
  if (args.clock_probe != nullptr && tid == 0) {
    const unsigned long long slot = (unsigned long long)gridDim.x + (unsigned long long)blockIdx.x;
    args.clock_probe[2 * slot] = __builtin_amdgcn_s_memtime() - t_shader;
    args.clock_probe[2 * slot + 1] = __builtin_amdgcn_s_memrealtime() - t_real;
  }
}

}  // namespace

uint32_t lshrs_flags_sig16(void) {
  uint32_t f = 0;
#ifdef LSHRS_AB_NO_XMID_NORM
  f |= LSHRS_BUILD_WRONG_KEYS | (1u << 11);
#endif
#ifdef LSHRS_AB_NO_STATIC_PRIO
  f |= LSHRS_BUILD_TUNED | (1u << 16);
#endif
#ifdef LSHRS_T16_BUILTIN
  f |= LSHRS_BUILD_TUNED | (1u << 20);
#endif
#if LSHRS_X_AUX != 0
  f |= LSHRS_BUILD_TUNED | (1u << 21);
#endif
  return f;
}

int lshrs_launch_sig16(const SigArgs& a, unsigned grid, bool compact, bool partial, bool half, hipStream_t s, hipEvent_t start,
                       hipEvent_t stop) {
  const dim3 g(grid, 1, 1), b(half ? 256 : 512, 1, 1);
  dispatch_bool(half, [&](auto h) {          // (half: 128-row workgroups, two per CU - `grid` counts those)
    dispatch_bool(compact, [&](auto c) {
      dispatch_bool(partial, [&](auto p) {
        hipExtLaunchKernelGGL((sig16_kernel<decltype(c)::value, decltype(p)::value, decltype(h)::value ? 4 : 8>), g, b, 0, s, start, stop, 0, a);
      });
    });
  });
  return -(int)hipGetLastError();
}
