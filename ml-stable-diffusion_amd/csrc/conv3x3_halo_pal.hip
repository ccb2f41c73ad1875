// Palettized form of the K-split 3x3 / stride-1 halo convolution (plan tile 25): conv3x3_halo_pal_kernel and its launcher.  Geometry,
// ring schedule and epilogue are conv3x3_halo_ks_kernel's (conv3x3_halo.hip, plan tile 7) - an 8x16-pixel output tile x 64 output
// channels per workgroup, four waves = 2 pixel halves x 2 K halves, 64-channel chunks of nine tap steps, split-K over whole chunks
// through fp32 slabs, two concatenated sources switched on a chunk boundary, the nearest x2 upsample folded into the halo gather, rows
// outside the image read as zeros through the buffer range check, the counted waits of halo_ring.h - so the planner's tile counts,
// ring codes, split-K rule and workspace arithmetic are tile 7's, and so is the RESULT: the MFMAs (v_mfma_f32_32x32x16_f16), their
// operand order and the accumulation order over (chunk, tap, s) are tile 7's on the fp16 bit patterns the LUT holds, the epilogue is
// the statement tile 7 runs (halo_epilogue.inc, included by both; only the fetch of the bias / time-embedding row sits behind the K
// loop here: two registers the decode needs), so the plain store, the slabs and the GroupNorm statistics are bit-identical to tile 7
// on lut[indices] at the same ring code and split-K.  Workgroup placement and chunk walk: the statements of halo_ring.h.
//
// Only the weight side differs:
//   * HBM: the index stream of weight_prep.h halo_pal_pack - per (64-row n-tile, chunk, tap) one block of NBITS * 128 dwords, blocks in
//     the order a workgroup walks them, so the scalar DMA offset advances by the constant 512 * NBITS bytes per tap step.
//   * RING: ONE 1-KB DMA piece per wave and step (WR = 1, as tile 18) into stages of a fixed 4-KB pitch: thread t fetches bytes
//     [16 t, 16 t + 16) of the block; threads past its 512 * NBITS bytes carry the out-of-range offset and write zeros nobody reads.
//     Every wave issues exactly one weight DMA per step at every width, so the counted waits are uniform; the ring runs the depth the
//     ring code names (2 / 3 / 4 / 6 / 8 stages).
//   * FRAGMENTS: a lane reads its NBITS dwords of the stage (dword j of stream (wk, lane) at [j][wk][lane]: consecutive lanes,
//     consecutive banks) into registers and pal_decode (pal_decode.h) turns its 32 fields - every field position a compile-time
//     constant - into the four half8 fragments tile 7's read_step reads: field (2 s + j) * 8 + e is row j * 32 + (lane & 31), channel
//     (2 (2 wk + s) + (lane >> 5)) * 8 + e.  Each index is one 2-byte read of the LUT in LDS.  Reads and decode of step s+1 sit between
//     the MFMAs of step s, where tile 7 has its fragment reads; a tap step stays one basic block.
//   * LUT: 512 B (zero-padded, kPalLutHalves) behind the ring; it arrives as every wave's OLDEST DMA piece, in front of the first halo
//     piece, so every counted wait that covers weight tile 0 covers it.  All four waves fetch it to the same place (the same bytes);
//     lanes 32-63 carry the out-of-range offset and write zeros over the epilogue constants and the 256 B behind them
//     (halo_pal_lds_bytes), which nobody reads before the epilogue writes them.
//   * NOT HERE: GroupNorm in the loader, ablation builds, out modes other than the plain one.
// Why a file of its own: LAB_NOTES.md round 34 (one body for both changed the register allocation of the fp16 instantiations).  What
// the two share as text instead, and the proof that it left the generated code alone: round 35.
#include "igemm_device.h"
#include "halo_ring.h"
#include "pal_decode.h"
#include "weight_prep.h"

namespace sd {

namespace {

struct HaloPalArgs {
  IgemmArgs a;             // a.w unused
  const uint8_t* stream;   // halo_pal_pack
  const half_t* lut;       // [kPalLutHalves]
  unsigned stream_bytes;
};

template <int NBITS, int D>
__global__ __launch_bounds__(256, 2) void conv3x3_halo_pal_kernel(HaloPalArgs pa) {
  const IgemmArgs& a = pa.a;
  constexpr int BN = 64, BM = 128, WR = 1, ROWB = BK * 2;   // ROWB: bytes per LDS row of the halo
  constexpr int WSTAGE = kHaloPalStageBytes, BLOCKB = 512 * NBITS;   // a ring stage; the bytes of one block of the stream
  constexpr int XH_BYTES = 2 * HALO_LDS_ROWS * ROWB;
  static_assert(halo_ks_wait_count<D, WR>(1) <= 63 && (D - 1) * WR <= 63, "vmcnt range");
  static_assert(BLOCKB <= WSTAGE && WSTAGE == 4 * 1024, "a block fits a stage; a stage is one 1-KB piece per wave");
  static_assert(halo_pal_lds_bytes(D) == XH_BYTES + D * WSTAGE + 1024, "two halo buffers, the ring, LUT | constants | the LUT piece's tail");
  static_assert(XH_BYTES + D * WSTAGE + kPalLutHalves * 2 >= 32 * 1024 + BM * (BN + 8) * 2, "the epilogue's buffers end in front of its constants");
  static_assert(2 * halo_pal_lds_bytes(D) <= kLdsBudget, "two workgroups per CU");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Xh = smem;                                          // [2][HALO_LDS_ROWS][BK] halves
  char* const Ws = smem + XH_BYTES;                               // [D][4 KB]: a stage is one block of the stream
  char* const Lut = Ws + D * WSTAGE;                              // [kPalLutHalves] halves
  const unsigned short* const lutp = reinterpret_cast<const unsigned short*>(Lut);
  float* const sconst = reinterpret_cast<float*>(Lut + kPalLutHalves * 2);   // [BN] bias + timestep-embedding row, written in the epilogue only

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wk = wave & 1;
  const int H = a.Ho, W = a.Wo;                 // output (= upsampled input) image; nearest-x2 is folded into the halo gather
  const int ush = a.up >> 1;

  const int n_tiles = (a.N + BN - 1) / BN;
  const int m_tiles = a.B * a.tiles_y * a.tiles_x;
  const int nwg = m_tiles * n_tiles;
  HALO_PLACE_WG                                 // -> bn_idx, mt
  const int b = mt / (a.tiles_y * a.tiles_x);
  const int trem = mt - b * (a.tiles_y * a.tiles_x);
  const int ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
  const int y0 = ty * 8, x0 = tx * 16;
  const int n_blk = bn_idx * BN;

  const int nch = a.Ctot / BK;
  const int split = blockIdx.y;
  const int ch_begin = split * a.nk_per_split;
  int ch_end = ch_begin + a.nk_per_split;
  if (ch_end > nch) ch_end = nch;

  constexpr unsigned kOob = 0x80000000u;
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(pa.stream), 0, (int)pa.stream_bytes, 0x00020000);
  const size_t xpix = (size_t)a.B * a.Hi * a.Wi;
  // this lane's 16 bytes of halo piece j: pixel * 128 + swizzled 16-B slot (< 128), or kOob outside the image.  The byte offset at
  // channel 0 of a source with C channels is pixel * 2 C + slot (C a multiple of 64): formed per chunk (HALO_PAL_SRC), so that one
  // register per piece lives through the tap steps where tile 7 keeps two (one per source) - the decode needs them
  unsigned hpix[HALO_PPW];
  // piece of slot j.  The 24th slot (wave 3, j = 5) has no piece of its own: it fetches piece 22 a second time (same bytes)
  auto piece_of = [&](int j) { return (wave + 4 * j < HALO_PIECES) ? wave + 4 * j : HALO_PIECES - 1; };
#pragma unroll
  for (int j = 0; j < HALO_PPW; ++j) {
    const int p = piece_of(j);
    const int hr = 8 * p + (lane >> 3);
    const int hy = hr / HALO_W, hx = hr - hy * HALO_W;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const bool ok = (hr < HALO_ROWS) && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const unsigned pix = (unsigned)((b * a.Hi + (iy >> ush)) * a.Wi + (ix >> ush));   // unet.py:498-500 nearest upsample
    const unsigned sw = (unsigned)(((lane & 7) ^ ((hx >> 1) & 7)) * 16);   // column-keyed swizzle
    hpix[j] = ok ? pix * 128u + sw : kOob;
  }
  const unsigned woff = tid * 16 < BLOCKB ? (unsigned)tid * 16u : kOob;   // this thread's 16 bytes of a block

  // the halo of one channel chunk: which of the two concatenated sources it comes from is decided once per chunk
  // (HALO_PAL_SRC - halo_ring.h's HALO_SRC with one register per piece - declares rs / soff for chunk `ch` as plain locals and off(j), this lane's byte offset of piece j in that source - formed
  // where the piece is issued, so that no array of offsets lives through the tap steps)
#define HALO_PAL_SRC(rs, off, soff, ch)                                                                                       \
  const bool rs##_second = (ch) * BK >= a.C0; /* wave-uniform */                                                           \
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(                                                     \
      const_cast<half_t*>(rs##_second ? a.x1 : a.x0), 0, (int)(xpix * (rs##_second ? a.C1 : a.C0) * 2), 0x00020000);       \
  const int soff = (rs##_second ? (ch) * BK - a.C0 : (ch) * BK) * 2;                                                       \
  const unsigned off##_pitch = (unsigned)((rs##_second ? a.C1 : a.C0) * 2);                                                \
  auto off = [&](int j_) { return hpix[j_] == kOob ? kOob : (hpix[j_] >> 7) * off##_pitch + (hpix[j_] & 127u); };
  auto issue_x_piece = [&](int j, const __amdgpu_buffer_rsrc_t& rs, unsigned off, int soff, int xstage) {
    dma16_to_lds(rs, Xh + xstage * (HALO_LDS_ROWS * ROWB) + piece_of(j) * 1024, off, soff);
  };
  // issue cursor of the weight ring: the blocks of (n-tile, chunk, tap) follow each other in the stream
  int iw_koff = (bn_idx * nch + ch_begin) * 9 * BLOCKB, iw_step = 0;
  auto issue_next_w = [&]() {
    dma16_to_lds(rs_w, Ws + ((unsigned)iw_step % D) * WSTAGE + wave * 1024, woff, iw_koff);
    ++iw_step;
    iw_koff += BLOCKB;
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31, hi = lane >> 5;
  // halo fragment byte offsets: this wave reads the 16-B chunks kc = 2 * (2 * wk + s) + hi, s = 0, 1 of every row
  // xaddr[kx][s]: halo row of this lane's pixel of block i = 0 (tap row 0) + the swizzled slot of chunk kc under column shift kx, in
  // bytes.  Block i = 1 lies two halo rows (32 pixels) further: an immediate offset, like the tap's row / column shift.
  constexpr int kBlockStride = 2 * HALO_W * ROWB;
  int xaddr[3][2];
  {
    const int ml = wm * 64 + frow, hx0 = frow & 15;
    const int hrb = ((ml >> 4) * HALO_W + (ml & 15)) * ROWB;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int kc = 2 * (2 * wk + s) + hi;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) xaddr[kx][s] = hrb + (kc ^ (((hx0 + kx) >> 1) & 7)) * 16;
    }
  }
  const int pal_off = (wk * 64 + lane) * 4;               // dword 0 of this lane's stream in a stage; dword j lies 512 j bytes behind

  constexpr int Q = (NBITS + 3) / 4;                      // the lane's NBITS dwords as pal_decode takes them
  // the raw reads of a step: the halo fragments (tile 7's) and the lane's NBITS dwords of the stage
  // (xs / ws: byte offsets in the LDS, wave-uniform.  They pass through an empty asm, so that every step forms its addresses anew:
  // the compiler otherwise keeps the sums of the taps that share a column shift in registers across three steps)
  auto read_step = [&](half8 (&xf)[2][2], uintx4 (&wq)[Q], int xs, int ws, int tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    const int toffb = (ky * HALO_W + kx) * ROWB;
    asm volatile("" : "+s"(xs), "+s"(ws));
#pragma unroll
    for (int j = 0; j < 4 * Q; ++j) wq[j >> 2][j & 3] = j < NBITS ? *reinterpret_cast<const unsigned*>(smem + ws + pal_off + j * 512) : 0u;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i) xf[s][i] = *reinterpret_cast<const half8*>(smem + xs + xaddr[kx][s] + toffb + i * kBlockStride);
  };
  // MFMA order: tile 7's mfma_step - (s, i, j) ascending.  Behind the pair (s, i, *) goes the decode of weight fragment 2 s + i of
  // the NEXT step (-> nw[s][i]): eight LUT reads and their packing at a time, so that a quarter of the indices and looked-up halves
  // are in flight at once beside the accumulators and the two fragment sets
  auto mfma_decode_step = [&](half8 (&xf)[2][2], half8 (&wf)[2][2], half8 (*nw)[2], const uintx4 (&wq)[Q]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[s][j], xf[s][i], acc[i][j], 0, 0, 0);
        if (nw) nw[s][i] = pal_decode<NBITS, Q>(wq, 2 * s + i, lutp);
      }
  };

  half8 xfA[2][2], wfA[2][2], xfB[2][2], wfB[2][2];
  if (ch_begin < ch_end) {
    {   // the LUT: the oldest piece of every wave
      const __amdgpu_buffer_rsrc_t rs_lut = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(pa.lut), 0, kPalLutHalves * 2, 0x00020000);
      dma16_to_lds(rs_lut, Lut, lane * 16 < kPalLutHalves * 2 ? (unsigned)lane * 16u : kOob, 0);
      asm volatile("" ::: "memory");
    }
    HALO_PAL_SRC(rs0, off0, soff0, ch_begin)
#pragma unroll
    for (int j = 0; j < HALO_PPW; ++j) issue_x_piece(j, rs0, off0(j), soff0, 0);
#pragma unroll
    for (int p = 0; p < D; ++p) {   // (a K range holds >= 9 steps > D)
      asm volatile("" ::: "memory");                      // keep the DMA issue order: the counted wait below relies on it
      issue_next_w();
    }
    wait_vmcnt_barrier<(D - 1) * WR>();                   // the LUT, the first halo and weight tile 0 have landed
    uintx4 wq0[Q];
    read_step(xfA, wq0, 0, XH_BYTES, 0);
#pragma unroll
    for (int f = 0; f < 4; ++f) wfA[f >> 1][f & 1] = pal_decode<NBITS, Q>(wq0, f, lutp);
  }
  int st = 0;
  // One chunk = nine tap steps.  PAR = parity of the chunk's first step (which register set holds its fragments); LAST = the
  // final chunk of this workgroup's K range: no next halo, no weight tiles past the end, the waits count what is left.
  auto chunk = [&](auto par, auto last, int ch) {
    constexpr int PAR = decltype(par)::value;
    constexpr bool LAST = decltype(last)::value;
    const int xst = (ch - ch_begin) & 1;
    const bool first_chunk = ch == ch_begin;
    HALO_PAL_SRC(rsn, offn, soffn, (LAST ? ch : ch + 1))
#pragma unroll
    for (int tap = 0; tap < 9; ++tap, ++st) {
      auto body = [&](half8 (&cx)[2][2], half8 (&cw)[2][2], half8 (&nx)[2][2], half8 (&nw)[2][2]) {
        uintx4 wq[Q];
        if (LAST && tap == 8) {                           // the final step: nothing left to fetch
          mfma_decode_step(cx, cw, nullptr, wq);
          return;
        }
        // this wave's reads of ring stage st % D (the raw dwords of step st) are in registers: after the barrier NO wave reads it any more
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // weight block st+1 (at tap 8: and the next halo) has landed
        if constexpr (LAST) halo_ks_wait_last<D, WR>(tap);
        else if (D > 4 && first_chunk) {
          // fewer halo pieces behind the weight blocks than in steady state: count the blocks only - but at tap 8 the next
          // chunk's halo (last piece issued at tap 5, two steps = 2 * WR weight pieces ago) must have landed as well
          if (tap == 8) wait_vmcnt_barrier<((D - 2) * WR < 2 * WR ? (D - 2) * WR : 2 * WR)>();
          else wait_vmcnt_barrier<(D - 2) * WR>();
        }
        else halo_ks_wait<D, WR>(tap);
        const int tapn = tap == 8 ? 0 : tap + 1;
        const int xs = (tap == 8 ? xst ^ 1 : xst) * (HALO_LDS_ROWS * ROWB);
        const int ws = XH_BYTES + (int)((unsigned)(st + 1) % D) * WSTAGE;
        read_step(nx, wq, xs, ws, tapn);                  // halo fragments of step st+1 -> the other register set; its raw index dwords
        const bool w_live = !LAST || tap + D < 9;
        if (w_live) issue_next_w();                       // weight block st+D -> stage st % D
        const bool x_live = !LAST && tap < HALO_PPW;
        if (x_live) issue_x_piece(tap, rsn, offn(tap < HALO_PPW ? tap : 0), soffn, xst ^ 1);
        mfma_decode_step(cx, cw, nw, wq);                 // ... decoded into the other set's weight fragments between the MFMAs
      };
      if (((tap + PAR) & 1) == 0) body(xfA, wfA, xfB, wfB);
      else body(xfB, wfB, xfA, wfA);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  HALO_WALK_CHUNKS(chunk, ch_begin, ch_end)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                        // every wave is out of the K loop: LDS is free

  // ---- epilogue: tile 7's (halo_epilogue.inc); the bias / time-embedding row is fetched here, not in front of the K loop (two registers) ----
  float const_b = 0.f, const_t = 0.f;
  if (!a.slab && tid < BN && n_blk + tid < a.N) {
    if (a.bias) const_b = a.bias[n_blk + tid];
    if (a.temb) const_t = a.temb[(size_t)b * a.temb_stride + n_blk + tid];
  }
#define HALO_OUT_PIXEL(y, x) (b * H + y) * W + x
#define HALO_GN_STATS true
#include "halo_epilogue.inc"
#undef HALO_OUT_PIXEL
#undef HALO_GN_STATS
}

#undef HALO_PAL_SRC

template <int NBITS, int D>
void launch_halo_pal_d(const HaloPalArgs& pa, hipStream_t s) {
  constexpr size_t lds = halo_pal_lds_bytes(D);
  auto k = conv3x3_halo_pal_kernel<NBITS, D>;
  static DynLdsOnce once;
  once.set(k, lds);
  const IgemmArgs& a = pa.a;
  dim3 grid(a.B * a.tiles_x * a.tiles_y * cdiv(a.N, 64), a.splitk);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, s, pa);
}

}  // namespace

// plan tile 25.  Returns the GroupNorm partial entries per (sample, group) the epilogue wrote (setup_gn_stats).
int launch_halo_pal(const ConvDesc& d, const ConvPlan& p, float* partial, hipStream_t s) {
  const int ctot = d.C0 + (d.x1 ? d.C1 : 0);
  SD_REQUIRE(halo_pal_ok(d) && d.cw.kind == WeightSource::PalHalo && d.cw.stream && d.cw.lut && palette_bits_ok(d.cw.bits), kInvalidArgument,
             "palettized halo conv: shape not eligible or no palettized weights (C0=%d C1=%d N=%d %dx%d up=%d bits=%d)", d.C0, d.C1, d.N, d.Ho, d.Wo, d.up,
             d.cw.bits);
  const size_t bytes = halo_pal_bytes(d.N, ctot, d.cw.bits);
  SD_REQUIRE(bytes < ((size_t)1 << 31), kInvalidArgument, "palettized halo conv: an index stream of %zu bytes is past the 32-bit buffer offsets", bytes);
  // (the kernel keeps pixel * 128 + slot per halo piece in 31 bits)
  SD_REQUIRE((size_t)d.B * d.Hi * d.Wi < ((size_t)1 << 24), kInvalidArgument, "palettized halo conv: %zu input pixels, the halo offsets hold 2^24", (size_t)d.B * d.Hi * d.Wi);
  HaloPalArgs pa;
  pa.a = planned_args(d, p, partial);
  set_tile_order(pa.a, p.bm, p.bn, true);
  const int gn_entries = setup_gn_stats(d, pa.a, 0);
  pa.a.nk_total = pa.a.Ctot / BK;   // the kernel walks 64-channel chunks
  pa.stream = d.cw.pal();
  pa.lut = d.cw.lut;
  pa.stream_bytes = (unsigned)bytes;
  pal_dispatch_bits(d.cw.bits, "palettized halo conv", [&](auto nb) {
    constexpr int NBITS = decltype(nb)::value;
    switch (p.stages) {
      case 2: launch_halo_pal_d<NBITS, 2>(pa, s); break;
      case 3: launch_halo_pal_d<NBITS, 3>(pa, s); break;
      case 4: launch_halo_pal_d<NBITS, 4>(pa, s); break;
      case 6: launch_halo_pal_d<NBITS, 6>(pa, s); break;
      case 8: launch_halo_pal_d<NBITS, 8>(pa, s); break;
      default: SD_REQUIRE(false, kInternal, "palettized halo conv: no kernel with a ring of %d stages", p.stages);
    }
  });
  return gn_entries;
}

}  // namespace sd
