// W8A8 form of the K-split 3x3 / stride-1 halo convolution (plan tile 18): conv3x3_halo_i8_kernel and its launcher.  The geometry is
// conv3x3_halo_ks_kernel's (conv3x3_halo.hip, plan tile 7) - an 8x16-pixel output tile x 64 output channels per workgroup, 64-channel
// chunks of nine tap steps, split-K over whole chunks, four waves = 2 pixel halves x 2 K halves, two concatenated sources switched on
// a chunk boundary, the nearest x2 upsample folded into the halo gather, rows outside the image read as zeros through the buffer range
// check, weight rows past N clamped - so the planner's tile counts, split-K rule and workspace arithmetic are tile 7's.  The
// semantics are wstream.hip's int8 source (plan tile 17; sd_weights_quantize_w8a8 in sd_mi355x.h): activations through ws_quantize8
// (quantize8.h) with ONE scale for both sources, int8 weights never -128, exact int32 sums over a workgroup's whole K range (the two
// K halves are added as int32 in the LDS exchange), one conversion to fp32, one product with cs[n] = fp32(s_a * s_w[n]), then tile 7's
// epilogue in its order - bias + time-embedding row, fp32 slabs when split, residual, GroupNorm statistics of the stored fp16 values -
// with ONE rounding to fp16 (tile 7 rounds in front of the residual and again behind it; here the residual meets the fp32 value, as in
// the slab combine, so that split or not, tile 17 or tile 18, a layer is one function of its inputs).
//
// What differs from tile 7, and why:
//   * WEIGHTS int8, tap-major [N][9 * Ctot] (weight_prep.h halo_i8_pack: tile 7's K order at one byte per weight), 64-byte rows per
//     (n, tap, chunk): a tap's 64 x 64-B tile is 4 KB = ONE 1-KB DMA piece per wave (tile 7: two).  LDS image [64 rows][4 x 16 B], the
//     16-B chunk kc of row r at position kc ^ ((r >> 2) & 3): a ds_read_b128 lane group ({0-3,12-15,20-27} / {4-11,16-19,28-31} of each
//     32-lane half, all reading the same kc) holds every row residue mod 4 four times, on rows whose (r >> 2) & 3 differ (0, 3, 1, 2
//     / 1, 2, 0, 3) - 16 distinct 16-B slots of the 256-B bank row.
//   * QUANTIZATION SITE: once per halo element per workgroup and chunk, by the wave that fetched it, on the schedule of tile 7's
//     GroupNorm loader: a wave issues the 1-KB fp16 pieces of the next chunk in tap steps 0-4 (two in step 0) into an fp16 STAGING
//     buffer and quantizes them in steps 3-7, when its counted wait says they have landed (rings of <= 4 stages).  The result goes to
//     a COMPACT int8 image, not over the fp16 bytes: a lane's 16 B of fp16 become 8 B, and the MFMA fragment is 16 consecutive channels
//     per lane - in place that fragment would straddle two lanes' slots of a 128-B row (an extra exchange), and the image would keep
//     tile 7's 128-B pitch, i.e. twice the LDS bytes per fragment read.  The compact image is double-buffered (the next chunk is written
//     while this one is read); the staging buffer is single (a piece is dead once its owner has quantized it, long before that wave
//     re-issues the slot).  The transform is branch-free (out-of-image lanes quantize the DMA's zeros to 0; the 24th slot re-fetches
//     and re-quantizes the wave's own previous piece: same bytes, same result), so a tap step stays one basic block.
//   * INT8 HALO IMAGE: 64 B per pixel, halo rows 20 pixels apart (not 18), chunk kc of pixel (hy, hx) at position kc ^ ((hx >> 2) & 3).
//     The slot of a fragment read is then ((hx & 3) * 4 + (kc ^ (hx >> 2) & 3)) mod 16 - a function of hx mod 16 alone (a halo row is
//     20 * 64 B = five bank rows) - and the 16 lanes of a group cover 16 consecutive columns (x = 0-3, 12-15 of one pixel row and 4-11
//     of the next) under every tap shift: conflict-free for all nine taps.  Pitch 18 would move the second row's residues by two
//     and collide with the first row's under kx = 1.
//   * MFMA: v_mfma_i32_32x32x32_i8 - a wave's K half of a chunk (32 channels) is ONE instruction per 32x32 block and tap: four MFMAs
//     and four ds_read_b128 per tap step and wave (tile 7: eight and eight).  Operand / result layout: bit 3 of sd_selftest_mfma.
//   * RING: 2 / 3 / 4 stages of 4 KB (the transform schedule needs D <= 4; a plan code that names a deeper ring runs the 4-stage one).
//     LDS: 23 KB staging + 2 x 12.75 KB int8 image + D x 4 KB: two workgroups per CU at every depth.
//   * NOT HERE: GroupNorm in the loader, ablation builds, out modes other than the plain one.
// Shared with tile 7 as text (halo_ring.h): workgroup placement, source switch, chunk walk.  NOT halo_epilogue.inc: this epilogue is
// another statement - int32 exchange, fp32 staging, one rounding.
#include "igemm_device.h"
#include "halo_ring.h"
#include "quantize8.h"

namespace sd {

namespace {

constexpr int XQ_PITCH = kHaloI8Pitch, XQ_BYTES = kHaloI8Rows * 64;   // the int8 halo image: conv_plan.h
constexpr int XS_BYTES = HALO_LDS_ROWS * BK * 2;                      // the fp16 staging buffer: 23 pieces of 1 KB
static_assert((HALO_ROWS + 3) / HALO_W * XQ_PITCH + 3 < kHaloI8Rows, "the last piece's rows past the halo stay inside the image");

struct HaloI8Args {
  IgemmArgs a;         // a.w unused
  const int8_t* wq;    // [N][9 * Ctot]
  const float* cs;     // [N] s_a * s_w[n]
  float inv_s;         // 1 / s_a
};

template <int D>
__global__ __launch_bounds__(256, 2) void conv3x3_halo_i8_kernel(HaloI8Args ha) {
  const IgemmArgs& a = ha.a;
  constexpr int BN = 64, BM = 128, WR = 1, WROWB = BK;   // WROWB: bytes per LDS weight row (64 int8 channels)
  static_assert(D >= 2 && D <= 4, "the quantization schedule needs rings of <= 4 stages");
  static_assert(halo_ks_wait_count<D, WR, true>(1) <= 63, "vmcnt range");
  static_assert(halo_i8_lds_bytes(D) >= XS_BYTES + 2 * XQ_BYTES + D * BN * WROWB + 2 * BN * 4, "K-loop buffers");
  static_assert(XS_BYTES + 2 * XQ_BYTES + D * BN * WROWB >= 32 * 1024, "the K-half exchange ends in front of the epilogue constants");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Xs = smem;                                  // [HALO_LDS_ROWS][BK] halves: staging, pixel-major, no swizzle
  char* const Xq = smem + XS_BYTES;                       // [2][kHaloI8Rows][64] int8
  char* const Ws = Xq + 2 * XQ_BYTES;                     // [D][BN][64] int8
  float* const sconst = reinterpret_cast<float*>(Ws + D * BN * WROWB);   // [BN] bias + timestep-embedding row | [BN] cs: epilogue only

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wk = wave & 1;
  const int H = a.Ho, W = a.Wo;
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
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(ha.wq), 0, (int)((size_t)a.N * a.K), 0x00020000);
  const size_t xpix = (size_t)a.B * a.Hi * a.Wi;
  unsigned hoff0[HALO_PPW], hoff1[HALO_PPW];   // byte offset of this lane's 16 bytes (8 channels) of halo piece j at channel 0
  int qoff[HALO_PPW];                          // where their 8 quantized bytes go in an int8 image
  // piece of slot j; the 24th slot (wave 3, j = 5) fetches and quantizes the wave's own previous piece a second time
  auto piece_of = [&](int j) { return (wave + 4 * j < HALO_PIECES) ? wave + 4 * j : wave + 4 * (j - 1); };
#pragma unroll
  for (int j = 0; j < HALO_PPW; ++j) {
    const int p = piece_of(j);
    const int hr = 8 * p + (lane >> 3);
    const int hy = hr / HALO_W, hx = hr - hy * HALO_W;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const bool ok = (hr < HALO_ROWS) && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const unsigned pix = (unsigned)((b * a.Hi + (iy >> ush)) * a.Wi + (ix >> ush));   // unet.py:498-500 nearest upsample
    const unsigned c8 = (unsigned)(lane & 7);
    hoff0[j] = ok ? pix * (unsigned)a.C0 * 2u + c8 * 16u : kOob;
    hoff1[j] = ok ? pix * (unsigned)a.C1 * 2u + c8 * 16u : kOob;
    qoff[j] = (hy * XQ_PITCH + hx) * 64 + (int)((c8 >> 1) ^ (unsigned)((hx >> 2) & 3)) * 16 + (int)(c8 & 1) * 8;
  }
  const int pchunk = tid & 3, lrow = tid >> 2;
  unsigned woff;
  {
    int n = n_blk + lrow;
    if (n > a.N - 1) n = a.N - 1;
    woff = (unsigned)n * (unsigned)a.K + (unsigned)(pchunk ^ ((lrow >> 2) & 3)) * 16u;
  }

  // the halo of one channel chunk: HALO_SRC (halo_ring.h), always two sources
  auto issue_x_piece = [&](int j, const __amdgpu_buffer_rsrc_t& rs, unsigned off, int soff) {
    dma16_to_lds(rs, Xs + piece_of(j) * 1024, off, soff);
  };
  // slot j of this wave: staging -> int8 image `xstage`.  Only called once the piece has landed (this wave's own DMA; no other wave
  // reads the staging buffer).  Branch-free: a tap step stays one basic block.
  const float inv_s = ha.inv_s;
  auto quantize_piece = [&](int j, int xstage) {
    const half8 raw = *reinterpret_cast<const half8*>(Xs + piece_of(j) * 1024 + lane * 16);
    *reinterpret_cast<uintx2*>(Xq + xstage * XQ_BYTES + qoff[j]) = ws_quantize8(raw, inv_s);
  };
  int iw_koff = ch_begin * BK, iw_tap = 0, iw_step = 0;   // issue cursor of the weight ring (koff in bytes)
  auto issue_next_w = [&]() {
    dma16_to_lds(rs_w, Ws + ((unsigned)iw_step % D) * (BN * WROWB) + wave * 1024, woff, iw_koff);
    ++iw_step;
    iw_koff += a.Ctot;                                    // next tap, same chunk
    if (++iw_tap == 9) {
      iw_tap = 0;
      iw_koff += BK - 9 * a.Ctot;                         // tap 0 of the next chunk
    }
  };

  intx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

  const int frow = lane & 31, hi = lane >> 5;
  const int kc = 2 * wk + hi;                             // this lane's 16 channels of a chunk: 16 * kc ..
  int hrb[2];                                             // int8 image row of this lane's pixel (tap (0,0)), in bytes
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ml = (wm * 2 + i) * 32 + frow;
    hrb[i] = ((ml >> 4) * XQ_PITCH + (ml & 15)) * 64;
  }
  const int hx0 = frow & 15;
  int xsw[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) xsw[kx] = (kc ^ (((hx0 + kx) >> 2) & 3)) * 16;
  const int wsw = frow * WROWB + (kc ^ ((frow >> 2) & 3)) * 16;

  float const_b = 0.f, const_t = 0.f, const_s = 0.f;
  if (tid < BN && n_blk + tid < a.N) {
    const_s = ha.cs[n_blk + tid];
    if (!a.slab) {
      if (a.bias) const_b = a.bias[n_blk + tid];
      if (a.temb) const_t = a.temb[(size_t)b * a.temb_stride + n_blk + tid];
    }
  }

  auto read_step = [&](intx4 (&xf)[2], intx4 (&wf)[2], const char* xs, const char* ws, int tap) {
    const int ky = tap / 3, kx = tap - ky * 3;
    const int toffb = (ky * XQ_PITCH + kx) * 64;
#pragma unroll
    for (int i = 0; i < 2; ++i) xf[i] = *reinterpret_cast<const intx4*>(xs + hrb[i] + toffb + xsw[kx]);
#pragma unroll
    for (int j = 0; j < 2; ++j) wf[j] = *reinterpret_cast<const intx4*>(ws + j * 32 * WROWB + wsw);
  };
  auto mfma_step = [&](intx4 (&xf)[2], intx4 (&wf)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[j], xf[i], acc[i][j], 0, 0, 0);
  };

  intx4 xfA[2], wfA[2], xfB[2], wfB[2];
  if (ch_begin < ch_end) {
    HALO_SRC(false, rs0, off0, soff0, ch_begin)
#pragma unroll
    for (int j = 0; j < HALO_PPW; ++j) issue_x_piece(j, rs0, off0[j], soff0);
#pragma unroll
    for (int p = 0; p < D; ++p) {   // (a K range holds >= 9 steps > D)
      asm volatile("" ::: "memory");                      // keep the DMA issue order: the counted wait below relies on it
      issue_next_w();
    }
    wait_vmcnt_barrier<(D - 1) * WR>();                   // this wave's first halo pieces and weight tile 0 have landed
#pragma unroll
    for (int j = 0; j < HALO_PPW; ++j) quantize_piece(j, 0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // every wave's share of the first int8 image is written
    read_step(xfA, wfA, Xq, Ws, 0);
  }
  int st = 0;
  // One chunk = nine tap steps.  PAR = parity of the chunk's first step (which register set holds its fragments); LAST = the
  // final chunk of this workgroup's K range: no next halo, no weight tiles past the end, the waits count what is left.
  auto chunk = [&](auto par, auto last, int ch) {
    constexpr int PAR = decltype(par)::value;
    constexpr bool LAST = decltype(last)::value;
    const int xst = (ch - ch_begin) & 1;
    HALO_SRC(false, rsn, offn, soffn, (LAST ? ch : ch + 1))
#pragma unroll
    for (int tap = 0; tap < 9; ++tap, ++st) {
      auto body = [&](intx4 (&cx)[2], intx4 (&cw)[2], intx4 (&nx)[2], intx4 (&nw)[2]) {
        if (LAST && tap == 8) {                           // the final step: nothing left to fetch
          mfma_step(cx, cw);
          return;
        }
        // this wave's fragment reads of step st are in registers and its quantized bytes of the last step are written: after the
        // barrier NO wave reads ring stage st % D any more, and at tap 8 the next int8 image is complete
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if constexpr (LAST) halo_ks_wait_last<D, WR>(tap);
        else halo_ks_wait<D, WR, true>(tap);              // weight tile st+1 has landed, and every piece issued in steps <= tap - (D - 1)
        const int tapn = tap == 8 ? 0 : tap + 1;
        const char* xs = Xq + (tap == 8 ? xst ^ 1 : xst) * XQ_BYTES;
        const char* ws = Ws + ((unsigned)(st + 1) % D) * (BN * WROWB);
        read_step(nx, nw, xs, ws, tapn);                  // fragments of step st+1 -> the other register set
        const bool w_live = !LAST || tap + D < 9;
        if (w_live) issue_next_w();                       // weight tile st+D -> stage st % D
        if (!LAST) {
          if (tap == 0) {
            issue_x_piece(0, rsn, offn[0], soffn);
            issue_x_piece(1, rsn, offn[1], soffn);
          } else if (tap <= 4) {
            issue_x_piece(tap + 1, rsn, offn[tap + 1 < HALO_PPW ? tap + 1 : 0], soffn);
          }
          // pieces issued in steps <= tap - 3 have landed behind the wait above (D <= 4): quantize them into the other image
          if (tap == 3) {
            quantize_piece(0, xst ^ 1);
            quantize_piece(1, xst ^ 1);
          } else if (tap >= 4 && tap <= 7) {
            quantize_piece(tap - 2, xst ^ 1);
          }
        }
        mfma_step(cx, cw);
      };
      if (((tap + PAR) & 1) == 0) body(xfA, wfA, xfB, wfB);
      else body(xfB, wfB, xfA, wfA);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  HALO_WALK_CHUNKS(chunk, ch_begin, ch_end)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();                                        // every wave is out of the K loop: LDS is free

  // ---- epilogue.  acc[i][j][r]: n = j*32 + (r&3) + 8*(r>>2) + 4*hi ; pixel block 2*wm + i, pixel frow ----
  // sum the two K halves, in int32: wave (wm, wk) keeps pixel block 2*wm + wk and hands the other one to its partner
  {
    intx4* red = reinterpret_cast<intx4*>(smem);          // [4 waves][2 j][4 q][64 lanes] = 32 KB
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        intx4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = wk ? acc[0][j][4 * q + e] : acc[1][j][4 * q + e];
        red[((wave * 2 + j) * 4 + q) * 64 + lane] = v;
      }
    if (tid < BN) {
      sconst[tid] = const_b + const_t;
      sconst[BN + tid] = const_s;
    }
    __syncthreads();
  }
  floatx16 fin[2];   // one conversion, one product with the column's scale
  {
    const intx4* red = reinterpret_cast<const intx4*>(smem);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const intx4 v = red[(((wave ^ 1) * 2 + j) * 4 + q) * 64 + lane];
        const floatx4 cs = *reinterpret_cast<const floatx4*>(sconst + BN + j * 32 + 8 * q + 4 * hi);   // 0 beyond N
#pragma unroll
        for (int e = 0; e < 4; ++e) fin[j][4 * q + e] = (float)((wk ? acc[1][j][4 * q + e] : acc[0][j][4 * q + e]) + v[e]) * cs[e];
      }
  }
  const int ml = (wm * 2 + wk) * 32 + frow;               // tile-local pixel of this lane
  if (a.slab) {
    const int y = y0 + (ml >> 4), x = x0 + (ml & 15);
    if (y < H && x < W) {
      const int m = (b * H + y) * W + x;
      float* prow = a.partial + ((size_t)split * a.M + m) * a.N;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n_blk + j * 32 + 8 * q + 4 * hi;
          if (n < a.N) {
            floatx4 v = {fin[j][4 * q], fin[j][4 * q + 1], fin[j][4 * q + 2], fin[j][4 * q + 3]};
            out_store(reinterpret_cast<floatx4*>(prow + n), v);
          }
        }
    }
    return;
  }
  // The tile is staged in fp32 (tile 7 stages fp16): the residual is added to the fp32 value and the sum rounded to fp16 ONCE, as the slab
  // combine does - so a layer is the same function of its inputs split or not, and from either int8 kernel.  The staging buffer lies
  // behind the GroupNorm scratch and over the reduction buffer, which every wave has read by the barrier in front.
  constexpr int OROW = BN + 4;
  constexpr int kStage = (kGnScratchFloats + 2 * BN) * 4;
  static_assert(kStage % 16 == 0 && kStage + BM * OROW * 4 <= XS_BYTES + 2 * XQ_BYTES + D * BN * WROWB, "fp32 staging in front of the epilogue constants");
  float* ot = reinterpret_cast<float*>(smem + kStage);    // [BM][OROW]
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int nl = j * 32 + 8 * q + 4 * hi;
      const floatx4 bb = *reinterpret_cast<const floatx4*>(sconst + nl);   // 0 beyond N
      floatx4 o = {fin[j][4 * q] + bb[0], fin[j][4 * q + 1] + bb[1], fin[j][4 * q + 2] + bb[2], fin[j][4 * q + 3] + bb[3]};
      *reinterpret_cast<floatx4*>(ot + ml * OROW + nl) = o;
    }
  __syncthreads();
  constexpr int WC = BN / 8;
  const bool gn = a.gn_partial != nullptr;   // block-uniform (launch_conv: N % 8 == 0)
  float fs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, fq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int idx = tid; idx < BM * WC; idx += 256) {
    const int r = idx / WC, c = idx - r * WC;
    const int y = y0 + (r >> 4), x = x0 + (r & 15);
    const int n = n_blk + c * 8;
    if (y < H && x < W && n < a.N) {
      const size_t m = (size_t)(b * H + y) * W + x;
      const floatx4 f0 = *reinterpret_cast<const floatx4*>(ot + r * OROW + c * 8), f1 = *reinterpret_cast<const floatx4*>(ot + r * OROW + c * 8 + 4);
      float f[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
      half_t* dst = a.out + m * a.N + n;
      half8 v;
      if (n + 8 <= a.N) {
        if (a.res) {
          const half8 rr = *reinterpret_cast<const half8*>(a.res + m * a.N + n);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] += (float)rr[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (half_t)f[e];
        out_store(reinterpret_cast<half8*>(dst), v);
        if (gn) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float f = (float)v[e];
            fs[e] += f;
            fq[e] = fmaf(f, f, fq[e]);
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)   // ragged last chunk (N % 8 == 4): four single stores
          if (e < a.N - n) dst[e] = (half_t)(a.res ? f[e] + (float)a.res[m * a.N + n + e] : f[e]);
      }
    }
  }
  // GroupNorm statistics of the stored pixels, as tile 7 leaves them (the scratch is the K-half reduction buffer)
  if (gn) tile_gn_stats<BN>(a, reinterpret_cast<float*>(smem), fs, fq, n_blk, b, ty * a.tiles_x + tx);
}

template <int D>
void launch_halo_i8_d(const HaloI8Args& ha, hipStream_t s) {
  constexpr size_t lds = halo_i8_lds_bytes(D);
  static_assert(2 * lds <= kLdsBudget, "two workgroups per CU");
  auto k = conv3x3_halo_i8_kernel<D>;
  static DynLdsOnce once;
  once.set(k, lds);
  const IgemmArgs& a = ha.a;
  dim3 grid(a.B * a.tiles_x * a.tiles_y * cdiv(a.N, 64), a.splitk);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, s, ha);
}

}  // namespace

// plan tile 18.  Returns the GroupNorm partial entries per (sample, group) the epilogue wrote (setup_gn_stats).
int launch_halo_i8(const ConvDesc& d, const ConvPlan& p, float* partial, hipStream_t s) {
  SD_REQUIRE(halo_ks_ok(d) && d.cw.kind == WeightSource::I8Halo && d.cw.stream && d.cw.scale && d.cw.inv_s > 0.f && std::isfinite(d.cw.inv_s) &&
                 !d.gnf_partial && !d.debug && d.C0 + (d.x1 ? d.C1 : 0) <= kHaloI8MaxCtot,
             kInvalidArgument, "int8 halo conv: shape not eligible or no int8 weights (C0=%d C1=%d N=%d %dx%d up=%d)", d.C0, d.C1, d.N, d.Ho, d.Wo, d.up);
  HaloI8Args ha;
  ha.a = planned_args(d, p, partial);
  set_tile_order(ha.a, p.bm, p.bn, true);
  const int gn_entries = setup_gn_stats(d, ha.a, 0);
  ha.a.nk_total = ha.a.Ctot / BK;   // the kernel walks 64-channel chunks
  ha.wq = d.cw.i8();
  ha.cs = d.cw.scale;
  ha.inv_s = d.cw.inv_s;
  switch (p.stages) {
    case 2: launch_halo_i8_d<2>(ha, s); break;
    case 3: launch_halo_i8_d<3>(ha, s); break;
    case 4: launch_halo_i8_d<4>(ha, s); break;
    default: SD_REQUIRE(false, kInternal, "int8 halo conv: no kernel with a ring of %d stages", p.stages);
  }
  return gn_entries;
}

}  // namespace sd
