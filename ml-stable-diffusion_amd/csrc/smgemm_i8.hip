// W8A8 form of the small-M 1x1 GEMM (plan tile 19): smgemm_i8_kernel and its launcher.  The geometry is smgemm_kernel's (smgemm.hip,
// plan tile 12) - five waves over a BM x 80 tile, BM = 32 / 64, wave w owns output columns 16 w .. 16 w + 15 of all BM rows, one
// workgroup per tile in the XCD runs of sm_tile.h behind its division-free prologue, epilogue from the accumulators through sm_swap16
// with no LDS and no barrier - so tile order, tile counts and eligibility (smgemm_shape_ok) are tile 12's.  One source only.
// The semantics are the int8 weight stream's (wstream.hip, plan tile 17; sd_weights_quantize_w8a8 in sd_mi355x.h): activations through
// ws_quantize8 (quantize8.h), int8 weights never -128, exact int32 sums over the WHOLE K (no split-K, no slab: 127 * 127 * K < 2^31,
// kSmI8MaxK), one conversion to fp32, one product with cs[n] = fp32(s_a * s_w[n]), then
//     out = fp16(((float(acc) * cs[n]) + bias[n]) + float(res[m][n]))
// with ONE rounding to fp16: the residual meets the fp32 value.  That is the order of splitk_reduce_kernel behind a one-slab launch of
// tile 17, so a shape both kernels take is bit-identical between tiles 17 and 19.  It is NOT tile 12's epilogue, which rounds to fp16
// in front of the residual and again behind it.  The product and the two sums are rounded to fp32 one by one (sm_i8_affine and
// gemm_value, fp contract off): tile 17 adds its bias to a product that went through memory, so an fma here would be another function.
//
// What differs from tile 12, and why:
//   * WEIGHTS int8 [N][K] as the checkpoint holds them (weight_prep.h smgemm_i8_pack), through the LDS-DMA ring.  A wave's 16 weight
//     rows of a K64 stage are 16 x 64 B = ONE 1-KB piece, so every wave fetches its own strip and nobody else reads it.  LDS image
//     and fragment read: the piece of sm_i8_ring.h (sm_i8_swz), with its bank-conflict argument.
//   * MFMA: v_mfma_i32_16x16x64_i8 - ONE instruction per 16 x 16 block and K64 stage (tile 12: two).  Operand / result layout: bit 4 of
//     sd_selftest_mfma.  (A and B share the lane -> k map, so the sums do not depend on it; the result layout is tile 12's.)
//   * QUANTIZATION SITE: once per activation element per workgroup, not once per wave.  All five waves consume the same BM activation
//     rows; the fp16 pieces (8 rows x 128 B) go by LDS-DMA into a STAGING part of the ring stage, the wave that fetched a piece
//     quantizes it when its own counted wait says it has landed, and writes 8 rows x 64 B into a COMPACT int8 image [BM rows][64 B]
//     with the swizzle above, double-buffered by stage parity.  Every wave reads its B fragments from that image.
//   * NO ORDINARY GLOBAL LOAD in the K loop: every byte arrives as a counted 1-KB piece.  A wave issues PPW = 1 + ceil(BM / 8 / 5)
//     pieces per stage - its weight strip first, then its activation pieces; the BM / 8 real activation pieces are dealt to the waves
//     (smi_piece) and the padding pieces repeat activation rows into a dump slot behind the image that nothing reads - so one immediate serves all.
//     Bias, cs and the residual (in the ACCUMULATOR layout: 8 B per lane and block, because it must meet the fp32 value in front of the
//     exchange) are requested right behind the first NST - 1 ring stages and counted in the same vmcnt.
//   * RING: 16 stages of 9 KB (BM = 32), 11 of 13 KB (BM = 64): 5 KB of weights + BM x 128 B of staging each; with 2 x BM x 64 B of
//     image and the dump slots 149 / 153 KB of the 160.
// The K loop, step s (stage s is multiplied; NST the ring depth):
//     [wait: this wave's pieces of stage s + 1 have landed | lgkmcnt(0) | s_barrier]
//     issue stage s + NST - 1 -> slot (s - 1) % NST;  read the weight fragment of stage s and the B fragments of image s & 1;
//     quantize this wave's pieces of stage s + 1 -> image (s + 1) & 1;  MFMAs of stage s
// and in front of step 0 a counted wait for stage 0 and its quantization into image 0.  One barrier per K64 stage:
//   * image (s + 1) & 1 is image (s - 1) & 1.  Its last readers are the fragment reads of step s - 1; every wave has them in registers
//     (lgkmcnt(0)) before it arrives at the barrier of step s, and the writes of stage s + 1 are issued behind that barrier.  The
//     readers of stage s + 1's image are behind the barrier of step s + 1, which every wave reaches with its writes done (lgkmcnt(0)).
//   * the ring itself is wave-private - a wave reads only the weight strip and the staging pieces it fetched - so its slots need no
//     barrier: slot (s - 1) % NST held stage s - 1, whose weight fragment this wave read in step s - 1 and whose staging pieces it
//     quantized in step s - 2, both finished by the lgkmcnt(0) in front of the issue.
//   * counted wait of step s: issued are stages 0 .. min(s + NST - 2, nk - 1), needed is stage min(s + 1, nk - 1); younger than it are
//     max(0, min(NST - 3, nk - 2 - s)) stages of PPW pieces and, while s + 1 <= NST - 2, the EPI epilogue loads.  In front of step 0:
//     min(NST - 2, nk - 1) stages and the epilogue loads.
// NOT HERE: a second source, GEGLU, the LayerNorm fold, GroupNorm statistics, out modes other than the plain one - what sm_tiles
// refuses, plus x1.
#include "conv_plan.h"
#include "kernels.h"
#include "quantize8.h"
#include "sm_i8_ring.h"
#include "weight_prep.h"

namespace sd {

namespace {

constexpr int SMI_BK = SM_I8_BK;        // K per ring stage: 64-B weight rows, 128-B activation rows
constexpr int SMI_BN = 80;              // output columns per workgroup
constexpr int SMI_NW = SMI_BN / 16;     // waves: one 16-column strip each

struct SmI8Args {
  const half_t* x;      // [M][K]
  const int8_t* w;      // [N][K]
  const float* cs;      // [N] s_a * s_w[n]
  const float* bias;    // [N]; has_bias == 0: any readable float[N] (the loads keep their count)
  const half_t* res;    // [M][res_ld]; has_res == 0: any readable half[N] with res_ld = 0
  half_t* out;          // [M][N]
  float inv_s;          // 1 / s_a
  int K, N, nk, res_ld;
  int has_bias, has_res;
  SmTileOrder order;
};

template <int BM>
struct SmI8Cfg {
  static constexpr int XP = BM / 8;                              // 1-KB pieces of real activation rows per stage
  static constexpr int XPW = (XP + SMI_NW - 1) / SMI_NW;         // activation pieces per wave per stage
  static constexpr int PPW = 1 + XPW;                            // pieces per wave per stage: the weight strip first
  static constexpr int PAD = SMI_NW * XPW - XP;                  // padding pieces per stage: into the dump slots
  static constexpr int XS = SMI_NW * 1024;                       // a stage: [5 weight strips | XP staging pieces]
  static constexpr int STAGE = XS + XP * 1024;
  static constexpr int NST = BM == 32 ? 16 : 11;                 // ring depth
  static constexpr int IMG = BM * 64;                            // one int8 image
  static constexpr int IMAGES = NST * STAGE;                     // byte offsets behind the ring
  static constexpr int DUMP = IMAGES + 2 * IMG;
  static constexpr int LDS = DUMP + PAD * 1024;
  static constexpr int TM = BM / 16;                             // 16 x 16 accumulator blocks per wave
  static constexpr int EPI = 2 + TM;                             // epilogue loads per lane: bias, cs, one residual quad per block
  static_assert(BM % 32 == 0 && XP * 8 == BM && PAD >= 0 && PAD < SMI_NW, "tile");
  static_assert(NST >= 3 && LDS <= SM_I8_LDS, "LDS budget");
  static_assert(PPW * (NST - 2) + EPI <= 63, "vmcnt range");
};

// The activation piece of slot j of wave w; >= XP: a padding piece (dump slot piece - XP).  Slot 0: piece w.  Slot 1 (BM = 64): pieces
// 5 - 7 go to waves 1 - 3, not 0 - 2: five waves on four SIMDs put waves 0 and 4 on one SIMD when they are placed round robin, and the
// quantization is the longest stretch of a stage - so those two get one piece each, and no SIMD quantizes more than two.
template <int XP>
__device__ __forceinline__ int smi_piece(int wave, int j) {
  static_assert(XP == 4 || XP == 8, "slot 1 exists at BM = 64 only, with three real pieces");
  if (j == 0) return wave;
  return wave >= 1 && wave <= 3 ? SMI_NW - 1 + wave : XP + (wave == 0 ? 0 : 1);
}

template <int BM>
__global__ __launch_bounds__(64 * SMI_NW, 1) void smgemm_i8_kernel(SmI8Args a) {
  using C = SmI8Cfg<BM>;
  constexpr int NST = C::NST, PPW = C::PPW, XPW = C::XPW, XP = C::XP, TM = C::TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

  int m_tile, n_tile;
  sm_tile_coords(a.order, m_tile, n_tile);
  const int m_blk = m_tile * BM, n_blk = n_tile * SMI_BN;
  const int g = lane >> 4, r16 = lane & 15;

  // ---- staging: this wave's weight strip (16 rows x 64 B, lane = 4 row + position), then its activation pieces (8 rows x 128 B) ----
  const int8_t* wsrc;
  {
    const int r = lane >> 2;
    wsrc = a.w + (size_t)(n_blk + 16 * wave + r) * a.K + sm_i8_swz(lane & 3, r) * 16;   // logical chunk at position lane & 3 (position = chunk ^ F, so chunk = position ^ F)
  }
  const half_t* xsrc[XPW];
  int qoff[XPW];   // where this lane's 8 quantized bytes of piece j go in an image
#pragma unroll
  for (int j = 0; j < XPW; ++j) {
    const int p = smi_piece<XP>(wave, j);
    const int pr = p >= XP ? p - XP : p;                  // the padding pieces repeat activation rows
    const int r = pr * 8 + (lane >> 3), c8 = lane & 7;    // activation row of the tile, its 8 channels 8 c8 ..
    xsrc[j] = a.x + (size_t)(m_blk + r) * a.K + c8 * 8;
    qoff[j] = r * 64 + sm_i8_swz(c8 >> 1, r) * 16 + (c8 & 1) * 8;
  }
  // ring stage idx (< nk) into slot idx % NST
  auto issue = [&](int idx) __attribute__((always_inline)) {
    char* st = smem + (idx % NST) * C::STAGE;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)wsrc,
                                     (__attribute__((address_space(3))) void*)(st + wave * 1024), 16, 0, 0);
    wsrc += SMI_BK;
#pragma unroll
    for (int j = 0; j < XPW; ++j) {
      const int p = smi_piece<XP>(wave, j);               // wave-uniform
      char* dst = p >= XP ? smem + C::DUMP + (p - XP) * 1024 : st + C::XS + p * 1024;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)xsrc[j],
                                       (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      xsrc[j] += SMI_BK;
    }
  };
  // this wave's real pieces of stage idx: staging -> image idx & 1.  Only called once they have landed (its own DMA; no other wave
  // reads the staging part)
  const float inv_s = a.inv_s;
  auto quantize = [&](int idx) __attribute__((always_inline)) {
    const char* st = smem + (idx % NST) * C::STAGE + C::XS;
    char* img = smem + C::IMAGES + (idx & 1) * C::IMG;
#pragma unroll
    for (int j = 0; j < XPW; ++j) {
      const int p = smi_piece<XP>(wave, j);
      if (p < XP) {                                       // wave-uniform
        const half8 raw = *reinterpret_cast<const half8*>(st + p * 1024 + lane * 16);
        *reinterpret_cast<uintx2*>(img + qoff[j]) = ws_quantize8(raw, inv_s);
      }
    }
  };

#pragma unroll
  for (int p = 0; p < NST - 1; ++p)
    if (p < a.nk) issue(p);
  // the epilogue operands right behind the first ring stages, in the accumulator layout: bias and cs of this lane's four columns, the
  // residual quad of each block (has_res == 0: a readable dummy row, so that every wave counts the same loads)
  __builtin_amdgcn_sched_barrier(0);
  const int ncol = n_blk + 16 * wave + 4 * g;
  const floatx4 bias4 = *reinterpret_cast<const floatx4*>(a.bias + ncol);
  const floatx4 cs4 = *reinterpret_cast<const floatx4*>(a.cs + ncol);
  half4 resv[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) resv[i] = *reinterpret_cast<const half4*>(a.res + (size_t)(m_blk + 16 * i + r16) * a.res_ld + ncol);
  __builtin_amdgcn_sched_barrier(0);

  // fragment offset inside a weight strip and inside a 16-row block of an image: row r16, logical chunk g
  const int foff = r16 * 64 + sm_i8_swz(g, r16) * 16;

  intx4 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) acc[i] = intx4{0, 0, 0, 0};

  // stage 0 has landed for this wave -> image 0 (the barrier of this wait is not needed, and harmless)
  sm_wait<PPW, C::EPI, NST - 2, true>(min(NST - 2, a.nk - 1));
  quantize(0);

  for (int s = 0; s < a.nk; ++s) {
    const int ahead = max(0, min(NST - 3, a.nk - 2 - s));
    if (s <= NST - 3) sm_wait<PPW, C::EPI, NST - 3, true>(ahead);
    else sm_wait<PPW, 0, NST - 3, true>(ahead);
    if (s + NST - 1 < a.nk) issue(s + NST - 1);
    const char* st = smem + (s % NST) * C::STAGE + wave * 1024;
    const char* img = smem + C::IMAGES + (s & 1) * C::IMG;
    const intx4 wf = *reinterpret_cast<const intx4*>(st + foff);
    intx4 xf[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) xf[i] = *reinterpret_cast<const intx4*>(img + i * 16 * 64 + foff);
    if (s + 1 < a.nk) quantize(s + 1);
#pragma unroll
    for (int i = 0; i < TM; ++i)   // rows = n, cols = m: lane holds n = 4 g + e of row m = r16 of block i
      acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, xf[i], acc[i], 0, 0, 0);
  }

  // ---- epilogue: one conversion, one product, bias and residual in fp32, ONE rounding; blocks (2p, 2p + 1) paired by sm_pack16 ->
  // 16 B of one output row per lane ----
  const int n = n_blk + 16 * wave + 8 * (g >> 1);
#pragma unroll
  for (int p = 0; p < TM / 2; ++p) {
    uintx2 h[2];   // block 2p | block 2p + 1: columns 4 g .. 4 g + 3 in fp16
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      floatx4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = gemm_value(acc[2 * p + b][e], cs4[e], bias4[e], a.has_bias != 0, (float)resv[2 * p + b][e], a.has_res != 0);
      h[b] = sm_round4(v);
    }
    const half8 o = sm_pack16(h[0], h[1]);
    const int m = m_blk + 32 * p + 16 * (g & 1) + r16;
    out_store(reinterpret_cast<half8*>(a.out + (size_t)m * a.N + n), o);
  }
}

}  // namespace

bool smgemm_i8_shape_ok(const ConvDesc& d, int variant) { return smgemm_shape_ok(d, variant) && !d.x1 && d.C0 <= kSmI8MaxK; }

void launch_smgemm_i8(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  const int bm = p.bm;
  SD_REQUIRE((bm == 32 || bm == 64) && smgemm_i8_shape_ok(d, bm == 32 ? 1 : 2) && d.cw.kind == WeightSource::I8Gemm && d.cw.stream && d.cw.scale &&
                 d.cw.inv_s > 0.f && std::isfinite(d.cw.inv_s),
             kInvalidArgument, "plan tile 19 (smgemm_i8.hip, int8): not a single-source 1x1 GEMM it tiles, or no int8 weights (C0=%d C1=%d N=%d M=%d)",
             d.C0, d.x1 ? d.C1 : 0, d.N, d.B * d.Ho * d.Wo);
  const int M = d.B * d.Ho * d.Wo, K = d.C0;
  SmI8Args a;
  a.x = d.x0;
  a.w = d.cw.i8();
  a.cs = d.cw.scale;
  a.bias = d.bias ? d.bias : d.cw.scale;                                   // absent: the scales stand in, N floats (the loads keep their count)
  a.res = d.res ? d.res : reinterpret_cast<const half_t*>(d.cw.scale);     // ... and N halves of them for a residual row
  a.out = d.out;
  a.inv_s = d.cw.inv_s;
  a.K = K;
  a.N = d.N;
  a.nk = K / SMI_BK;
  a.res_ld = d.res ? d.N : 0;
  a.has_bias = d.bias != nullptr;
  a.has_res = d.res != nullptr;
  a.order = sm_tile_order(M, d.N, K, M / bm, d.N / SMI_BN);   // tile 12's order, from the fp16 sizes
  conv_plan_log(d, p, a.order.n_fast);
  const unsigned nwg = 8 * a.order.per_xcd;   // one workgroup per tile: 8 XCD runs
  if (bm == 32) sm_i8_launch<smgemm_i8_kernel<32>>(a, nwg, SMI_NW, SmI8Cfg<32>::LDS, s);
  else sm_i8_launch<smgemm_i8_kernel<64>>(a, nwg, SMI_NW, SmI8Cfg<64>::LDS, s);
  SD_HIP(hipGetLastError());
}

}  // namespace sd
