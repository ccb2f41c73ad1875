// W8A8 form of the GEGLU projection (plan tile 20): smgeglu_i8_kernel and its launcher.  The geometry is smgeglu_kernel's (smgeglu.hip,
// plan tile 13) - BM x 80 output columns = 160 weight rows in 16-column value / gate units, BM = 128 / 256, ten waves = 5 units x 2 row
// halves, one workgroup per tile in the XCD runs of sm_tile.h behind its division-free prologue, epilogue from the accumulators through
// sm_swap16 with no LDS and no barrier - so tile order, tile counts and eligibility (smgeglu_shape_ok) are tile 13's.
// The semantics are the int8 kernels' (sd_weights_quantize_w8a8 in sd_mi355x.h): int8 weights never -128, exact int32 sums over the WHOLE
// K (127 * 127 * K < 2^31, kSmI8MaxK), one conversion to fp32, one product with cs[n] = fp32(s_a * s_w[n]), the bias added in fp32 - each
// operation rounded on its own (sm_i8_affine) - and then tile 13's own ending, out = fp16(v * gelu_erf(g)).
// Stage, LDS image, piece distribution, issue, counted wait and the K loop's RAW / WAR and vmcnt arguments: sm_i8_ring.h.
//
// What differs from tile 13, and why:
//   * THE ACTIVATIONS ARRIVE AS INT8.  The LayerNorm in front of ff.net.0.proj is not folded: layernorm_q8_kernel (norm.hip) writes
//     int8(norm3(x)) once, the tensor the reference calibrates and quantizes, and this kernel streams it.  No row statistics, no colsum,
//     no quantizer between two barriers (tile 19's cost: LAB_NOTES round 26) - the K loop holds LDS reads and MFMAs only.
//   * MFMA: v_mfma_i32_16x16x64_i8, ONE instruction per 16 x 16 block and K64 stage (tile 13: two K32 steps).  Operand / result layout:
//     bit 4 of sd_selftest_mfma; A and B share the lane -> k map, the result layout is tile 13's.
//   * WEIGHTS int8 in the order of smgeglu_i8_pack (weight_prep.h): 16-row strips, strip 2 U + v = the value (v = 0) / gate (v = 1) rows
//     of the output's 16-column unit U, so a tile's 160 rows are ten consecutive strips and a wave's strip pair is one unit.
//   * STAGE = K64, 18 KB (BM = 128) / 26 KB (BM = 256), half of tile 13's.  K64 and not K128 (two MFMA steps per barrier): the kernel
//     keeps tile 13's eligibility rule C % 64 == 0 with no tail stage, the ring gets twice the depth in stages for the same bytes in
//     flight, and a barrier still covers 8 / 16 MFMAs of 16 x 16 x 64 per wave - the MFMA time of a tile-13 K64 stage, whose barrier
//     count this kernel therefore shares.  Not measured against a K128 build.
//   * Q8OUT (a third and fourth instantiation; the two fp16 ones keep their text): behind sm_round4 and the exchange the lane holds the
//     eight fp16 values it would store; it quantizes exactly those with ws_quantize8(o8, inv_s_out) and stores 8 B of out_q [M][N / 2]
//     int8 instead - bit for bit the plain quantizer over what the fp16 launch stores, the tensor the reference calibrates for
//     ff.net.2, and the activations of plan tile 24 (smgemm_q8.hip) with no launch in between.
#include "conv_plan.h"
#include "igemm_device.h"
#include "kernels.h"
#include "quantize8.h"
#include "sm_i8_ring.h"
#include "weight_prep.h"

namespace sd {

namespace {

constexpr int SGG_UNITS = SM_I8_WROWS / 32;   // 16-column units side by side: 16 value + 16 gate rows each

struct SgI8Args {
  const int8_t* xq;     // [M][K]
  const int8_t* w;      // [N / 16 strips][16][K], smgeglu_i8_pack
  const float* cs;      // [N] s_a * s_w, rows interleaved 32 value / 32 gate (geglu_row)
  const float* bias;    // [N], the same order; has_bias == 0: any readable float[N] (the loads keep their count)
  half_t* out;          // [M][N / 2]
  int8_t* out_q;        // Q8OUT: [M][N / 2] int8 in place of out
  float inv_s_out;      // Q8OUT: 1 / s of the output's range
  int K, nk, ldo;
  int has_bias;
  SmTileOrder order;
};

// first row, in the upload's interleaved order, of 16-column unit U of the output: its 16 value rows; the gate rows are 32 further on
__device__ __forceinline__ int geglu_unit_row(int U) { return 64 * (U >> 1) + 16 * (U & 1); }

template <int BM, bool Q8OUT>
__global__ __launch_bounds__(64 * SM_I8_NW, 1) void smgeglu_i8_kernel(SgI8Args a) {
  using C = SmI8RingCfg<BM, 4>;   // EPI = 4: bias_v, bias_g, cs_v, cs_g below
  constexpr int NST = C::NST, PPW = C::PPW, TM = C::TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int u = wave % SGG_UNITS, h = wave / SGG_UNITS;   // column unit, row half

  int m_tile, n_tile;
  sm_tile_coords(a.order, m_tile, n_tile);
  const int m_blk = m_tile * BM, u_blk = n_tile * SGG_UNITS;   // first row, first 16-column unit of the tile

  // ---- staging: piece wave + 10 j of every stage (the last j only on the first FULL waves); lane = 4 row + position ----
  const bool full = wave < C::FULL;
  const int8_t* src[PPW];
  int pdst[PPW];
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    int p = wave + SM_I8_NW * j;
    if (p >= C::PIECES) p -= C::PIECES;                   // (never issued: keeps the address in range)
    pdst[j] = p * 1024;
    const int r = lane >> 2;
    const int chunk = sm_i8_swz(lane & 3, r);             // logical chunk at physical position lane & 3
    const int wp = SM_I8_WROWS / 16;                      // weight pieces: strips 2 u_blk .. 2 u_blk + 9
    src[j] = (p < wp ? a.w + ((size_t)(2 * u_blk + p) * 16 + r) * a.K : a.xq + (size_t)(m_blk + 16 * (p - wp) + r) * a.K) + chunk * 16;
  }
  const SmI8Ring<C> ring{smem, full, src, pdst};

#pragma unroll
  for (int p = 0; p < NST - 1; ++p)
    if (p < a.nk) ring.issue(p);
  // the epilogue operands right behind the first ring stages: bias and cs of this lane's four value and four gate rows (bias absent: a
  // readable dummy, so that every launch counts the same loads)
  const int g = lane >> 4, r16 = lane & 15;
  const int vrow = geglu_unit_row(u_blk + u) + 4 * g;
  __builtin_amdgcn_sched_barrier(0);
  const floatx4 bias_v = *reinterpret_cast<const floatx4*>(a.bias + vrow);
  const floatx4 bias_g = *reinterpret_cast<const floatx4*>(a.bias + vrow + 32);
  const floatx4 cs_v = *reinterpret_cast<const floatx4*>(a.cs + vrow);
  const floatx4 cs_g = *reinterpret_cast<const floatx4*>(a.cs + vrow + 32);
  __builtin_amdgcn_sched_barrier(0);

  // fragment offset inside a piece: row r16, logical chunk g
  const int foff = r16 * 64 + sm_i8_swz(g, r16) * 16;
  const int w_off = 2 * u * 1024;                                  // the unit's value strip; the gate strip is the next piece
  const int x_off = (SM_I8_WROWS / 16 + h * TM) * 1024;            // the half's first row block

  intx4 accv[TM], accg[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) accv[i] = accg[i] = intx4{0, 0, 0, 0};

  int slot = 0;   // slot of stage s
  for (int s = 0; s < a.nk; ++s) {
    ring.wait_stage(s, a.nk);
    if (s + NST - 1 < a.nk) ring.issue(slot == 0 ? NST - 1 : slot - 1);
    const char* st = smem + slot * C::STAGE;
    const intx4 wv = *reinterpret_cast<const intx4*>(st + w_off + foff);
    const intx4 wg = *reinterpret_cast<const intx4*>(st + w_off + 1024 + foff);
    intx4 xf[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) xf[i] = *reinterpret_cast<const intx4*>(st + x_off + i * 1024 + foff);
#pragma unroll
    for (int i = 0; i < TM; ++i) {   // rows = weight row, cols = m: lane holds columns 4 g + e of pixel r16
      accv[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wv, xf[i], accv[i], 0, 0, 0);
      accg[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wg, xf[i], accg[i], 0, 0, 0);
    }
    slot = slot + 1 == NST ? 0 : slot + 1;
  }

  // ---- epilogue: int32 -> fp32, scale and bias (sm_i8_affine), then tile 13's ending: v * gelu_erf(g) in fp32, one rounding to fp16,
  // blocks (2p, 2p + 1) paired by sm_pack16 -> 16 B of one output row per lane ----
  const bool has_bias = a.has_bias != 0;
  const int n = (u_blk + u) * 16 + 8 * (g >> 1);
#pragma unroll
  for (int p = 0; p < TM / 2; ++p) {
    uintx2 ho[2];   // block 2p | block 2p + 1: columns 4 g .. 4 g + 3 in fp16
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int i = 2 * p + b;
      floatx4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = sm_i8_affine(accv[i][e], cs_v[e], bias_v[e], has_bias);
        const float gt = sm_i8_affine(accg[i][e], cs_g[e], bias_g[e], has_bias);
        o[e] = v * gelu_erf(gt);
      }
      ho[b] = sm_round4(o);
    }
    const half8 o8 = sm_pack16(ho[0], ho[1]);
    const int m = m_blk + h * (BM / 2) + 32 * p + 16 * (g & 1) + r16;
    if constexpr (Q8OUT) out_store(reinterpret_cast<uintx2*>(a.out_q + (size_t)m * a.ldo + n), ws_quantize8(o8, a.inv_s_out));
    else out_store(reinterpret_cast<half8*>(a.out + (size_t)m * a.ldo + n), o8);
  }
}

}  // namespace

bool smgeglu_i8_shape_ok(const ConvDesc& d, int variant) { return smgeglu_shape_ok(d, variant) && !d.ln_colsum && !d.prof && d.C0 <= kSmI8MaxK; }

void launch_smgeglu_i8(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  const int bm = p.bm;
  SD_REQUIRE((bm == 128 || bm == 256) && smgeglu_i8_shape_ok(d, bm == 128 ? 1 : 2) && d.cw.kind == WeightSource::I8Geglu && d.cw.stream && d.cw.scale &&
                 d.x0_i8 && (!d.out_q8 || (d.out_inv_s > 0.f && std::isfinite(d.out_inv_s))),
             kInvalidArgument,
             "plan tile 20 (smgeglu_i8.hip, int8): not a 1x1 GEGLU projection it tiles, or no int8 weights / activations (C0=%d N=%d M=%d bm=%d)", d.C0,
             d.N, d.B * d.Ho * d.Wo, bm);
  const int M = d.B * d.Ho * d.Wo, K = d.C0;
  SgI8Args a;
  a.xq = d.x0_i8;
  a.w = d.cw.i8();
  a.cs = d.cw.scale;
  a.bias = d.bias ? d.bias : d.cw.scale;   // absent: the scales stand in, N floats (the loads keep their count)
  a.out = d.out;
  a.out_q = d.out_q8;
  a.inv_s_out = d.out_inv_s;
  a.K = K;
  a.nk = K / SM_I8_BK;
  a.ldo = d.N / 2;
  a.has_bias = d.bias != nullptr;
  a.order = sm_tile_order(M, d.N, K, M / bm, d.N / SM_I8_WROWS);   // tile 13's order, from the fp16 sizes
  const unsigned nwg = (unsigned)(M / bm) * (d.N / SM_I8_WROWS);
  conv_plan_log(d, p, a.order.n_fast);
  if (d.out_q8) {
    if (bm == 128) sm_i8_launch<smgeglu_i8_kernel<128, true>>(a, nwg, SM_I8_NW, SmI8RingGeom<128>::LDS, s);
    else sm_i8_launch<smgeglu_i8_kernel<256, true>>(a, nwg, SM_I8_NW, SmI8RingGeom<256>::LDS, s);
  } else if (bm == 128) sm_i8_launch<smgeglu_i8_kernel<128, false>>(a, nwg, SM_I8_NW, SmI8RingGeom<128>::LDS, s);
  else sm_i8_launch<smgeglu_i8_kernel<256, false>>(a, nwg, SM_I8_NW, SmI8RingGeom<256>::LDS, s);
  SD_HIP(hipGetLastError());
}

}  // namespace sd
