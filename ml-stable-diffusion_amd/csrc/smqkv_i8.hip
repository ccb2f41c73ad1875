// W8A8 form of the self-attention q|k|v projection (plan tile 22): smqkv_i8_kernel and its launcher.  The ring is the one of sm_i8_ring.h
// as plan tile 20 runs it, with one change of meaning: where tile 20's wave holds the value and the gate strip of ONE 16-column unit,
// this wave holds the strips of TWO plain 16-column units - a BM x 160-column tile, BM = 128 / 256, ten waves = 5 unit pairs x 2 row
// halves, one workgroup per tile in the XCD runs of sm_tile.h.
// The semantics are the int8 kernels' (sd_weights_quantize_w8a8 in sd_mi355x.h): exact int32 sums over the WHOLE K (kSmI8MaxK), one
// conversion to fp32, one product with cs[n] = fp32(s_a * s_w[n]), the bias added in fp32, the queries' q_scale - each operation
// rounded on its own, the fp32 value pinned in front of the one rounding to fp16 (qkv_value).
//
// WEIGHTS: the stacked matrix [Wq | Wk | Wv] (3C, C) int8 in the order of smqkv_i8_pack (weight_prep.h): 16-row strips in row order, so
// a tile reads the ten consecutive strips 10 n_tile .. 10 n_tile + 9.  C % 160 == 0 (smqkv_i8_shape_ok): a tile lies inside q, k or v,
// and which of them is a property of the WORKGROUP (n_tile), never of a lane.
//
// THE EPILOGUE leaves from the accumulators, no LDS, no barrier.  A and B of v_mfma_i32_16x16x64_i8 share the lane -> (row, k) map (bit 4
// of sd_selftest_mfma: A[i = l & 15][k = 16 (l >> 4) + e], B[k][j = l & 15], D lane l register r = D[i = 4 (l >> 4) + r][j = l & 15]), so
// the two operands may trade places, and the result then arrives transposed:
//   * q and k tiles: A = weights, B = activations (tile 20's order) - lane (g, r16) holds output columns 4 g + r of token r16;
//     sm_pack16 pairs two row blocks into 16 B of one out_qk row, as tile 20 stores.
//   * v tiles:       A = activations, B = weights - lane (g, r16) holds TOKENS 4 g + r of output column r16: four consecutive tokens of
//     one V^T row, one 8-byte store.  S % 16 == 0 (the shape rule) keeps a 16-token block inside one sample, and vt_perm - the two
//     middle 4-token blocks of every 16 tokens swapped (AttnDesc::vt_perm) - is a permutation of whole lane groups: g -> (0, 2, 1, 3)[g].
// The choice is one wave-uniform branch around two instances of the K loop.
#include <type_traits>

#include "conv_plan.h"
#include "igemm_device.h"
#include "kernels.h"
#include "quantize8.h"
#include "sm_i8_ring.h"
#include "weight_prep.h"

namespace sd {

namespace {

constexpr int SQV_PAIRS = SM_I8_WROWS / 32;   // pairs of 16-column units side by side
static_assert(kSmQkvCols == SM_I8_WROWS, "tile width of plan tile 22");

struct SqI8Args {
  const int8_t* xq;     // [M][K]
  const int8_t* w;      // [3C / 16 strips][16][K], smqkv_i8_pack
  const float* cs;      // [3C] s_a * s_w
  const float* bias;    // [3C]; has_bias == 0: any readable float[3C] (the loads keep their count)
  half_t* out_qk;       // [M][2C]
  half_t* out_vt;       // [B][C][ldT]
  int K, nk, C, S, ldT;
  int has_bias, vt_perm, q_mul;
  float q_scale;        // q_mul != 0: the q tiles' values are multiplied by it
  SmTileOrder order;
};

// one output value in fp32: every operation rounded on its own (no fma), and the result pinned in a register so that the last product
// and the rounding to fp16 that follows stay two instructions (hipcc otherwise fuses them into v_fma_mixlo_f16: ONE rounding)
__device__ __forceinline__ float qkv_value(int acc, float cs, float bias, bool has_bias, float q_scale, bool q_mul) {
#pragma clang fp contract(off)
  float v = sm_i8_affine(acc, cs, bias, has_bias);
  if (q_mul) v = v * q_scale;
  asm volatile("" : "+v"(v));
  return v;
}

template <int BM>
__global__ __launch_bounds__(64 * SM_I8_NW, 1) void smqkv_i8_kernel(SqI8Args a) {
  using C = SmI8RingCfg<BM, 4>;   // EPI = 4: bias0, bias1, cs0, cs1 below
  constexpr int NST = C::NST, PPW = C::PPW, TM = C::TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int u = wave % SQV_PAIRS, h = wave / SQV_PAIRS;   // unit pair, row half

  int m_tile, n_tile;
  sm_tile_coords(a.order, m_tile, n_tile);
  const int m_blk = m_tile * BM, n_blk = n_tile * kSmQkvCols;   // first row, first output column of the tile
  const bool is_v = n_blk >= 2 * a.C;                           // the whole tile: V^T columns
  const bool q_mul = a.q_mul != 0 && n_blk < a.C;               // the whole tile: queries

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
    const int wp = kSmQkvCols / 16;                       // weight pieces: strips 10 n_tile .. 10 n_tile + 9
    src[j] = (p < wp ? a.w + ((size_t)(n_blk + 16 * p) + r) * a.K : a.xq + (size_t)(m_blk + 16 * (p - wp) + r) * a.K) + chunk * 16;
  }
  const SmI8Ring<C> ring{smem, full, src, pdst};

#pragma unroll
  for (int p = 0; p < NST - 1; ++p)
    if (p < a.nk) ring.issue(p);
  // the epilogue operands right behind the first ring stages: bias and cs of the lane's columns in both units, four 16-B loads whatever
  // the tile (bias absent: a readable dummy, so that every launch counts the same loads).  q / k tiles: columns 4 g .. 4 g + 3 of a
  // unit; v tiles: column r16, element r16 & 3 of the aligned four that hold it.
  const int g = lane >> 4, r16 = lane & 15;
  const int n0 = n_blk + 32 * u + (is_v ? (r16 & ~3) : 4 * g);
  __builtin_amdgcn_sched_barrier(0);
  const floatx4 bias0 = *reinterpret_cast<const floatx4*>(a.bias + n0);
  const floatx4 bias1 = *reinterpret_cast<const floatx4*>(a.bias + n0 + 16);
  const floatx4 cs0 = *reinterpret_cast<const floatx4*>(a.cs + n0);
  const floatx4 cs1 = *reinterpret_cast<const floatx4*>(a.cs + n0 + 16);
  __builtin_amdgcn_sched_barrier(0);

  // fragment offset inside a piece: row r16, logical chunk g
  const int foff = r16 * 64 + sm_i8_swz(g, r16) * 16;
  const int w_off = 2 * u * 1024;                                  // the pair's first strip; the second is the next piece
  const int x_off = (kSmQkvCols / 16 + h * TM) * 1024;             // the half's first row block

  intx4 acc0[TM], acc1[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) acc0[i] = acc1[i] = intx4{0, 0, 0, 0};

  // the K loop; VT: the activations are operand A, the result holds tokens along the registers
  auto k_loop = [&](auto vt) __attribute__((always_inline)) {
    constexpr bool VT = decltype(vt)::value;
    int slot = 0;   // slot of stage s
    for (int s = 0; s < a.nk; ++s) {
      ring.wait_stage(s, a.nk);
      if (s + NST - 1 < a.nk) ring.issue(slot == 0 ? NST - 1 : slot - 1);
      const char* st = smem + slot * C::STAGE;
      const intx4 w0 = *reinterpret_cast<const intx4*>(st + w_off + foff);
      const intx4 w1 = *reinterpret_cast<const intx4*>(st + w_off + 1024 + foff);
      intx4 xf[TM];
#pragma unroll
      for (int i = 0; i < TM; ++i) xf[i] = *reinterpret_cast<const intx4*>(st + x_off + i * 1024 + foff);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        if constexpr (VT) {   // rows = token, cols = weight row: lane holds tokens 4 g + e of column r16
          acc0[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf[i], w0, acc0[i], 0, 0, 0);
          acc1[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xf[i], w1, acc1[i], 0, 0, 0);
        } else {              // rows = weight row, cols = token: lane holds columns 4 g + e of token r16
          acc0[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, xf[i], acc0[i], 0, 0, 0);
          acc1[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, xf[i], acc1[i], 0, 0, 0);
        }
      }
      slot = slot + 1 == NST ? 0 : slot + 1;
    }
  };
  if (is_v) k_loop(std::true_type{});
  else k_loop(std::false_type{});

  const bool has_bias = a.has_bias != 0;
  const int m_half = m_blk + h * (BM / 2);   // first row of this wave's half
  if (is_v) {
    // ---- V^T: column r16 of each unit, tokens 16 i + 4 g + (0 .. 3) -> 8 B at out_vt[b][n - 2C][s'], s' the token's place in the key
    // order (vt_perm: lane groups 1 and 2 trade places inside their 16 tokens) ----
    const int e4 = r16 & 3;
    const float c0 = cs0[e4], c1 = cs1[e4], b0 = bias0[e4], b1 = bias1[e4];
    const int pg = a.vt_perm ? ((0xd8 >> (2 * g)) & 3) : g;   // (0, 2, 1, 3)
    const int nv = n_blk - 2 * a.C + 32 * u + r16;            // V^T row of unit 0; unit 1: 16 further on
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m16 = m_half + 16 * i;                        // a 16-token block of one sample (S % 16 == 0)
      const int b = m16 / a.S, sp = m16 - b * a.S + 4 * pg;
      half4 o0, o1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o0[e] = (half_t)qkv_value(acc0[i][e], c0, b0, has_bias, 1.f, false);
        o1[e] = (half_t)qkv_value(acc1[i][e], c1, b1, has_bias, 1.f, false);
      }
      half_t* dst = a.out_vt + ((size_t)b * a.C + nv) * a.ldT + sp;
      *reinterpret_cast<half4*>(dst) = o0;
      *reinterpret_cast<half4*>(dst + (size_t)16 * a.ldT) = o1;
    }
  } else {
    // ---- q | k: blocks (2p, 2p + 1) paired by sm_pack16 -> 16 B of one out_qk row per lane and unit ----
    const int ldo = 2 * a.C;
#pragma unroll
    for (int p = 0; p < TM / 2; ++p) {
      const int m = m_half + 32 * p + 16 * (g & 1) + r16;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const floatx4 cs = j ? cs1 : cs0, bias = j ? bias1 : bias0;
        uintx2 ho[2];   // block 2p | block 2p + 1: columns 4 g .. 4 g + 3 in fp16
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const intx4 acc = j ? acc1[2 * p + b] : acc0[2 * p + b];
          floatx4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = qkv_value(acc[e], cs[e], bias[e], has_bias, a.q_scale, q_mul);
          ho[b] = sm_round4(o);
        }
        const half8 o8 = sm_pack16(ho[0], ho[1]);
        const int n = n_blk + 32 * u + 16 * j + 8 * (g >> 1);
        out_store(reinterpret_cast<half8*>(a.out_qk + (size_t)m * ldo + n), o8);
      }
    }
  }
}

}  // namespace

void launch_smqkv_i8(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  const int bm = p.bm;
  SD_REQUIRE((bm == 128 || bm == 256) && smqkv_i8_shape_ok(d, bm == 128 ? 1 : 2) && d.cw.kind == WeightSource::I8Qkv && d.cw.stream && d.cw.scale &&
                 d.x0_i8 && d.out && d.out_t,
             kInvalidArgument,
             "plan tile 22 (smqkv_i8.hip, int8): not a q|k|v projection it tiles, or no int8 weights / activations / outputs (C0=%d N=%d M=%d S=%d bm=%d)",
             d.C0, d.N, d.B * d.Ho * d.Wo, d.Ho * d.Wo, bm);
  const int M = d.B * d.Ho * d.Wo, K = d.C0;
  SqI8Args a;
  a.xq = d.x0_i8;
  a.w = d.cw.i8();
  a.cs = d.cw.scale;
  a.bias = d.bias ? d.bias : d.cw.scale;   // absent: the scales stand in, 3C floats (the loads keep their count)
  a.out_qk = d.out;
  a.out_vt = d.out_t;
  a.K = K;
  a.nk = K / SM_I8_BK;
  a.C = d.C0;
  a.S = d.Ho * d.Wo;
  a.ldT = d.ldT;
  a.has_bias = d.bias != nullptr;
  a.vt_perm = d.vt_perm ? 1 : 0;
  a.q_mul = d.q_cols > 0 ? 1 : 0;
  a.q_scale = d.q_scale;
  a.order = sm_tile_order(M, d.N, K, M / bm, d.N / kSmQkvCols);   // from the fp16 operand sizes, as tiles 13 / 20
  const unsigned nwg = (unsigned)(M / bm) * (d.N / kSmQkvCols);
  conv_plan_log(d, p, a.order.n_fast);
  if (bm == 128) sm_i8_launch<smqkv_i8_kernel<128>>(a, nwg, SM_I8_NW, SmI8RingGeom<128>::LDS, s);
  else sm_i8_launch<smqkv_i8_kernel<256>>(a, nwg, SM_I8_NW, SmI8RingGeom<256>::LDS, s);
  SD_HIP(hipGetLastError());
}

}  // namespace sd
