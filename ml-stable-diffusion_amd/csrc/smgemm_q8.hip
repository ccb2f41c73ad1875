// The small-M 1x1 GEMM from int8 weights and int8 ACTIVATIONS (plan tile 24): smgemm_q8_kernel and its launcher.  Geometry, tile order,
// eligibility and epilogue are tile 12 / 19's (smgemm.hip, smgemm_i8.hip) - five waves over a BM x 80 tile, BM = 32 / 64, wave w owns
// output columns 16 w .. 16 w + 15 of all BM rows, one workgroup per tile in the XCD runs of sm_tile.h, epilogue from the accumulators
// through sm_swap16 with no LDS and no barrier, smgemm_shape_ok with one source and K <= kSmI8MaxK.  The K loop is tile 20 / 22's kind
// (sm_i8_ring.h): every byte of a K64 stage arrives as a 16-row x 64-B LDS-DMA piece, one barrier per stage, and between two barriers
// stand LDS reads and MFMAs only.
// The semantics are tile 19's behind its quantizer: exact int32 sums over the WHOLE K (v_mfma_i32_16x16x64_i8, no split-K, no slab),
//     out = fp16(((float(acc) * cs[n]) + bias[n]) + float(res[m][n]))
// with every fp32 operation rounded on its own and ONE rounding to fp16 (gemm_value, sm_i8_ring.h).  Tile 24 on xq is therefore the same
// function as tile 19 on any x with ws_quantize8(x) == xq.
//
// What differs from tile 19, and why:
//   * THE ACTIVATIONS ARRIVE AS INT8 [M][K] (ConvDesc::x0_i8), written by their producer - the GEGLU epilogue of tile 20 with an int8
//     output, or a plain-form layernorm_q8 launch.  No fp16 staging part, no quantized image, no VALU between the barriers: tile 19's
//     quantizer between two barriers is what made it slower than its fp16 twin (LAB_NOTES round 26).
//   * A STAGE is [5 weight strips | BM / 16 activation strips], every strip one piece of sm_i8_ring.h (sm_i8_swz on the source address,
//     fragment read lane (g, r16) -> row r16, chunk g): 7 KB (BM = 32) / 9 KB (BM = 64).  The activation strips are shared by the five
//     waves - hence the barrier, which tile 19's wave-private ring did without - the weight strip of wave w is piece w.
//   * PIECES: wave + 5 j.  PPW = 2; the first FULL = 2 / 4 waves issue two pieces per stage (their weight strip and an activation
//     strip), the others their weight strip alone, and every wave counts its own vmcnt (SmI8Ring::wait_stage).
//   * RING: the whole LDS, 22 stages of 7 KB = 154 KB / 17 stages of 9 KB = 153 KB, one workgroup of five waves per CU: the shapes this
//     kernel is for have at most 256 tiles (smgemm_q8_wanted), one round of the chip, so a second resident workgroup would find no work
//     and the depth is what keeps a CU's share of HBM in flight.  vmcnt: 2 x 20 + 4 = 44 / 2 x 15 + 6 = 36 of 63.  Not measured
//     against a shallower ring at two workgroups per CU.
//   * WEIGHTS: tile 19's layout, int8 [N][K] as the checkpoint holds them (weight_prep.h smgemm_i8_pack).
//   * Bias, cs and the residual (in the accumulator layout, 8 B per lane and block) are requested right behind the first NST - 1 ring
//     stages and counted in the same vmcnt: EPI = 2 + BM / 16 loads per lane, as in tile 19.
// RAW, WAR and the counted wait of the K loop: sm_i8_ring.h, THE RING.
// NOT HERE: a second source, GEGLU, the LayerNorm fold, GroupNorm statistics, out modes other than the plain one - what sm_tiles refuses.
#include "conv_plan.h"
#include "kernels.h"
#include "sm_i8_ring.h"
#include "weight_prep.h"

namespace sd {

namespace {

constexpr int SMQ_BN = 80;              // output columns per workgroup
constexpr int SMQ_NW = SMQ_BN / 16;     // waves: one 16-column strip each

struct SmQ8Args {
  const int8_t* xq;     // [M][K]
  const int8_t* w;      // [N][K]
  const float* cs;      // [N] s_a * s_w[n]
  const float* bias;    // [N]; has_bias == 0: any readable float[N] (the loads keep their count)
  const half_t* res;    // [M][res_ld]; has_res == 0: any readable half[N] with res_ld = 0
  half_t* out;          // [M][N]
  int K, N, nk, res_ld;
  int has_bias, has_res;
  SmTileOrder order;
};

// the five-wave sibling of SmI8RingCfg: what SmI8Ring reads (NST, PPW, STAGE, EPI) and what the kernel and the host need beside it
template <int BM>
struct SmQ8Cfg {
  static constexpr int WP = SMQ_NW;                               // weight pieces per stage: one strip per wave
  static constexpr int TM = BM / 16;                              // activation pieces per stage = 16 x 16 accumulator blocks per wave
  static constexpr int PIECES = WP + TM;                          // pieces per stage: weights, then activations
  static constexpr int PPW = (PIECES + SMQ_NW - 1) / SMQ_NW;      // pieces per wave per stage: the first FULL waves; the others one less
  static constexpr int FULL = PIECES - SMQ_NW * (PPW - 1);
  static constexpr int STAGE = PIECES * 1024;
  static constexpr int NST = SM_I8_LDS / STAGE;                   // ring depth: 22 / 17
  static constexpr size_t LDS = (size_t)NST * STAGE;
  static constexpr int EPI = 2 + TM;                              // epilogue loads per lane: bias, cs, one residual quad per block
  static_assert(BM % 32 == 0 && PPW == 2 && FULL >= 1 && FULL <= SMQ_NW, "tile");
  static_assert(NST >= 3 && LDS <= SM_I8_LDS, "ring");
  static_assert(PPW * (NST - 2) + EPI <= 63, "vmcnt range");
};

template <int BM>
__global__ __launch_bounds__(64 * SMQ_NW, 1) void smgemm_q8_kernel(SmQ8Args a) {
  using C = SmQ8Cfg<BM>;
  constexpr int NST = C::NST, PPW = C::PPW, TM = C::TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

  int m_tile, n_tile;
  sm_tile_coords(a.order, m_tile, n_tile);
  const int m_blk = m_tile * BM, n_blk = n_tile * SMQ_BN;
  const int g = lane >> 4, r16 = lane & 15;

  // ---- staging: piece wave + 5 j of every stage (the last j only on the first FULL waves); lane = 4 row + position ----
  const bool full = wave < C::FULL;
  const int8_t* src[PPW];
  int pdst[PPW];
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    int p = wave + SMQ_NW * j;
    if (p >= C::PIECES) p -= C::PIECES;                   // (never issued: keeps the address in range)
    pdst[j] = p * 1024;
    const int r = lane >> 2;
    const int chunk = sm_i8_swz(lane & 3, r);             // logical chunk at physical position lane & 3
    src[j] = (p < C::WP ? a.w + (size_t)(n_blk + 16 * p + r) * a.K : a.xq + (size_t)(m_blk + 16 * (p - C::WP) + r) * a.K) + chunk * 16;
  }
  const SmI8Ring<C> ring{smem, full, src, pdst};

#pragma unroll
  for (int p = 0; p < NST - 1; ++p)
    if (p < a.nk) ring.issue(p);
  // the epilogue operands right behind the first ring stages, in the accumulator layout: bias and cs of this lane's four columns, the
  // residual quad of each block (has_res == 0: a readable dummy row, so that every launch counts the same loads)
  __builtin_amdgcn_sched_barrier(0);
  const int ncol = n_blk + 16 * wave + 4 * g;
  const floatx4 bias4 = *reinterpret_cast<const floatx4*>(a.bias + ncol);
  const floatx4 cs4 = *reinterpret_cast<const floatx4*>(a.cs + ncol);
  half4 resv[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) resv[i] = *reinterpret_cast<const half4*>(a.res + (size_t)(m_blk + 16 * i + r16) * a.res_ld + ncol);
  __builtin_amdgcn_sched_barrier(0);

  // fragment offset inside a piece: row r16, logical chunk g
  const int foff = r16 * 64 + sm_i8_swz(g, r16) * 16;
  const int w_off = wave * 1024;                                   // this wave's weight strip
  const int x_off = C::WP * 1024;                                  // the first row block

  intx4 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) acc[i] = intx4{0, 0, 0, 0};

  int slot = 0;   // slot of stage s
  for (int s = 0; s < a.nk; ++s) {
    ring.wait_stage(s, a.nk);
    if (s + NST - 1 < a.nk) ring.issue(slot == 0 ? NST - 1 : slot - 1);
    const char* st = smem + slot * C::STAGE;
    const intx4 wf = *reinterpret_cast<const intx4*>(st + w_off + foff);
    intx4 xf[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) xf[i] = *reinterpret_cast<const intx4*>(st + x_off + i * 1024 + foff);
#pragma unroll
    for (int i = 0; i < TM; ++i)   // rows = n, cols = m: lane holds n = 4 g + e of row m = r16 of block i
      acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, xf[i], acc[i], 0, 0, 0);
    slot = slot + 1 == NST ? 0 : slot + 1;
  }

  // ---- epilogue, tile 19's: one conversion, one product, bias and residual in fp32, ONE rounding; blocks (2p, 2p + 1) paired by
  // sm_pack16 -> 16 B of one output row per lane ----
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

bool smgemm_q8_shape_ok(const ConvDesc& d, int variant) { return smgemm_i8_shape_ok(d, variant); }

void launch_smgemm_q8(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  const int bm = p.bm;
  SD_REQUIRE((bm == 32 || bm == 64) && smgemm_q8_shape_ok(d, bm == 32 ? 1 : 2) && d.cw.kind == WeightSource::I8GemmQ && d.cw.stream && d.cw.scale && d.x0_i8,
             kInvalidArgument,
             "plan tile 24 (smgemm_q8.hip, int8): not a single-source 1x1 GEMM it tiles, or no int8 weights / activations (C0=%d C1=%d N=%d M=%d)",
             d.C0, d.x1 ? d.C1 : 0, d.N, d.B * d.Ho * d.Wo);
  const int M = d.B * d.Ho * d.Wo, K = d.C0;
  SmQ8Args a;
  a.xq = d.x0_i8;
  a.w = d.cw.i8();
  a.cs = d.cw.scale;
  a.bias = d.bias ? d.bias : d.cw.scale;                                   // absent: the scales stand in, N floats (the loads keep their count)
  a.res = d.res ? d.res : reinterpret_cast<const half_t*>(d.cw.scale);     // ... and N halves of them for a residual row
  a.out = d.out;
  a.K = K;
  a.N = d.N;
  a.nk = K / SM_I8_BK;
  a.res_ld = d.res ? d.N : 0;
  a.has_bias = d.bias != nullptr;
  a.has_res = d.res != nullptr;
  a.order = sm_tile_order(M, d.N, K, M / bm, d.N / SMQ_BN);   // tile 12's order, from the fp16 sizes
  conv_plan_log(d, p, a.order.n_fast);
  const unsigned nwg = 8 * a.order.per_xcd;   // one workgroup per tile: 8 XCD runs
  if (bm == 32) sm_i8_launch<smgemm_q8_kernel<32>>(a, nwg, SMQ_NW, SmQ8Cfg<32>::LDS, s);
  else sm_i8_launch<smgemm_q8_kernel<64>>(a, nwg, SMQ_NW, SmQ8Cfg<64>::LDS, s);
  SD_HIP(hipGetLastError());
}

}  // namespace sd
