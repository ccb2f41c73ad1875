// Small-M 1x1 GEMM (plan tile 12): the transformer projections of the 640- and 1280-channel levels
// (unet.py:533-551 proj_in / proj_out, :62-118 to_out, :594-617 ff.net.2; plain epilogue: bias, optional residual).
// One activation source, or two concatenated along K (the merged transformer tail [Wp W2 | Wp] [g | h2], wfold.hip): the weight
// rows run along the whole K, the activation pieces change their source at ring stage C0 / 64.
//
// At M <= 2048 these GEMMs are neither FLOP- nor byte-bound on igemm_kernel's 64 x 64 tile: 160 workgroups leave 96 CUs idle, the
// general im2col loader does integer divisions before its first DMA, a 3- / 4-stage ring keeps only 48-64 KB in flight per CU,
// and the epilogue round-trips the tile through LDS behind two barriers (LAB_NOTES.md round 5 ablations).
// This kernel is the same LDS-DMA ring, cut to that case:
//   * workgroup = five waves over a BM x 80 tile (wave w: output columns 16 w .. 16 w + 15 of all BM rows, v_mfma_f32_16x16x32_f16),
//     so M = 512 / N = 1280 (BM = 32) and M = 2048 / N = 640 (BM = 64) are 256 workgroups: one per CU;
//   * the whole LDS is the ring: 10 stages of K64 at BM = 32, 8 at BM = 64.  A stage is [80 weight rows | BM activation rows] of
//     128 B with the bank swizzle of igemm.hip on the source address; every wave issues the same number of 1-KiB pieces per
//     stage (the last pieces of a stage repeat activation rows into an unused slot) so that one counted vmcnt serves all waves;
//   * the prologue has no division and no load before the first DMA: the host passes the XCD run length and a multiply-high
//     reciprocal for the tile index; a stage's pieces are weight rows first;
//   * the epilogue operands (bias, residual rows in the store layout) are requested right behind the first NST - 1 ring stages and
//     counted in the same vmcnt;
//   * epilogue from the accumulators: fp16 pairs of two 16-row blocks meet through v_permlane16_swap, every lane stores 16 B of
//     one output row; no LDS, no barrier.
#include <algorithm>

#include "conv_plan.h"
#include "kernels.h"
#include "sm_ring.h"

namespace sd {

namespace {

constexpr int SM_BK = 64;              // K halves per ring stage (128-B rows)
constexpr int SM_BN = 80;              // output columns per workgroup
constexpr int SM_NW = SM_BN / 16;      // waves: one 16-column strip each
constexpr int SM_LDS = 160 * 1024;

struct SmArgs {
  const half_t* x;      // [M][ldx0]: K stages [0, nk0)
  const half_t* x1;     // [M][ldx1]: K stages [nk0, nk) (single source: nk0 == nk, never read)
  const half_t* w;      // [N][K]
  const float* bias;    // [N]; has_bias == 0: any readable float[N] (the loads keep their count)
  const half_t* res;    // [M][res_ld]; has_res == 0: any readable half[N] with res_ld = 0
  half_t* out;          // [M][N]
  int K, N, nk, res_ld;
  int nk0, ldx0, ldx1;
  int has_bias, has_res;
  unsigned per_xcd;     // workgroups of one XCD's contiguous tile run (grid % 8 == 0)
  unsigned fast_div;    // tiles along the fast dimension (>= 2)
  unsigned fast_magic;  // floor(2^32 / fast_div) + 1: mulhi(t, magic) == t / fast_div for t * fast_div < 2^32
  int n_fast;           // 1: consecutive tiles share an activation panel, 0: a weight panel (igemm_device.h IgemmArgs::n_fast)
};

template <int BM>
struct SmCfg {
  static constexpr int ROWS = SM_BN + BM;                      // staged rows per stage: weights, then activations
  static constexpr int PIECES = ROWS / 8;                      // 1-KiB LDS-DMA pieces (8 rows x 128 B) per stage
  static constexpr int PPW = (PIECES + SM_NW - 1) / SM_NW;     // pieces per wave per stage
  static constexpr int STAGE = SM_NW * PPW * 1024;             // bytes per stage
  static constexpr int NST = SM_LDS / STAGE;                   // ring depth
  static constexpr int TM = BM / 16;                           // 16 x 16 accumulator blocks per wave
  static constexpr int EPI = 1 + TM / 2;                       // epilogue loads per lane: bias, residual rows
  static_assert(BM % 32 == 0 && ROWS % 8 == 0, "tile");
  static_assert(NST >= 3 && NST * STAGE <= SM_LDS, "ring");
  static_assert(PPW * (NST - 2) + EPI <= 63, "vmcnt range");
};

template <int BM>
__global__ __launch_bounds__(64 * SM_NW, 1) void smgemm_kernel(SmArgs a) {
  using C = SmCfg<BM>;
  constexpr int NST = C::NST, PPW = C::PPW, TM = C::TM;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

  // XCD-aware tile order (block b runs on XCD b % 8): XCD x walks tiles [x * per_xcd, (x + 1) * per_xcd)
  const unsigned t = (blockIdx.x & 7u) * a.per_xcd + (blockIdx.x >> 3);
  const unsigned slow = __umulhi(t, a.fast_magic);
  const unsigned fast = t - slow * a.fast_div;
  const int m_blk = (int)(a.n_fast ? slow : fast) * BM;
  const int n_blk = (int)(a.n_fast ? fast : slow) * SM_BN;

  // ---- staging: piece wave + 5 j of every stage, one 16-B chunk of one staged row per lane ----
  const half_t* src[PPW];
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    const int r = (wave + SM_NW * j) * 8 + (lane >> 3);   // staged row
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);        // logical chunk at physical slot lane & 7
    int rx = r - SM_BN;
    if (rx >= BM) rx -= BM;                               // the padding pieces repeat activation rows
    src[j] = (r < SM_BN ? a.w + (size_t)(n_blk + r) * a.K : a.x + (size_t)(m_blk + rx) * a.ldx0) + chunk * 8;
  }
  // second source: the activation pieces (j >= SM_BN / 8 / SM_NW: the first 80 staged rows are weights, whole pieces of them)
  // restart on x1 when ring stage nk0 is issued - a wave-uniform compare per stage, vector work once per kernel
  static_assert(SM_BN % (8 * SM_NW) == 0, "a piece is all weights or all activations, by j alone");
  auto switch_source = [&]() {
#pragma unroll
    for (int j = SM_BN / (8 * SM_NW); j < PPW; ++j) {
      const int r = (wave + SM_NW * j) * 8 + (lane >> 3);
      const int chunk = (lane & 7) ^ ((r >> 1) & 7);
      int rx = r - SM_BN;
      if (rx >= BM) rx -= BM;
      src[j] = a.x1 + (size_t)(m_blk + rx) * a.ldx1 + chunk * 8;
    }
  };
  // ring stage idx (< nk) into slot idx % NST
  auto issue = [&](int idx) {
    char* st = smem + (idx % NST) * C::STAGE + wave * 1024;   // wave-uniform piece base (M0)
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src[j],
                                       (__attribute__((address_space(3))) void*)(st + j * SM_NW * 1024), 16, 0, 0);
      src[j] += SM_BK;
    }
  };

#pragma unroll
  for (int p = 0; p < NST - 1; ++p)
    if (p < a.nk) issue(p);
  // the epilogue operands right behind the first ring stages, in the store layout: the bias of this lane's four columns, the
  // residual rows it stores (has_res == 0: a readable dummy row, so that every wave counts the same loads)
  const int g = lane >> 4, r16 = lane & 15;
  __builtin_amdgcn_sched_barrier(0);
  const floatx4 bias4 = *reinterpret_cast<const floatx4*>(a.bias + n_blk + 16 * wave + 4 * g);
  half8 resv[TM / 2];
#pragma unroll
  for (int p = 0; p < TM / 2; ++p)
    resv[p] = *reinterpret_cast<const half8*>(a.res + (size_t)(m_blk + 32 * p + 16 * (g & 1) + r16) * a.res_ld + n_blk + 16 * wave +
                                              8 * (g >> 1));
  __builtin_amdgcn_sched_barrier(0);

  // fragment offsets inside a stage: row (16-row block base + r16), logical chunk 4 kk + g; every block base is a multiple of 16,
  // so the swizzle of the row is (r16 >> 1) & 7
  int foff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) foff[kk] = r16 * 128 + (((4 * kk + g) ^ ((r16 >> 1) & 7)) * 16);

  floatx4 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};

  for (int rel = 0; rel < a.nk; ++rel) {
    // stage rel has landed for this wave once only the newer ring stages - and, while rel is one of the first NST - 1, the
    // epilogue loads - are in flight; the barrier then says so for every wave, and that every wave is done reading the slot the
    // next issue overwrites
    const int ahead = min(NST - 2, a.nk - 1 - rel);
    if (rel <= NST - 2) sm_wait<PPW, C::EPI, NST - 2>(ahead);
    else sm_wait<PPW, 0, NST - 2>(ahead);
    const char* st = smem + (rel % NST) * C::STAGE;
    half8 wf[2], xf[2][TM];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      wf[kk] = *reinterpret_cast<const half8*>(st + 16 * wave * 128 + foff[kk]);
#pragma unroll
      for (int i = 0; i < TM; ++i) xf[kk][i] = *reinterpret_cast<const half8*>(st + (SM_BN + 16 * i) * 128 + foff[kk]);
    }
    __builtin_amdgcn_sched_barrier(0);   // reads first, then the next DMA, then the MFMAs
    if (rel + NST - 1 < a.nk) {
      if (rel + NST - 1 == a.nk0) switch_source();   // (nk0 >= NST: never in the prologue, smgemm_shape_ok)
      issue(rel + NST - 1);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < TM; ++i)   // rows = n, cols = m: lane holds n = 4 g + e of pixel m = r16
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[kk], xf[kk][i], acc[i], 0, 0, 0);
  }

  // ---- epilogue: bias in fp32, one rounding to fp16, blocks (2p, 2p + 1) paired by v_permlane16_swap -> 16 B per lane ----
  const floatx4 bv = a.has_bias ? bias4 : floatx4{0.f, 0.f, 0.f, 0.f};
  const int n = n_blk + 16 * wave + 8 * (g >> 1);
#pragma unroll
  for (int p = 0; p < TM / 2; ++p) {
    unsigned lo[2], hi[2];   // [block 2p | block 2p + 1] x {columns 4 g, 4 g + 1 | 4 g + 2, 4 g + 3}
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const floatx4 v = acc[2 * p + b];
      const half2v h01 = {(half_t)(v[0] + bv[0]), (half_t)(v[1] + bv[1])};
      const half2v h23 = {(half_t)(v[2] + bv[2]), (half_t)(v[3] + bv[3])};
      lo[b] = __builtin_bit_cast(unsigned, h01);
      hi[b] = __builtin_bit_cast(unsigned, h23);
    }
    // the odd 16-lane rows of block 2p trade with the even rows of block 2p + 1: afterwards lane (g, r16) holds columns
    // 8 (g >> 1) .. + 7 of row 16 (2p + (g & 1)) + r16, the first four in the `vdst` results
    const auto s0 = __builtin_amdgcn_permlane16_swap(lo[0], lo[1], false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap(hi[0], hi[1], false, false);
    const unsigned d0 = s0[0], d1 = s1[0], d2 = s0[1], d3 = s1[1];   // scalars first (igemm.hip xor32_sum)
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    half8 o = __builtin_bit_cast(half8, (u4){d0, d1, d2, d3});
    if (a.has_res) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)o[e] + (float)resv[p][e]);
    }
    const int m = m_blk + 32 * p + 16 * (g & 1) + r16;
    out_store(reinterpret_cast<half8*>(a.out + (size_t)m * a.N + n), o);
  }
}

int sm_nst(int bm) { return bm == 32 ? SmCfg<32>::NST : SmCfg<64>::NST; }

int sm_bm(const ConvDesc& d, int variant) {   // variant 1 / 2: BM = 32 / 64; 0: by M
  if (variant == 1) return 32;
  if (variant == 2) return 64;
  return (long)d.B * d.Ho * d.Wo <= 1024 ? 32 : 64;
}

}  // namespace

bool smgemm_shape_ok(const ConvDesc& d, int variant) {
  if (!(d.ksize == 1 && d.stride == 1 && d.up == 1 && d.out_mode == kOutHalf && !d.ln_colsum && !d.out_t && !d.temb &&
        d.q_cols == 0 && !d.gnf_partial && d.n_twins == 0 && !d.debug && variant >= 0 && variant <= 2))
    return false;
  const long M = (long)d.B * d.Ho * d.Wo;
  const int bm = sm_bm(d, variant);
  const long mt = M / bm, nt = d.N / SM_BN;
  // a second source starts on a stage boundary, behind the prologue's NST - 1 stages (the kernel switches inside the K loop only)
  if (d.x1 && !(d.C1 % SM_BK == 0 && d.C1 >= SM_BK && d.C0 / SM_BK >= sm_nst(bm))) return false;
  return d.C0 % SM_BK == 0 && d.C0 >= SM_BK && d.N % SM_BN == 0 && M % bm == 0 && mt >= 2 && nt >= 2 && (mt * nt) % 8 == 0 &&
         mt * nt <= 65535;
}

// the library's rule: the shapes whose grid fills the chip once (M <= 2048; larger M has enough tiles for igemm.hip's kernels).
// Launches that must also leave GroupNorm statistics of their output (d.gn_partial) stay on igemm_kernel's epilogue, and so do
// K > 2560: 80 serial K stages per workgroup lose to the 4-way split-K plan of 5120 -> 1280 at M = 512 (32.3 vs 28.3 us in sequence,
// profiles/r07_smgemm_op_ab.txt).  Two sources (the merged transformer tail): K = C0 + C1 <= 3200, the 32x32 level's 2560 + 640.
bool smgemm_wanted(const ConvDesc& d) {
  static const int k2_max = tune_env_int("SD_SMGEMM_K2_MAX", 3200);   // (with SD_TUNE: 6400 sends the 16x16 level's merged tail here, A/B)
  if (!smgemm_shape_ok(d, 0) || d.gn_partial || (d.x1 ? d.C0 + d.C1 > k2_max : d.C0 > 2560)) return false;
  const long M = (long)d.B * d.Ho * d.Wo;
  const long tiles = M / sm_bm(d, 0) * (d.N / SM_BN);
  return M >= 256 && M <= 2048 && tiles >= 192 && tiles <= 256;
}

void launch_smgemm(const ConvDesc& d, int variant, hipStream_t s) {
  SD_REQUIRE(smgemm_shape_ok(d, variant), kInvalidArgument, "plan tile 12 (smgemm.hip): not a 1x1 GEMM it tiles (C0=%d C1=%d N=%d)",
             d.C0, d.x1 ? d.C1 : 0, d.N);
  const int M = d.B * d.Ho * d.Wo, K = d.C0 + (d.x1 ? d.C1 : 0);
  const int bm = sm_bm(d, variant);
  const unsigned mt = M / bm, nt = d.N / SM_BN, nwg = mt * nt;
  SmArgs a;
  a.x = d.x0;
  a.x1 = d.x1 ? d.x1 : d.x0;
  a.ldx0 = d.C0;
  a.ldx1 = d.x1 ? d.C1 : d.C0;
  a.w = d.w;
  a.bias = d.bias ? d.bias : reinterpret_cast<const float*>(d.w);   // K >= 64: the weights hold more than N floats
  a.res = d.res ? d.res : d.w;
  a.out = d.out;
  a.K = K;
  a.N = d.N;
  a.nk = K / SM_BK;
  a.nk0 = d.C0 / SM_BK;
  a.res_ld = d.res ? d.N : 0;
  a.has_bias = d.bias != nullptr;
  a.has_res = d.res != nullptr;
  a.per_xcd = nwg / 8;
  // tile order by the bytes each pulls into the 8 XCD L2s: m fastest streams every weight panel once and the activations once per
  // XCD; n fastest the other way round (no A/B switch here)
  a.n_fast = choose_tile_order(2.0 * M * K, 2.0 * d.N * K, (double)mt, (double)nt, false);
  a.fast_div = a.n_fast ? nt : mt;
  a.fast_magic = (unsigned)((1ull << 32) / a.fast_div + 1);
  conv_plan_log(d, ConvPlan{12, variant, 1, false, 0}, bm, a.n_fast);
  if (bm == 32) {
    auto k = smgemm_kernel<32>;
    constexpr size_t lds = (size_t)SmCfg<32>::NST * SmCfg<32>::STAGE;
    static DynLdsOnce once;
    once.set(k, lds);
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * SM_NW), lds, s, a);
  } else {
    auto k = smgemm_kernel<64>;
    constexpr size_t lds = (size_t)SmCfg<64>::NST * SmCfg<64>::STAGE;
    static DynLdsOnce once;
    once.set(k, lds);
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * SM_NW), lds, s, a);
  }
  SD_HIP(hipGetLastError());
}

}  // namespace sd
