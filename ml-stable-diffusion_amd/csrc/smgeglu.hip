// GEGLU projection of the 640- and 1280-channel levels in one chip-filling round (plan tile 13): unet.py:609-617 ff.net.0.proj with
// or without the LayerNorm in front of it folded in (UNet::fold_layernorm), out[m][j] = v * gelu_erf(g).
//
// On igemm_kernel's 64 x 128 tile these launches are 640 / 1280 workgroups on 512 slots (1.25 / 2.5 rounds, each round paying the
// kernel's shell), every workgroup pulls (64 + 128) rows x K through LDS (43 FLOP per byte filled) and the ring is 2 stages deep.
// This kernel is smgemm.hip's whole-LDS ring cut to the GEGLU case:
//   * workgroup = BM rows x 80 output columns = 160 weight rows, BM = 128 (M = 512) / 256 (M = 2048): 256 workgroups, one per CU;
//   * the weights are read as uploaded (rows interleaved 32 value / 32 gate): a 16-column unit is 16 value rows + the 16 gate rows
//     32 further on, both as A operands of v_mfma_f32_16x16x32_f16, so value and gate of an output meet in one lane's accumulators;
//   * ten waves = 5 column units x 2 row halves (3, 3, 2, 2 per SIMD); per K64 stage a wave reads its unit's two weight fragments
//     and its BM / 32 row blocks, two K32 sub-steps each;
//   * ring stage = [160 weight rows, unit-major | BM activation rows] of 128 B: 36 KB x 4 stages / 52 KB x 3 stages, no padding.
//     36 / 52 1-KiB pieces do not divide by ten: the first 6 / 2 waves issue one piece more per stage than the others, and every
//     wave counts its own vmcnt (two instances of the wait ladder behind a wave-uniform branch);
//   * LayerNorm row statistics by fdot2 from the activation fragments, the row blocks of a half dealt out to four of its five
//     waves, exchanged once through LDS behind one barrier after the K loop;
//   * bias / colsum of the lane's columns requested right behind the first ring stages (same vmcnt); epilogue from the
//     accumulators with the arithmetic of igemm.hip tile_epilogue, fp16 pairs of two row blocks meet through v_permlane16_swap,
//     every lane stores 16 B of one output row.
// PROF instantiation (ConvDesc::prof): every wave leaves six shader-clock stamps (sd_op_geglu_ln prints the table).
// NBITS > 0 instantiations (plan tile 16, smgeglu_pal_kernel): the same launch from palettized weights - the comment above SgPalArgs.
#include <algorithm>
#include <type_traits>
#include <utility>

#include "conv_plan.h"
#include "kernels.h"
#include "pal_decode.h"
#include "sm_ring.h"
#include "sm_tile.h"
#include "weight_prep.h"

namespace sd {

namespace {

constexpr int SG_BK = 64;                  // K halves per ring stage (128-B rows)
constexpr int SG_UNITS = 5;                // 16-column units side by side
constexpr int SG_WROWS = 32 * SG_UNITS;    // weight rows per workgroup: 16 value + 16 gate rows per unit
constexpr int SG_BN = 16 * SG_UNITS;       // output columns per workgroup
constexpr int SG_NW = 2 * SG_UNITS;        // waves: unit x row half
constexpr int SG_LDS = 160 * 1024;
constexpr int SG_STAMPS = 8;               // long long slots per wave in ConvDesc::prof (six used)

struct SgArgs {
  const half_t* x;       // [M][K]
  const half_t* w;       // [N][K], rows interleaved 32 value / 32 gate
  const float* bias;     // [N]; has_bias == 0: any readable float[N] (the loads keep their count)
  const float* colsum;   // [N]; lnf == 0: any readable float[N]
  half_t* out;           // [M][N / 2]
  long long* prof;       // PROF: [workgroup][wave][SG_STAMPS]
  int K, nk, ldo;
  int has_bias, lnf;
  float ln_eps;
  SmTileOrder order;
};

template <int BM>
struct SgCfg {
  static constexpr int ROWS = SG_WROWS + BM;                   // staged rows per stage: weights, then activations
  static constexpr int PIECE0 = 0;                             // first staged piece that travels by LDS-DMA
  static constexpr int PIECES = ROWS / 8;                      // 1-KiB LDS-DMA pieces (8 rows x 128 B) per stage
  static constexpr int PPW = (PIECES + SG_NW - 1) / SG_NW;     // pieces per wave per stage: the first FULL waves; the others one less
  static constexpr int FULL = PIECES - SG_NW * (PPW - 1);
  static constexpr int STAGE = PIECES * 1024;                  // bytes per stage
  static constexpr int NST = (SG_LDS - BM * 8) / STAGE;        // ring depth; the row statistics (float2 per row) sit behind the ring
  static constexpr int TM = BM / 32;                           // 16-row blocks per wave (one row half)
  static constexpr int SB = TM / 4;                            // blocks whose statistics a wave of units 0-3 carries
  static constexpr int EPI = 4;                                // epilogue loads per lane: bias and colsum of value / gate rows
  static constexpr size_t LDS = (size_t)NST * STAGE + BM * 8;
  static constexpr int LUT = 0, GAMMA = 0, WORDS = 0, HQ = 1;  // (palettized kernel only)
  static_assert(BM % 128 == 0 && ROWS % 8 == 0 && PPW >= 2 && FULL >= 1 && FULL <= SG_NW, "tile");
  static_assert(NST >= 3 && LDS <= SG_LDS, "ring");
  static_assert(PPW * (NST - 2) + EPI <= 63, "vmcnt range");
};

// ---------------------------------------------------------------------------------------------------------------------
// The same launch from PALETTIZED weights (plan tile 16): smgeglu_pal_kernel<BM, NBITS>.  Tile, waves, MFMAs and their order per
// accumulator block (ascending K64 stage, then kk = 0, 1), tile order, row statistics and epilogue are one text, so the output is
// bit-identical to smgeglu_kernel on the folded fp16 weights.  Only the source of a stage's 160 weight rows changes:
//   * no fp16 weight exists in global memory.  The stream is smgemm_pal_pack's (weight_prep.h smgeglu_pal_pack: one 16-row strip
//     per wave, groups of 8 stages, NBITS 16-B words per lane and group).  The tile's 160 staged rows are ten strips; wave w decodes
//     strip w of stage rel + 1 beside the MFMAs of stage rel - per weight one field of its bit stream (pal_decode.h), one 2-byte
//     LDS read of the LUT and, with the LayerNorm fold, w' = (half)((float)lut_value * gamma[k]): one fp32 product, one
//     round-to-nearest-even, fold_layernorm_rows' expression - and writes its two 16-B chunks per row to `strip base + foff[kk]`
//     of the stage's slot, the address the MFMA loop reads.  Decode and product are paid once per workgroup, not once per row half;
//   * the slot of stage rel + 1 last held stage rel + 1 - NST, which every wave left before the barrier at the end of stage
//     rel - 1 (NST >= 2); the lgkmcnt(0) in front of the barrier at the end of stage rel publishes the writes;
//   * the ring's DMA pieces are the BM activation rows only: 16 pieces over ten waves, the first FULL = 6 waves issue two per stage,
//     the others one (the rule of the fp16 kernel with other numbers).  The stage layout is unchanged, 36 KB x NST = 3;
//   * index words, LUT and gamma arrive by LDS-DMA, counted by hand: the LUT (2 pieces of 256 B: waves 0, 1) and gamma (one 256-B
//     piece per K64 stage, piece p by wave p % 10; K <= kSgPalMaxK = 2560: 10 KB) once per workgroup in front of everything else, the
//     index words through a transit buffer per wave of HALF a group: HQ = max(1, NBITS / 2) words (stages 4 i .. 4 i + 3 begin on a
//     word boundary for every width but 1 bit, whose single word is brought for both halves).  From there a lane takes its 16 B
//     per word into registers when stage 4 i is the next to decode.  LDS: 108 KB ring + 1 KB statistics + 0.5 KB LUT + 10 KB gamma
//     + 10 HQ KB transit = 159.5 KB at 8 bits;
//   * BM = 256 is not built: its stage is 52 KB, and the ring of three the K loop's pipelining and wait ladder are written for
//     (SgCfg: NST >= 3) leaves 2 KB of the 160 beside the statistics, against 10.5 KB of LUT and gamma and up to 40 KB of transit.
//     Those launches (640 -> 5120 at M = 2048) stay on fp16; plan tile 16 refuses bm = 256.
// Order of a wave's LDS-DMA pieces (they retire in order; the only ordinary loads, bias and colsum, come first and are used behind the
// loop), P = 2 (wave < FULL) or 1 activation pieces per stage:
//     [LUT] [gamma] [H_0] [stages 0 .. min(NST - 1, nk) - 1]      -> wait A: vmcnt(P min(NST - 1, nk)) + barrier: LUT, gamma, H_0
//     H_0 -> registers, stage 0 decoded into slot 0, lgkmcnt(0)   -> wait for stage 0 (+ barrier)
//     [H_1, if nk > 1] [stage NST - 1, if < nk]
//     end of stage rel (rel + 1 < nk): lgkmcnt(0), wait for stage rel + 1 (+ barrier), [H_((rel + 1) / 4 + 1), if 4 | rel + 1]
//                                      [stage rel + NST, if < nk]
// (H_i: the words of half-group min(i, last)).  H_(j+1) is issued at the end of stage 4 j - 1 (j = 0: behind the wait for stage 0) in
// front of stage 4 j - 1 + NST and moves to registers at the top of stage 4 j + 3, behind the wait for stage 4 j + 3 > 4 j + 2, which
// is younger; the transit buffer is free again behind the lgkmcnt(0) at the end of that stage.  Younger than stage s at its wait
// are the `ahead` = min(NST - 2, nk - 1 - s) stages behind it and batch H_(j+1) when 4 j < s < 4 j - 1 + NST:
//     vmcnt immediate = P * ahead + HQ * [s % 4 in 1 .. NST - 2]        (NST = 3: s % 4 == 1)
// tests/test_palettize_geglu.py replays this order for every K / 64 from 1 to 44 and finds each immediate equal to the count.
constexpr int kSgPalMaxK = 2560;

struct SgPalArgs : SgArgs {   // (w unused)
  const uint8_t* pal;    // [N / 16 strips][groups][NBITS][64 lanes][16 B], strips in the order of smgeglu_pal_pack
  const half_t* lut;     // kPalLutHalves entries
  const float* gamma;    // [K] fp32 LayerNorm weight; lnf == 0: not read
  int nhalf;             // half-groups of a strip's stream: 2 * groups
};
template <int BM, int NBITS>
struct SgPalCfg {
  static constexpr int ROWS = SG_WROWS + BM;                   // the stage layout of SgCfg; the weight rows are written by the waves
  static constexpr int PIECE0 = SG_WROWS / 8;
  static constexpr int PIECES = BM / 8;
  static constexpr int PPW = (PIECES + SG_NW - 1) / SG_NW;
  static constexpr int FULL = PIECES - SG_NW * (PPW - 1);
  static constexpr int STAGE = ROWS / 8 * 1024;
  static constexpr int NST = 3;
  static constexpr int TM = BM / 32;
  static constexpr int SB = TM / 4;
  static constexpr int HQ = NBITS >= 2 ? NBITS / 2 : 1;        // index words per half-group of 4 stages
  static constexpr int EPI = 0;                                // (the epilogue loads come first: no wait counts them)
  static constexpr int STAT = NST * STAGE;                     // byte offsets behind the ring
  static constexpr int LUT = STAT + BM * 8;
  static constexpr int GAMMA = LUT + kPalLutHalves * 2;
  static constexpr int WORDS = GAMMA + kSgPalMaxK * 4;
  static constexpr size_t LDS = (size_t)WORDS + SG_NW * HQ * 1024;
  static_assert(BM == 128 && PPW == 2 && FULL >= 1 && FULL <= SG_NW, "tile");
  static_assert(LDS <= SG_LDS, "ring");
  static_assert(PPW * (NST - 1) + HQ <= 63, "vmcnt range");
};

template <int... I, typename F>
__device__ __forceinline__ void sg_static_for(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}

__device__ __forceinline__ float sg_gelu_erf(float x) {   // igemm.hip gelu_erf (Abramowitz-Stegun 7.1.26)
  const float z = x * 0.70710678118654752f;
  const float az = fabsf(z);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.0f));
  float p = 1.061405429f;
  p = fmaf(p, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(-az * az * 1.4426950408889634f);
  const float erf_abs = fmaf(-p * t, e, 1.0f);
  return 0.5f * x * (1.0f + copysignf(erf_abs, z));
}

// first weight row of 16-column unit U of the output: its 16 value rows; the gate rows are 32 further on
__device__ __forceinline__ int sg_unit_row(int U) { return 64 * (U >> 1) + 16 * (U & 1); }

// One body for both launches: NBITS == 0 is the fp16 kernel (weights by LDS-DMA), NBITS > 0 the palettized one (smgeglu_pal_kernel).
template <int BM, bool PROF, int NBITS = 0>
__global__ __launch_bounds__(64 * SG_NW, 1) void smgeglu_kernel(std::conditional_t<(NBITS > 0), SgPalArgs, SgArgs> a) {
  constexpr bool PAL = NBITS > 0;
  using C = std::conditional_t<PAL, SgPalCfg<BM, PAL ? NBITS : 1>, SgCfg<BM>>;
  constexpr int NST = C::NST, PPW = C::PPW, TM = C::TM, SB = C::SB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  long long stamp[6] = {};
  if constexpr (PROF) stamp[0] = clock64();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int u = wave % SG_UNITS, h = wave / SG_UNITS;   // column unit, row half

  int m_tile, n_tile;
  sm_tile_coords(a.order, m_tile, n_tile);
  const int m_blk = m_tile * BM, u_blk = n_tile * SG_UNITS;   // first row, first 16-column unit of the tile

  // ---- staging: piece wave + 10 j of every stage (the last j only on the first FULL waves), one 16-B chunk of one staged row per
  // lane.  Staged weight row r: unit r / 32, value (r & 16 == 0) or gate row r & 15 ----
  const bool full = wave < C::FULL;
  const half_t* src[PPW];
  int pdst[PPW];
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    int p = wave + SG_NW * j;
    if (p >= C::PIECES) p -= C::PIECES;                   // (never issued: keeps the address in range)
    if constexpr (PAL) p += C::PIECE0;                    // (the activation pieces only)
    pdst[j] = p * 1024;
    const int r = p * 8 + (lane >> 3);                    // staged row
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);        // logical chunk at physical slot lane & 7
    const int wrow = sg_unit_row(u_blk + (r >> 5)) + 2 * (r & 16) + (r & 15);
    src[j] = (r < SG_WROWS ? a.w + (size_t)wrow * a.K : a.x + (size_t)(m_blk + r - SG_WROWS) * a.K) + chunk * 8;
  }
  // ring stage into slot `slot`
  auto issue = [&](int slot) {
    char* st = smem + slot * C::STAGE;
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      if (j == PPW - 1 && !full) break;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src[j],
                                       (__attribute__((address_space(3))) void*)(st + pdst[j]), 16, 0, 0);
      src[j] += SG_BK;
    }
  };

  // fp16: the epilogue operands right behind the first ring stages: bias and colsum of this lane's four value and four gate rows
  // (absent: a readable dummy, so that every launch counts the same loads).  Palettized: in front of every LDS-DMA piece, so that
  // no wait of the K loop counts them
  if constexpr (!PAL) {
#pragma unroll
    for (int p = 0; p < NST - 1; ++p)
      if (p < a.nk) issue(p);
  }
  const int g = lane >> 4, r16 = lane & 15;
  const int vrow = sg_unit_row(u_blk + u) + 4 * g;
  __builtin_amdgcn_sched_barrier(0);
  const floatx4 bias_v = *reinterpret_cast<const floatx4*>(a.bias + vrow);
  const floatx4 bias_g = *reinterpret_cast<const floatx4*>(a.bias + vrow + 32);
  const floatx4 cs_v = *reinterpret_cast<const floatx4*>(a.colsum + vrow);
  const floatx4 cs_g = *reinterpret_cast<const floatx4*>(a.colsum + vrow + 32);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (PROF) stamp[1] = clock64();

  // ---- palettized: LUT and gamma for the workgroup, this wave's index words (header comment) ----
  const unsigned short* const lutp = reinterpret_cast<const unsigned short*>(smem + (PAL ? C::LUT : 0));
  const float* const gam = reinterpret_cast<const float*>(smem + (PAL ? C::GAMMA : 0));
  char* const wbuf = smem + (PAL ? C::WORDS + wave * (C::HQ * 1024) : 0);
  // half-group min(i, last) into the transit buffer
  auto issue_half = [&](int i) __attribute__((always_inline)) {
    if constexpr (PAL) {
      i = min(i, a.nhalf - 1);
      const uintx4* p = reinterpret_cast<const uintx4*>(a.pal) + ((size_t)(2 * u_blk + wave) * (a.nhalf >> 1) + (i >> 1)) * (NBITS * 64) +
                        (NBITS >= 2 ? (i & 1) * (C::HQ * 64) : 0) + lane;
#pragma unroll
      for (int q = 0; q < C::HQ; ++q)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p + q * 64),
                                         (__attribute__((address_space(3))) void*)(wbuf + q * 1024), 16, 0, 0);
    }
  };
  if constexpr (PAL) {
    if (wave < 2)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.lut + wave * 128 + lane * 2),
                                       (__attribute__((address_space(3))) void*)(smem + C::LUT + wave * 256), 4, 0, 0);
    if (a.lnf) {
      for (int p = wave; p < a.nk; p += SG_NW)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.gamma + p * SG_BK + lane),
                                         (__attribute__((address_space(3))) void*)(smem + C::GAMMA + p * (SG_BK * 4)), 4, 0, 0);
    }
    issue_half(0);
#pragma unroll
    for (int p = 0; p < NST - 1; ++p)
      if (p < a.nk) issue(p);
    __builtin_amdgcn_sched_barrier(0);
  }

  // fragment offsets inside a stage: row (16-row block base + r16), logical chunk 4 kk + g; every block base is a multiple of 16,
  // so the swizzle of the row is (r16 >> 1) & 7
  int foff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) foff[kk] = r16 * 128 + (((4 * kk + g) ^ ((r16 >> 1) & 7)) * 16);
  const int w_off = 32 * u * 128;                                   // the unit's value rows; gate rows 16 further on
  const int x_off = (SG_WROWS + h * (BM / 2)) * 128;                // the half's first row block

  floatx4 accv[TM], accg[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) accv[i] = accg[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  float ln_s1[SB], ln_s2[SB];   // sum x, sum x^2 over this lane's K chunks of row r16 of blocks u * SB .. (units 0-3)
#pragma unroll
  for (int s = 0; s < SB; ++s) ln_s1[s] = ln_s2[s] = 0.f;
  const half2v one2 = {(half_t)1.f, (half_t)1.f};

  // The K loop runs on the stage in quarters q = (sub-step kk = q / NG, row blocks 4 (q % NG) .. + 3), software-pipelined across
  // the stage boundary: while the MFMAs of one quarter run, the fragments of the next are on their way from LDS - the next
  // stage's weight fragments and first quarter during the last quarter of this one, so a wave never holds more than two
  // quarters of fragments beside its 2 TM accumulators (all of a 256-row stage's would not fit in 168 VGPRs).  Against reading a
  // whole stage behind the barrier and then running its MFMAs this measured no gain at BM = 128 (LAB_NOTES Finding 22).
  constexpr int NG = TM / 4, NQ = 2 * NG;
  half8 wv[2], wg[2], wvn[2], wgn[2], xq[2][4];
  auto read_w = [&](const char* st, half8 (&v)[2], half8 (&gt)[2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      v[kk] = *reinterpret_cast<const half8*>(st + w_off + foff[kk]);
      gt[kk] = *reinterpret_cast<const half8*>(st + w_off + 16 * 128 + foff[kk]);
    }
  };
  auto read_q = [&](const char* st, int q) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      xq[q & 1][i] = *reinterpret_cast<const half8*>(st + x_off + 16 * (4 * (q % NG) + i) * 128 + foff[q / NG]);
  };
  // stage s has landed for this wave once only the newer ring stages - and, while s is one of the first NST - 1, the epilogue
  // loads - are in flight; the barrier then says so for every wave
  auto wait_stage = [&](int s) {
    const int ahead = min(NST - 2, a.nk - 1 - s);
    if constexpr (PAL) {   // no epilogue loads to count; the index batch issued behind the wait for stage s - 1 when s % 4 == 1
      static_assert(!PAL || NST == 3, "the batch is younger than stages 4 j + 1 .. 4 j + NST - 2");
      if (full) {
        if ((s & 3) == 1) sm_wait<PPW, C::HQ, NST - 2>(ahead);
        else sm_wait<PPW, 0, NST - 2>(ahead);
      } else {
        if ((s & 3) == 1) sm_wait<PPW - 1, C::HQ, NST - 2>(ahead);
        else sm_wait<PPW - 1, 0, NST - 2>(ahead);
      }
      return;
    }
    if (full) {
      if (s <= NST - 2) sm_wait<PPW, C::EPI, NST - 2>(ahead);
      else sm_wait<PPW, 0, NST - 2>(ahead);
    } else {
      if (s <= NST - 2) sm_wait<PPW - 1, C::EPI, NST - 2>(ahead);
      else sm_wait<PPW - 1, 0, NST - 2>(ahead);
    }
  };

  // ---- palettized: the current half-group's words, and stage s's strip of this wave decoded into its slot ----
  uintx4 cur[PAL ? C::HQ : 1];
  auto read_words = [&]() __attribute__((always_inline)) {
    if constexpr (PAL) {
#pragma unroll
      for (int q = 0; q < C::HQ; ++q) cur[q] = *reinterpret_cast<const uintx4*>(wbuf + q * 1024 + lane * 16);
    }
  };
  auto decode_stage = [&](int s, char* st) __attribute__((always_inline)) {
    if constexpr (PAL) {
      char* const strip = st + 16 * wave * 128;   // staged strip `wave`: unit wave / 2, value or gate rows
      const float* const gs = gam + s * SG_BK + 8 * g;
      // the stage's place in the words held: a compile-time fragment number per case (no variable shift in pal_decode)
      sg_static_for(std::make_integer_sequence<int, 8>{}, [&](auto tc) __attribute__((always_inline)) {
        constexpr int T = decltype(tc)::value;
        if ((s & 7) == T) {
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            half8 f = pal_decode<NBITS>(cur, (NBITS >= 2 ? 2 * (T & 3) : 2 * T) + kk, lutp);
            if (a.lnf) {
              const floatx4 g0 = *reinterpret_cast<const floatx4*>(gs + 32 * kk);
              const floatx4 g1 = *reinterpret_cast<const floatx4*>(gs + 32 * kk + 4);
#pragma unroll
              for (int e = 0; e < 8; ++e) f[e] = (half_t)((float)f[e] * (e < 4 ? g0[e & 3] : g1[e & 3]));
            }
            *reinterpret_cast<half8*>(strip + foff[kk]) = f;
          }
        }
      });
    }
  };
  if constexpr (PAL) {
    // wait A: LUT, gamma and H_0 are older than the stages issued; the barrier publishes the workgroup's LUT and gamma
    if (full) sm_wait<PPW, 0, NST - 1>(min(NST - 1, a.nk));
    else sm_wait<PPW - 1, 0, NST - 1>(min(NST - 1, a.nk));
    read_words();
    decode_stage(0, smem);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  wait_stage(0);
  if constexpr (PROF) stamp[2] = clock64();
  if constexpr (PAL) {
    if (a.nk > 1) issue_half(1);
  }
  if (NST - 1 < a.nk) issue(NST - 1);
  read_w(smem, wv, wg);
  read_q(smem, 0);
  __builtin_amdgcn_sched_barrier(0);
  int slot = 0;   // slot of stage rel
  for (int rel = 0; rel < a.nk; ++rel) {
    const char* st = smem + slot * C::STAGE;
    const int nslot = slot + 1 == NST ? 0 : slot + 1;
    if constexpr (PAL) {
      if (rel + 1 < a.nk) {   // the next stage's weight rows; its half-group has landed (header comment)
        if (((rel + 1) & 3) == 0) read_words();
        decode_stage(rel + 1, smem + nslot * C::STAGE);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int kk = q / NG;
      const bool next_stage = q + 1 == NQ && rel + 1 < a.nk;
      if (next_stage) {
        // every read of stage rel is back (this wave), the next stage has landed, and behind the barrier both hold for every
        // wave: stage rel + NST may overwrite this stage's slot
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wait_stage(rel + 1);
        if constexpr (PAL) {
          if (((rel + 1) & 3) == 0) issue_half(((rel + 1) >> 2) + 1);
        }
        if (rel + NST < a.nk) issue(slot);
      }
      // the quarter's first MFMA, then the next quarter's reads, then the rest: hipcc waits for ALL outstanding LDS reads in front
      // of the first MFMA that needs one (lgkmcnt(0), not a counted wait), so the new reads must not be among them
      __builtin_amdgcn_sched_barrier(0);
      accv[4 * (q % NG)] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[kk], xq[q & 1][0], accv[4 * (q % NG)], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (q + 1 < NQ) {
        read_q(st, q + 1);
      } else if (next_stage) {
        read_w(smem + nslot * C::STAGE, wvn, wgn);
        read_q(smem + nslot * C::STAGE, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {   // rows = weight row, cols = m: lane holds columns 4 g + e of pixel r16
        const int blk = 4 * (q % NG) + i;
        if (i > 0) accv[blk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[kk], xq[q & 1][i], accv[blk], 0, 0, 0);
        accg[blk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wg[kk], xq[q & 1][i], accg[blk], 0, 0, 0);
      }
      if (a.lnf) {   // VALU work between the MFMAs; row block blk belongs to the wave of unit blk / SB
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int blk = 4 * (q % NG) + i;
          if (blk / SB == u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const half2v p2 = {xq[q & 1][i][2 * e], xq[q & 1][i][2 * e + 1]};
              ln_s2[blk % SB] = __builtin_amdgcn_fdot2(p2, p2, ln_s2[blk % SB], false);
              ln_s1[blk % SB] = __builtin_amdgcn_fdot2(p2, one2, ln_s1[blk % SB], false);
            }
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);   // keeps the later quarters' reads from being hoisted over this one
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) wv[kk] = wvn[kk], wg[kk] = wgn[kk];
    slot = nslot;
  }
  if constexpr (PROF) stamp[3] = clock64();
  if constexpr (PAL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a last index batch may still be on its way to the LDS

  // ---- row statistics: the four K-chunk groups of a row meet by lane shuffles, (ln_a, ln_b) of the tile's rows through LDS ----
  float ln_a[TM], ln_b[TM];
  if (a.lnf) {
    float2* stat = reinterpret_cast<float2*>(smem + NST * C::STAGE);   // [BM], behind the ring
    const float inv_k = 1.0f / (float)a.K;
#pragma unroll
    for (int s = 0; s < SB; ++s) {
      float s1 = ln_s1[s], s2 = ln_s2[s];
      s1 += __shfl_xor(s1, 16);
      s2 += __shfl_xor(s2, 16);
      s1 += __shfl_xor(s1, 32);
      s2 += __shfl_xor(s2, 32);
      const float mean = s1 * inv_k;
      const float var = fmaxf(s2 * inv_k - mean * mean, 0.f);
      const float la = rsqrtf(var + a.ln_eps);
      if (u < 4 && g == 0) stat[h * (BM / 2) + 16 * (u * SB + s) + r16] = make_float2(la, -la * mean);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float2 ab = stat[h * (BM / 2) + 16 * i + r16];
      ln_a[i] = ab.x;
      ln_b[i] = ab.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i) ln_a[i] = 1.f, ln_b[i] = 0.f;
  }
  if constexpr (PROF) stamp[4] = clock64();

  // ---- epilogue: tile_epilogue's arithmetic in fp32, one rounding to fp16, blocks (2p, 2p + 1) paired by sm_pack16 ----
  const floatx4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const floatx4 bv = a.has_bias ? bias_v : zero4, bg = a.has_bias ? bias_g : zero4;
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
        float v, gt;
        if (a.lnf) {
          v = fmaf(accv[i][e], ln_a[i], fmaf(ln_b[i], cs_v[e], bv[e]));
          gt = fmaf(accg[i][e], ln_a[i], fmaf(ln_b[i], cs_g[e], bg[e]));
        } else {
          v = accv[i][e] + bv[e];
          gt = accg[i][e] + bg[e];
        }
        o[e] = v * sg_gelu_erf(gt);
      }
      ho[b] = sm_round4(o);
    }
    const half8 o8 = sm_pack16(ho[0], ho[1]);
    const int m = m_blk + h * (BM / 2) + 32 * p + 16 * (g & 1) + r16;
    out_store(reinterpret_cast<half8*>(a.out + (size_t)m * a.ldo + n), o8);
  }
  if constexpr (PROF) {
    stamp[5] = clock64();
    if (lane == 0) {
      long long* dst = a.prof + ((size_t)blockIdx.x * SG_NW + wave) * SG_STAMPS;
#pragma unroll
      for (int k = 0; k < 6; ++k) dst[k] = stamp[k];
    }
  }
}

template <int BM, int NBITS>
constexpr auto smgeglu_pal_kernel = smgeglu_kernel<BM, false, NBITS>;

// variant 1 / 2: BM = 128 / 256; 0: the smaller tile height whose grid is at most one round of 256 CUs
int sg_bm(const ConvDesc& d, int variant) {
  if (variant == 1) return 128;
  if (variant == 2) return 256;
  const long M = (long)d.B * d.Ho * d.Wo;
  return M % 128 == 0 && M / 128 * (d.N / SG_WROWS) <= 256 ? 128 : 256;
}

template <int BM, bool PROF>
void sg_launch(const SgArgs& a, unsigned nwg, hipStream_t s) {
  auto k = smgeglu_kernel<BM, PROF>;
  static DynLdsOnce once;
  once.set(k, SgCfg<BM>::LDS);
  hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * SG_NW), SgCfg<BM>::LDS, s, a);
}

// a GEGLU projection the kernel tiles with bm-row tiles
bool sg_tiles(const ConvDesc& d, int bm) {
  if (!(d.ksize == 1 && d.stride == 1 && d.up == 1 && !d.x1 && d.out_mode == kOutGeglu && !d.out_t && !d.temb && !d.res &&
        d.q_cols == 0 && !d.gnf_partial && !d.gn_partial && d.n_twins == 0 && !d.debug && (!d.ln_colsum || d.bias) && (bm == 128 || bm == 256)))
    return false;
  const long M = (long)d.B * d.Ho * d.Wo;
  const long mt = M / bm, nt = d.N / SG_WROWS;
  return d.C0 % SG_BK == 0 && d.C0 >= SG_BK && d.N % SG_WROWS == 0 && d.N % 64 == 0 && M % bm == 0 && mt >= 2 && nt >= 2 &&
         (mt * nt) % 8 == 0 && mt * nt <= 65535;
}

}  // namespace

int smgeglu_bm(const ConvDesc& d, int variant) { return sg_bm(d, variant); }

size_t smgeglu_prof_entries(const ConvDesc& d, int variant) {
  const long M = (long)d.B * d.Ho * d.Wo;
  return (size_t)(M / sg_bm(d, variant) * (d.N / SG_WROWS)) * SG_NW * SG_STAMPS;
}

bool smgeglu_shape_ok(const ConvDesc& d, int variant) { return variant >= 0 && variant <= 2 && sg_tiles(d, sg_bm(d, variant)); }

// the library's rule: GEGLU projections whose grid of BM x 80 tiles fills the chip once (192-256 workgroups): SD2.1's 1280 -> 10240
// at M = 512 and 640 -> 5120 at M = 2048.  Everything else - the M = 128 level (64 tiles), the 64 x 64 level (wsgemm.hip), SDXL's and
// the refiner's widths, batched prompts (more than one round) - keeps its measured plan.
bool smgeglu_wanted(const ConvDesc& d) {
  if (!smgeglu_shape_ok(d, 0)) return false;
  const long M = (long)d.B * d.Ho * d.Wo;
  const long tiles = M / sg_bm(d, 0) * (d.N / SG_WROWS);
  return tiles >= 192 && tiles <= 256;
}

namespace {

// the launch arguments both kernels share; `dummy`: readable memory of at least N floats that stands in for an absent bias / colsum
SgArgs sg_common_args(const ConvDesc& d, int bm, const void* dummy) {
  const int M = d.B * d.Ho * d.Wo, K = d.C0;
  SgArgs a;
  a.x = d.x0;
  a.w = d.w;
  a.bias = d.bias ? d.bias : static_cast<const float*>(dummy);
  a.colsum = d.ln_colsum ? d.ln_colsum : a.bias;
  a.out = d.out;
  a.prof = d.prof;
  a.K = K;
  a.nk = K / SG_BK;
  a.ldo = d.N / 2;
  a.has_bias = d.bias != nullptr;
  a.lnf = d.ln_colsum != nullptr;
  a.ln_eps = d.ln_eps;
  a.order = sm_tile_order(M, d.N, K, M / bm, d.N / SG_WROWS);   // (palettized too: from the fp16 operand sizes)
  return a;
}

}  // namespace

bool smgeglu_pal_shape_ok(const ConvDesc& d, int variant) {
  return variant >= 0 && variant <= 2 && sg_bm(d, variant) == 128 && sg_tiles(d, 128) && d.C0 <= kSgPalMaxK && !d.prof;
}

void launch_smgeglu_pal(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  SD_REQUIRE(p.bm == 128 && sg_tiles(d, p.bm) && d.C0 <= kSgPalMaxK && !d.prof && d.cw.kind == WeightSource::PalGeglu && d.cw.stream && d.cw.lut &&
                 palette_bits_ok(d.cw.bits) && (d.cw.ln_gamma != nullptr) == (d.ln_colsum != nullptr),
             kInvalidArgument,
             "plan tile 16 (smgeglu.hip, palettized): not a 1x1 GEGLU projection it tiles with 128-row tiles, or no palette / norm weight "
             "(C0=%d N=%d M=%d bm=%d bits=%d)", d.C0, d.N, d.B * d.Ho * d.Wo, p.bm, d.cw.bits);
  SgPalArgs a;
  static_cast<SgArgs&>(a) = sg_common_args(d, p.bm, d.cw.pal());   // the stream holds at least 64 N bytes
  a.pal = d.cw.pal();
  a.lut = d.cw.lut;
  a.gamma = d.cw.ln_gamma;
  a.nhalf = 2 * smgemm_pal_groups(d.C0);
  const unsigned nwg = (unsigned)(d.B * d.Ho * d.Wo / p.bm) * (d.N / SG_WROWS);
  conv_plan_log(d, p, a.order.n_fast);
  pal_dispatch_bits(d.cw.bits, "palettized smgeglu", [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    constexpr size_t lds = SgPalCfg<128, NB>::LDS;
    auto k = smgeglu_pal_kernel<128, NB>;
    static DynLdsOnce once;
    once.set(k, lds);
    hipLaunchKernelGGL(k, dim3(nwg), dim3(64 * SG_NW), lds, s, a);
  });
  SD_HIP(hipGetLastError());
}

void launch_smgeglu(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  SD_REQUIRE(sg_tiles(d, p.bm), kInvalidArgument,
             "plan tile 13 (smgeglu.hip): not a single-source 1x1 GEGLU projection it tiles (C0=%d N=%d M=%d)", d.C0, d.N, d.B * d.Ho * d.Wo);
  const int bm = p.bm;
  const unsigned nwg = (unsigned)(d.B * d.Ho * d.Wo / bm) * (d.N / SG_WROWS);
  const SgArgs a = sg_common_args(d, bm, d.w);   // K >= 64: the weights hold more than N floats
  conv_plan_log(d, p, a.order.n_fast);
  if (bm == 128) {
    if (d.prof) sg_launch<128, true>(a, nwg, s);
    else sg_launch<128, false>(a, nwg, s);
  } else {
    if (d.prof) sg_launch<256, true>(a, nwg, s);
    else sg_launch<256, false>(a, nwg, s);
  }
  SD_HIP(hipGetLastError());
}

}  // namespace sd
