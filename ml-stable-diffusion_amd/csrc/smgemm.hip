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
#include <utility>

#include "conv_plan.h"
#include "kernels.h"
#include "pal_decode.h"
#include "sm_ring.h"
#include "sm_tile.h"
#include "weight_prep.h"

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
  SmTileOrder order;
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

  int m_tile, n_tile;
  sm_tile_coords(a.order, m_tile, n_tile);
  const int m_blk = m_tile * BM, n_blk = n_tile * SM_BN;

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

  // ---- epilogue: bias in fp32, one rounding to fp16, blocks (2p, 2p + 1) paired by sm_swap16 -> 16 B of one output row per lane ----
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
    half8 o = sm_swap16(lo[0], lo[1], hi[0], hi[1]);
    if (a.has_res) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)o[e] + (float)resv[p][e]);
    }
    const int m = m_blk + 32 * p + 16 * (g & 1) + r16;
    out_store(reinterpret_cast<half8*>(a.out + (size_t)m * a.N + n), o);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The second kernel of this file: the same GEMM from PALETTIZED weights (plan tile 15).  Geometry, MFMAs, their order per accumulator
// block (ascending K64 stage, then kk = 0, 1), tile order (sm_tile.h) and epilogue are smgemm_kernel's, so the output is bit-identical
// to smgemm_kernel<BM> on lut[indices].  The K loop is its own - another ring, other wait arithmetic - because of where the weight
// fragment comes from:
//   * no fp16 weight exists anywhere.  Lane (g, r16) of wave w owns the bit stream of its palette indices (weight_prep.h
//     smgemm_pal_pack: NBITS coalesced 16-B words per GROUP of 8 stages), keeps the current group's words in registers and turns every
//     index into one 2-byte LDS read of the LUT, placed in the low or high half of a fragment register.  Field positions are
//     compile-time constants (the 8 stages of a group are unrolled); the two fragments of stage s + 1 are decoded beside the MFMAs of
//     stage s (register double buffer wf[2]);
//   * the index words arrive by LDS-DMA too: one 1-KB piece per word into the wave's own two group buffers, from where the lane
//     takes its 16 B back with one ds_read_b128 per word and group.  They were ordinary loads first; hipcc then waits vmcnt(0) in front
//     of EVERY use of a word register while LDS-DMA is in flight (seen in the assembly: one full drain of the ring per stage), and
//     the loads cannot be hidden from it without inline assembly.  As pieces they are counted by hand with everything else;
//   * the LUT (zero-padded to kPalLutHalves) is ONE COPY PER WAVE, brought by two 4-byte LDS-DMA pieces of the wave itself in front of
//     everything else: no barrier and no register pass of its own - the counted wait for stage 0 retires it (pieces retire in
//     order), and a workgroup copy would make five waves share its two pieces unevenly;
//   * the ring holds the BM activation rows only: NST = 16 / 8 stages of K64 (BM = 32 / 64), BM / 8 pieces of 1 KB each.  Five waves
//     issue PPW = 1 / 2 pieces per stage; the 1 / 2 pieces beyond BM / 8 repeat activation rows into a dump slot behind the ring that
//     nothing reads, so every wave issues the same number of pieces and one immediate serves all.
// Order of the LDS-DMA pieces of a wave (they share vmcnt and retire in order; the only ordinary loads, bias and residual rows, come
// first and are used behind the loop):
//     [LUT: 2] [W_0 -> buffer 0: NBITS] [W_1 -> buffer 1: NBITS] [stages 0 .. NST - 2]                          prologue
//     step rel = 8 j + t:  wait for stage rel -> [t == 0: W_(j+2) -> buffer j & 1] [stage rel + NST - 1, if < nk]
// (W_i: the words of group min(i, groups - 1) - behind the last group it is loaded again, so the count is the same at every step).
// Group j + 1 moves from its buffer to registers in step 8 j + 7: W_(j+1) is older than stage 8 j + 7 (issued in step 8 (j - 1) in
// front of stage 8 (j - 1) + NST - 1 <= 8 j + 7), whose wait that step has passed; group 0 in step 0.  Buffer j & 1 is re-filled in
// step 8 j behind an lgkmcnt(0): the reads that emptied it are done.
// Younger than stage rel at the wait of step rel are the `ahead` = min(NST - 2, nk - 1 - rel) stages behind it and every batch W
// issued in a step 8 u < rel with rel <= 8 u + NST - 2 (the last stage issued in front of it):
//     u = j:      0 < t <= NST - 2
//     u = j - 1:  j > 0 and t + 8 <= NST - 2         (u = j - 2: t + 16 <= NST - 2, never for NST <= 17)
//     vmcnt immediate = PPW * ahead + NBITS * (number of those batches).
// t is a compile-time constant of the unrolled group body, j > 0 its `FIRST = false` instantiation.
struct SmPalArgs {
  const half_t* x;      // [M][K]
  const uint8_t* pal;   // [N / 16][groups][NBITS][64 lanes][16 B]
  const half_t* lut;    // kPalLutHalves entries
  const float* bias;    // as SmArgs
  const half_t* res;
  half_t* out;
  int K, N, nk, ngroups, res_ld;
  int has_bias, has_res;
  SmTileOrder order;
};

template <int BM, int NBITS>
struct SmPalCfg {
  static constexpr int PIECES = BM / 8;                          // 1-KiB pieces of real activation rows per stage
  static constexpr int PPW = (PIECES + SM_NW - 1) / SM_NW;       // pieces per wave per stage
  static constexpr int PAD = SM_NW * PPW - PIECES;               // padding pieces per stage: into the dump slots
  static constexpr int STAGE = PIECES * 1024;
  static constexpr int NST = 512 / BM;                           // 64 KB of ring
  static constexpr int G = kSmPalGroup;
  static constexpr int DUMP = NST * STAGE;                       // byte offsets behind the ring
  static constexpr int LUT = DUMP + PAD * 1024;                  // SM_NW copies
  static constexpr int WORDS = LUT + SM_NW * kPalLutHalves * 2;  // per wave: two group buffers of NBITS KB
  static constexpr int LDS = WORDS + SM_NW * 2 * NBITS * 1024;
  static constexpr int TM = BM / 16;
  // index-word batches younger than stage 8 j + t at its wait (header comment)
  static constexpr int batches(int t, bool first) { return ((t > 0 && t <= NST - 2) ? 1 : 0) + ((!first && t + G <= NST - 2) ? 1 : 0); }
  static_assert(BM % 32 == 0 && LDS <= SM_LDS, "tile");
  static_assert(G == 8 && NST >= G && NST <= 2 * G, "the batch count above, and group j + 1 landed by step 8 j + 7");
  static_assert(PPW * (NST - 2) + 2 * NBITS <= 63, "vmcnt range");
};

template <int... I, typename F>
__device__ __forceinline__ void sm_static_for(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}

template <int BM, int NBITS>
__global__ __launch_bounds__(64 * SM_NW, 1) void smgemm_pal_kernel(SmPalArgs a) {
  using C = SmPalCfg<BM, NBITS>;
  constexpr int NST = C::NST, PPW = C::PPW, TM = C::TM, Q = NBITS, G = C::G;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

  int m_tile, n_tile;
  sm_tile_coords(a.order, m_tile, n_tile);
  const int m_blk = m_tile * BM, n_blk = n_tile * SM_BN;
  const int g = lane >> 4, r16 = lane & 15;

  // ---- epilogue operands first (nothing in the K loop counts them), in the store layout as in smgemm_kernel ----
  const floatx4 bias4 = *reinterpret_cast<const floatx4*>(a.bias + n_blk + 16 * wave + 4 * g);
  half8 resv[TM / 2];
#pragma unroll
  for (int p = 0; p < TM / 2; ++p)
    resv[p] = *reinterpret_cast<const half8*>(a.res + (size_t)(m_blk + 32 * p + 16 * (g & 1) + r16) * a.res_ld + n_blk + 16 * wave +
                                              8 * (g >> 1));
  __builtin_amdgcn_sched_barrier(0);
  // ---- this wave's copy of the LUT: 2 x (64 lanes x 4 B) by LDS-DMA ----
  char* const lut_lds = smem + C::LUT + wave * (kPalLutHalves * 2);
#pragma unroll
  for (int h = 0; h < 2; ++h)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.lut + h * 128 + lane * 2),
                                     (__attribute__((address_space(3))) void*)(lut_lds + h * 256), 4, 0, 0);
  const unsigned short* const lutp = reinterpret_cast<const unsigned short*>(lut_lds);
  // ---- index words: batch W_i = group min(i, groups - 1) into this wave's buffer i & 1 ----
  char* const wbuf = smem + C::WORDS + wave * (2 * Q * 1024);
  const uintx4* const wbase = reinterpret_cast<const uintx4*>(a.pal) + (size_t)(n_blk / 16 + wave) * a.ngroups * (Q * 64) + lane;
  auto issue_words = [&](int i) __attribute__((always_inline)) {
    const uintx4* p = wbase + (size_t)min(i, a.ngroups - 1) * (Q * 64);
    char* dst = wbuf + (i & 1) * (Q * 1024);
#pragma unroll
    for (int q = 0; q < Q; ++q)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p + q * 64),
                                       (__attribute__((address_space(3))) void*)(dst + q * 1024), 16, 0, 0);
  };
  auto read_words = [&](uintx4(&wq)[Q], int grp) __attribute__((always_inline)) {
    const char* srcw = wbuf + (grp & 1) * (Q * 1024) + lane * 16;
#pragma unroll
    for (int q = 0; q < Q; ++q) wq[q] = *reinterpret_cast<const uintx4*>(srcw + q * 1024);
  };
  issue_words(0);
  issue_words(1);

  // ---- activation staging: piece wave + 5 j of every stage; pieces >= BM / 8 repeat rows into their dump slot ----
  const half_t* src[PPW];
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    const int p = wave + SM_NW * j;
    const int pr = p >= C::PIECES ? p - C::PIECES : p;
    const int r = pr * 8 + (lane >> 3);                   // activation row of the tile
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);        // logical chunk at physical slot lane & 7
    src[j] = a.x + (size_t)(m_blk + r) * a.K + chunk * 8;
  }
  auto issue = [&](int idx) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      const int p = wave + SM_NW * j;                     // wave-uniform
      char* dst = p >= C::PIECES ? smem + C::DUMP + (p - C::PIECES) * 1024 : smem + (idx % NST) * C::STAGE + p * 1024;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src[j],
                                       (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      src[j] += SM_BK;
    }
  };
#pragma unroll
  for (int p = 0; p < NST - 1; ++p)
    if (p < a.nk) issue(p);
  __builtin_amdgcn_sched_barrier(0);

  int foff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) foff[kk] = r16 * 128 + (((4 * kk + g) ^ ((r16 >> 1) & 7)) * 16);

  floatx4 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};

  // the two weight fragments of stage t of a group: fragments 2 t, 2 t + 1 of the lane's stream (pal_decode.h)
  auto decode = [&](half8(&wf)[2], const uintx4(&wq)[Q], auto tc) __attribute__((always_inline)) {
    constexpr int t = decltype(tc)::value;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) wf[kk] = pal_decode<NBITS>(wq, t * 2 + kk, lutp);
  };

  half8 wf[2][2];   // [stage parity][kk]
  // one group of 8 stages: `cur` holds its words, `nxt` receives the next group's in its last stage
  auto run_group = [&](auto first_c, uintx4(&cur)[Q], uintx4(&nxt)[Q], int grp) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first_c)::value;
    sm_static_for(std::make_integer_sequence<int, G>{}, [&](auto tc) __attribute__((always_inline)) {
      constexpr int t = decltype(tc)::value;
      const int rel = grp * G + t;
      if (rel < a.nk) {   // (the same for every wave of every workgroup)
        sm_wait<PPW, Q * C::batches(t, FIRST), NST - 2>(min(NST - 2, a.nk - 1 - rel));
        if constexpr (FIRST && t == 0) {   // group 0 and stage 0's fragments: the wait has retired the LUT and W_0, which are older
          read_words(cur, 0);
          decode(wf[0], cur, std::integral_constant<int, 0>{});
        }
        const char* st = smem + (rel % NST) * C::STAGE;
        half8 xf[2][TM];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int i = 0; i < TM; ++i) xf[kk][i] = *reinterpret_cast<const half8*>(st + 16 * i * 128 + foff[kk]);
        __builtin_amdgcn_sched_barrier(0);   // reads first, then the next DMA, then decode and MFMAs
        if constexpr (t == 0) {
          __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the reads that moved this group out of its buffer are done
          __builtin_amdgcn_sched_barrier(0);
          issue_words(grp + 2);
        }
        if (rel + NST - 1 < a.nk) issue(rel + NST - 1);
        __builtin_amdgcn_sched_barrier(0);
        // stage rel + 1's fragments beside this stage's MFMAs.  Unconditional, so that both stay in one block: behind the last stage
        // it decodes zero padding fields, or the re-loaded last group, into fragments no MFMA consumes
        if constexpr (t == G - 1) {
          read_words(nxt, grp + 1);
          decode(wf[0], nxt, std::integral_constant<int, 0>{});
        } else {
          decode(wf[(t + 1) & 1], cur, std::integral_constant<int, t + 1>{});
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int i = 0; i < TM; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[t & 1][kk], xf[kk][i], acc[i], 0, 0, 0);
      }
    });
  };
  uintx4 wa[Q], wb[Q];
  run_group(std::true_type{}, wa, wb, 0);
  for (int grp = 1; grp < a.ngroups; grp += 2) {
    run_group(std::false_type{}, wb, wa, grp);
    if (grp + 1 < a.ngroups) run_group(std::false_type{}, wa, wb, grp + 1);
  }

  // ---- epilogue: smgemm_kernel's ----
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
    half8 o = sm_swap16(lo[0], lo[1], hi[0], hi[1]);
    if (a.has_res) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)o[e] + (float)resv[p][e]);
    }
    const int m = m_blk + 32 * p + 16 * (g & 1) + r16;
    out_store(reinterpret_cast<half8*>(a.out + (size_t)m * a.N + n), o);
  }
}

// one workgroup per tile: 8 XCD runs of per_xcd tiles
template <class K, class A>
void launch_sm(K kernel, size_t lds, DynLdsOnce& once, const A& a, hipStream_t s) {
  once.set(kernel, lds);
  hipLaunchKernelGGL(kernel, dim3(8 * a.order.per_xcd), dim3(64 * SM_NW), lds, s, a);
}

template <int BM>
void launch_sm_fp16(const SmArgs& a, hipStream_t s) {
  static DynLdsOnce once;
  launch_sm(smgemm_kernel<BM>, (size_t)SmCfg<BM>::NST * SmCfg<BM>::STAGE, once, a, s);
}

template <int BM, int NBITS>
void launch_sm_pal(const SmPalArgs& a, hipStream_t s) {
  static DynLdsOnce once;
  launch_sm(smgemm_pal_kernel<BM, NBITS>, SmPalCfg<BM, NBITS>::LDS, once, a, s);
}

// what SmArgs and SmPalArgs share, for the single source d.x0 of K channels; `dummy`: readable memory of at least N floats that stands
// in for an absent bias / residual row (the loads keep their count).  Returns the tile order's n_fast for the plan log.
template <class A>
int sm_common_args(A& a, const ConvDesc& d, int K, int bm, const void* dummy) {
  const int M = d.B * d.Ho * d.Wo;
  a.x = d.x0;
  a.bias = d.bias ? d.bias : static_cast<const float*>(dummy);
  a.res = d.res ? d.res : static_cast<const half_t*>(dummy);
  a.out = d.out;
  a.K = K;
  a.N = d.N;
  a.nk = K / SM_BK;
  a.res_ld = d.res ? d.N : 0;
  a.has_bias = d.bias != nullptr;
  a.has_res = d.res != nullptr;
  a.order = sm_tile_order(M, d.N, K, M / bm, d.N / SM_BN);
  return a.order.n_fast;
}

int sm_nst(int bm) { return bm == 32 ? SmCfg<32>::NST : SmCfg<64>::NST; }

int sm_bm(const ConvDesc& d, int variant) {   // variant 1 / 2: BM = 32 / 64; 0: by M
  if (variant == 1) return 32;
  if (variant == 2) return 64;
  return (long)d.B * d.Ho * d.Wo <= 1024 ? 32 : 64;
}

// a 1x1 GEMM the kernels tile with bm-row tiles
bool sm_tiles(const ConvDesc& d, int bm) {
  if (!(d.ksize == 1 && d.stride == 1 && d.up == 1 && d.out_mode == kOutHalf && !d.ln_colsum && !d.out_t && !d.temb &&
        d.q_cols == 0 && !d.gnf_partial && d.n_twins == 0 && !d.debug && (bm == 32 || bm == 64)))
    return false;
  const long M = (long)d.B * d.Ho * d.Wo;
  const long mt = M / bm, nt = d.N / SM_BN;
  // a second source starts on a stage boundary, behind the prologue's NST - 1 stages (the kernel switches inside the K loop only)
  if (d.x1 && !(d.C1 % SM_BK == 0 && d.C1 >= SM_BK && d.C0 / SM_BK >= sm_nst(bm))) return false;
  return d.C0 % SM_BK == 0 && d.C0 >= SM_BK && d.N % SM_BN == 0 && M % bm == 0 && mt >= 2 && nt >= 2 && (mt * nt) % 8 == 0 &&
         mt * nt <= 65535;
}

}  // namespace

bool smgemm_shape_ok(const ConvDesc& d, int variant) { return variant >= 0 && variant <= 2 && sm_tiles(d, sm_bm(d, variant)); }

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

int smgemm_bm(const ConvDesc& d, int variant) { return sm_bm(d, variant); }

void launch_smgemm(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  SD_REQUIRE(sm_tiles(d, p.bm), kInvalidArgument, "plan tile 12 (smgemm.hip): not a 1x1 GEMM it tiles (C0=%d C1=%d N=%d)",
             d.C0, d.x1 ? d.C1 : 0, d.N);
  const int bm = p.bm;
  SmArgs a;
  const int n_fast = sm_common_args(a, d, d.C0 + (d.x1 ? d.C1 : 0), bm, d.w);   // K >= 64: the weights hold more than N floats
  a.x1 = d.x1 ? d.x1 : d.x0;
  a.ldx0 = d.C0;
  a.ldx1 = d.x1 ? d.C1 : d.C0;
  a.w = d.w;
  a.nk0 = d.C0 / SM_BK;
  conv_plan_log(d, p, n_fast);
  if (bm == 32) launch_sm_fp16<32>(a, s);
  else launch_sm_fp16<64>(a, s);
  SD_HIP(hipGetLastError());
}

void launch_smgemm_pal(const ConvDesc& d, const ConvPlan& p, hipStream_t s) {
  SD_REQUIRE(sm_tiles(d, p.bm) && !d.x1 && d.cw.kind == WeightSource::PalGemm && d.cw.stream && d.cw.lut && palette_bits_ok(d.cw.bits), kInvalidArgument,
             "plan tile 15 (smgemm.hip, palettized): not a single-source 1x1 GEMM it tiles, or no palette (C0=%d C1=%d N=%d M=%d bits=%d)", d.C0,
             d.x1 ? d.C1 : 0, d.N, d.B * d.Ho * d.Wo, d.cw.bits);
  const int bm = p.bm;
  SmPalArgs a;
  const int n_fast = sm_common_args(a, d, d.C0, bm, d.cw.pal());   // the stream holds at least 64 N bytes; tile 12's order, from the fp16 sizes
  a.pal = d.cw.pal();
  a.lut = d.cw.lut;
  a.ngroups = smgemm_pal_groups(d.C0);
  conv_plan_log(d, p, n_fast);
  pal_dispatch_bits(d.cw.bits, "palettized smgemm", [&](auto nb) {
    if (bm == 32) launch_sm_pal<32, decltype(nb)::value>(a, s);
    else launch_sm_pal<64, decltype(nb)::value>(a, s);
  });
  SD_HIP(hipGetLastError());
}

}  // namespace sd
