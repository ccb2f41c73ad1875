// What the int8 small-M kernels (smgemm_i8.hip, smgeglu_i8.hip, smqkv_i8.hip, smgemm_q8.hip: plan tiles 19, 20, 22, 24) share: the LDS
// image of a 1-KiB LDS-DMA piece, the geometry, issue and counted wait of the ring of tiles 20 and 22 (tile 24 runs the same issue and
// wait over a five-wave geometry of its own, SmQ8Cfg in smgemm_q8.hip), the epilogue's arithmetic and the host launch.
// (sm_ring.h: the ladder behind the counted waits, here with the LDS counter drained in front of the barrier; sm_tile.h: tile order,
// sm_round4 / sm_pack16.)  As in sm_tile.h the device helpers hold no arithmetic the compiler re-associates with its surroundings.
//
// THE PIECE: 16 rows x 64 B of int8, weights and activations alike.  LDS image [16 rows][4 x 16 B], the 16-B chunk kc of row r at
// position kc ^ F((r >> 2) & 3), F = (0, 2, 3, 1) (an involution per row), applied on the source address.  A fragment read is lane
// (g, r16) -> row r16, chunk g.  A ds_read_b128 lane group ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} of each 32-lane half) holds every
// row residue mod 4 four times: chunk c on row quads R = 0, 3 and chunk c ^ 1 on R = 1, 2 (or the other way round).  Their positions
// c ^ F(0), c ^ F(3), c ^ 1 ^ F(1), c ^ 1 ^ F(2) = c ^ (0, 1, 3, 2) and c ^ F(1), c ^ F(2), c ^ 1 ^ F(0), c ^ 1 ^ F(3) = c ^ (2, 3, 1, 0)
// are four different ones: 16 distinct 16-B slots of the 256-B bank row.  (The halo kernel's kc ^ ((r >> 2) & 3) serves lanes that all
// read the SAME chunk; here the two 16-lane rows of a group read different ones.)
//
// THE RING of tiles 20 and 22 (tile 19 keeps its own: wave-private strips, a staging part, a quantized image).  A workgroup is ten waves
// = 5 pairs of weight strips x 2 row halves over BM x 160 weight rows, BM = 128 / 256.  A stage is K64: [10 weight strips | BM / 16
// activation strips], every strip one piece - 18 / 26 KB, 8 / 6 stages = 144 / 156 KB of the 160.  Pieces: wave + 10 j; the first
// FULL = 8 / 6 waves issue PPW = 2 / 3 per stage, the others one less, and every wave counts its own vmcnt (two instances of the ladder
// behind a wave-uniform branch).  The K loop, step s (NST the ring depth), one barrier per stage:
//     [wait_stage(s): this wave's pieces of stage s have landed | lgkmcnt(0) | s_barrier]
//     issue stage s + NST - 1 -> slot (s - 1) % NST;  read the two weight fragments and the TM activation fragments of stage s;  MFMAs
//   * RAW: a stage is read behind the barrier that follows every wave's counted wait for its own pieces of it.
//   * WAR: slot (s - 1) % NST held stage s - 1; every wave has its fragments of that stage in registers (the lgkmcnt(0) in front of the
//     barrier of step s) before any wave issues into the slot behind that barrier.
//   * counted wait of step s: issued are stages 0 .. min(s + NST - 2, nk - 1); younger than stage s are min(NST - 2, nk - 1 - s) stages
//     of this wave's pieces and, while s <= NST - 2, the EPI epilogue loads: the kernel issues exactly EPI vector loads per lane between
//     its fill of the first NST - 1 stages and its K loop, inside two sched_barriers, and names that number in its SmI8RingCfg.
// WHAT STAYS IN THE KERNELS, in their own text: the piece sources, the fill and the K loop.  hipcc simplifies a helper before it inlines
// it, and each of the three, moved into a helper, changes the kernels' code (LAB_NOTES round 30); issue and wait_stage were lambdas that
// captured the kernel's locals by reference, and SmI8Ring is that closure written out.
#pragma once
#include "kernels.h"
#include "quantize8.h"
#include "sm_ring.h"
#include "sm_tile.h"

namespace sd {

constexpr int SM_I8_BK = 64;              // K bytes per ring stage and row
constexpr int SM_I8_LDS = 160 * 1024;

// position of the 16-B chunk kc in a 64-B row of row quad R = (row >> 2) & 3: kc ^ F(R), F = (0, 2, 3, 1)
__device__ __forceinline__ int sm_i8_swz(int kc, int row) { return kc ^ ((0x78 >> (2 * ((row >> 2) & 3))) & 3); }

// the int8 epilogue's arithmetic for one accumulator: one conversion, one product, the bias in fp32, each operation rounded on its own
// (hipcc contracts a * b + c into an fma by default).  What a kernel puts behind it is a rounding of its own too.
__device__ __forceinline__ float sm_i8_affine(int acc, float cs, float bias, bool has_bias) {
#pragma clang fp contract(off)
  float v = (float)acc * cs;
  if (has_bias) v = v + bias;
  return v;
}
// ... and the plain GEMM's ending (tiles 19 and 24) for one element: the residual meets the fp32 value, in a rounding of its own
__device__ __forceinline__ float gemm_value(int acc, float cs, float bias, bool has_bias, float res, bool has_res) {
#pragma clang fp contract(off)
  float v = sm_i8_affine(acc, cs, bias, has_bias);
  if (has_res) v = v + res;
  return v;
}

constexpr int SM_I8_WROWS = 160;         // weight rows per workgroup of the ring: ten 16-row strips
constexpr int SM_I8_NW = 10;              // waves: strip pair x row half

// geometry of the ring: what the host needs too
template <int BM>
struct SmI8RingGeom {
  static constexpr int PIECES = (SM_I8_WROWS + BM) / 16;          // pieces per stage: weights, then activations
  static constexpr int PPW = (PIECES + SM_I8_NW - 1) / SM_I8_NW;  // pieces per wave per stage: the first FULL waves; the others one less
  static constexpr int FULL = PIECES - SM_I8_NW * (PPW - 1);
  static constexpr int STAGE = PIECES * 1024;
  static constexpr int NST = SM_I8_LDS / STAGE;                   // ring depth: 8 / 6
  static constexpr int TM = BM / 32;                              // 16-row blocks per wave (one row half)
  static constexpr size_t LDS = (size_t)NST * STAGE;
  static_assert(BM % 128 == 0 && PPW >= 2 && FULL >= 1 && FULL <= SM_I8_NW, "tile");
  static_assert(NST >= 3 && LDS <= SM_I8_LDS, "ring");
};
// ... and EPI, the epilogue loads per lane that the kernel issues behind its fill and the counted waits count
template <int BM, int EPI_>
struct SmI8RingCfg : SmI8RingGeom<BM> {
  static constexpr int EPI = EPI_;
  static_assert(SmI8RingGeom<BM>::PPW * (SmI8RingGeom<BM>::NST - 2) + EPI <= 63, "vmcnt range");
};

// issue and counted wait over the kernel's ring state: full = this wave issues PPW pieces per stage (wave < FULL); slot j of the wave is
// piece p = wave + 10 j (tile 24: wave + 5 j; wrapped at PIECES: never issued), pdst[j] = 1024 p, src[j] = the lane's 16 B of it in the next stage to issue
template <class C>
struct SmI8Ring {
  static constexpr int NST = C::NST, PPW = C::PPW;
  char* smem;
  const bool& full;
  const int8_t* (&src)[PPW];
  int (&pdst)[PPW];

  // the next ring stage into slot `slot`
  __device__ __forceinline__ void issue(int slot) const {
    char* st = smem + slot * C::STAGE;
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      if (j == PPW - 1 && !full) break;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src[j],
                                       (__attribute__((address_space(3))) void*)(st + pdst[j]), 16, 0, 0);
      src[j] += SM_I8_BK;
    }
  }

  // this wave's pieces of stage s (of nk) have landed, every wave's LDS reads are done, barrier
  __device__ __forceinline__ void wait_stage(int s, int nk) const {
    const int ahead = min(NST - 2, nk - 1 - s);
    if (full) {
      if (s <= NST - 2) sm_wait<PPW, C::EPI, NST - 2, true>(ahead);
      else sm_wait<PPW, 0, NST - 2, true>(ahead);
    } else {
      if (s <= NST - 2) sm_wait<PPW - 1, C::EPI, NST - 2, true>(ahead);
      else sm_wait<PPW - 1, 0, NST - 2, true>(ahead);
    }
  }
};

// launch of the int8 small-M kernel K, one workgroup of `waves` waves per tile; its dynamic LDS size is set once per kernel and device
template <auto K, class Args>
void sm_i8_launch(const Args& a, unsigned nwg, int waves, size_t lds, hipStream_t s) {
  static DynLdsOnce once;
  once.set(K, lds);
  hipLaunchKernelGGL(K, dim3(nwg), dim3(64 * waves), lds, s, a);
}

}  // namespace sd
