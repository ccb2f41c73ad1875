// What the whole-LDS-ring kernels (smgemm.hip, smgeglu.hip and their int8 forms) share around their K loops: the XCD-aware tile order -
// the host's four numbers and the division-free prologue that reads them - and the register epilogue's rounding and lane exchange.
// (sm_ring.h: the counted waits; sm_i8_ring.h: what only the int8 forms share.)
// The device helpers take and return VALUES and hold no arithmetic the compiler re-associates with its surroundings: with those two
// properties hipcc's code for the kernels is the code of the same text written in place (LAB_NOTES.md, "one body").
#pragma once
#include "conv_plan.h"
#include "sd_common.h"

namespace sd {

struct SmTileOrder {
  unsigned per_xcd;      // workgroups of one XCD's contiguous tile run (grid % 8 == 0)
  unsigned fast_div;     // tiles along the fast dimension (>= 2)
  unsigned fast_magic;   // floor(2^32 / fast_div) + 1: mulhi(t, magic) == t / fast_div for t * fast_div < 2^32
  int n_fast;            // 1: consecutive tiles share an activation panel, 0: a weight panel (igemm_device.h IgemmArgs::n_fast)
};

// tile order by the bytes each pulls into the 8 XCD L2s, from the fp16 operand sizes: m fastest streams every weight panel once and
// the activations once per XCD; n fastest the other way round (no A/B switch here)
inline SmTileOrder sm_tile_order(int M, int N, int K, unsigned mt, unsigned nt) {
  SmTileOrder o;
  o.per_xcd = mt * nt / 8;
  o.n_fast = choose_tile_order(2.0 * M * K, 2.0 * N * K, (double)mt, (double)nt, false);
  o.fast_div = o.n_fast ? nt : mt;
  o.fast_magic = (unsigned)((1ull << 32) / o.fast_div + 1);
  return o;
}

// (m tile, n tile) of this workgroup.  Block b runs on XCD b % 8: XCD x walks tiles [x * per_xcd, (x + 1) * per_xcd)
__device__ __forceinline__ void sm_tile_coords(SmTileOrder o, int& m_tile, int& n_tile) {
  const unsigned t = (blockIdx.x & 7u) * o.per_xcd + (blockIdx.x >> 3);
  const unsigned slow = __umulhi(t, o.fast_magic);
  const unsigned fast = t - slow * o.fast_div;
  m_tile = (int)(o.n_fast ? slow : fast);
  n_tile = (int)(o.n_fast ? fast : slow);
}

// The register epilogue's exchange.  Lane (g, r16) holds columns 4 g .. 4 g + 3 of pixel r16 of two 16 x 16 accumulator blocks (rows
// 16 (2p) .., 16 (2p + 1) ..), rounded to fp16 pairs: lo0 | hi0 of the first block, lo1 | hi1 of the second.  The odd 16-lane rows of
// the first block trade with the even rows of the second (v_permlane16_swap): afterwards the lane holds columns 8 (g >> 1) .. + 7 of
// row 16 (2p + (g & 1)) + r16 - 16 B of one output row - the first four in the `vdst` results.
__device__ __forceinline__ half8 sm_swap16(unsigned lo0, unsigned lo1, unsigned hi0, unsigned hi1) {
  const auto s0 = __builtin_amdgcn_permlane16_swap(lo0, lo1, false, false);
  const auto s1 = __builtin_amdgcn_permlane16_swap(hi0, hi1, false, false);
  const unsigned d0 = s0[0], d1 = s1[0], d2 = s0[1], d3 = s1[1];   // scalars first (igemm.hip xor32_sum)
  return __builtin_bit_cast(half8, (uintx4){d0, d1, d2, d3});
}

// ... from fp32: sm_round4 rounds the lane's four columns of one block to fp16 once, {lo | hi}, as soon as the block has them (where
// the roundings stand decides hipcc's schedule of the epilogue); sm_pack16 exchanges the two blocks
__device__ __forceinline__ uintx2 sm_round4(floatx4 v) {
  const half2v h01 = {(half_t)v[0], (half_t)v[1]};
  const half2v h23 = {(half_t)v[2], (half_t)v[3]};
  return uintx2{__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23)};
}
__device__ __forceinline__ half8 sm_pack16(uintx2 b0, uintx2 b1) { return sm_swap16(b0[0], b1[0], b0[1], b1[1]); }

}  // namespace sd
