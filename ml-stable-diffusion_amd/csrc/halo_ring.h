// What the 3x3 / stride-1 halo kernels share (conv3x3_halo.hip plan tile 7, conv3x3_halo_i8.hip plan tile 18, conv3x3_halo_sp.hip plan
// tile 21, conv3x3_halo_pal.hip plan tile 25): halo geometry, which halo pieces a wave issues in which tap step, the counted waits that
// follow from that order (tiles 7 / 18 / 25; tile 21 has a four-step schedule of its own), and at the end the statements they share
// as text: workgroup placement, source switch, chunk walk.
// Included behind igemm_device.h; everything sits in an unnamed namespace like the helpers there.
#pragma once
#include "igemm_device.h"

namespace sd {

namespace {

constexpr int HALO_W = 18, HALO_ROWS = 180, HALO_PIECES = 23, HALO_LDS_ROWS = kHaloLdsRows, HALO_PPW = 6;

constexpr int halo_mod9(int t) { return ((t % 9) + 9) % 9; }
// halo pieces of the NEXT chunk a wave issues in tap step `tap`.  Plain kernel: one per step in steps 0-5.  GNL (GroupNorm in the
// loader): two in step 0, one in steps 1-4 - the last piece must have LANDED one step before the halo is first read (step 8), so
// that its owner can still transform it in place behind the barrier of step 7.
template <bool GNL = false>
constexpr int halo_x_issued(int tap) {
  const int t = halo_mod9(tap);
  return GNL ? (t == 0 ? 2 : (t <= 4 ? 1 : 0)) : (t < HALO_PPW ? 1 : 0);
}
// D = stages of the weight ring (D - 1 tap steps of weights in flight; 2 = the round-1 double buffer): halo_lds_bytes (conv_plan.h)

template <int D, int WR, bool GNL = false>
constexpr int halo_ks_wait_count(int tap) {
  // VMEM ops a wave has issued after the weight tile of step s+1 when it waits in step s (tap `tap`): per step, in
  // order, [WR weight pieces of step s'+D] [one halo piece of the next chunk when tap(s') < HALO_PPW]
  // (the halo piece issued in the same step as the awaited tile is waited for too: the count then does not depend on
  // the order of the DMA instructions inside one step)
  int n = 0;
  for (int i = 2; i <= D - 1; ++i) n += WR + halo_x_issued<GNL>(tap - D + i);
  if (tap == 8 && n > 2 * WR) n = 2 * WR;   // the next chunk's halo (last piece went out at tap 5) is read right after
  return n;
}
template <int D, int WR, bool GNL = false>
__device__ __forceinline__ void halo_ks_wait(int tap) {
  switch (tap) {
    case 0: wait_vmcnt_barrier<halo_ks_wait_count<D, WR, GNL>(0)>(); break;
    case 1: wait_vmcnt_barrier<halo_ks_wait_count<D, WR, GNL>(1)>(); break;
    case 2: wait_vmcnt_barrier<halo_ks_wait_count<D, WR, GNL>(2)>(); break;
    case 3: wait_vmcnt_barrier<halo_ks_wait_count<D, WR, GNL>(3)>(); break;
    case 4: wait_vmcnt_barrier<halo_ks_wait_count<D, WR, GNL>(4)>(); break;
    case 5: wait_vmcnt_barrier<halo_ks_wait_count<D, WR, GNL>(5)>(); break;
    case 6: wait_vmcnt_barrier<halo_ks_wait_count<D, WR, GNL>(6)>(); break;
    case 7: wait_vmcnt_barrier<halo_ks_wait_count<D, WR, GNL>(7)>(); break;
    default: wait_vmcnt_barrier<halo_ks_wait_count<D, WR, GNL>(8)>(); break;
  }
}

// ... in the final chunk of a workgroup's K range: weight tiles are issued only while they exist (tap + D < 9), no halo
// pieces; steps before the chunk (u < 0) count as one full weight tile each (conservative: their halo pieces are waited for)
template <int D, int WR>
constexpr int halo_ks_wait_count_last(int tap) {
  int n = 0;
  for (int u = tap - D + 2; u <= tap - 1; ++u) n += (u < 0 || u + D < 9) ? WR : 0;
  return n;
}
template <int D, int WR>
__device__ __forceinline__ void halo_ks_wait_last(int tap) {
  switch (tap) {
    case 0: wait_vmcnt_barrier<halo_ks_wait_count_last<D, WR>(0)>(); break;
    case 1: wait_vmcnt_barrier<halo_ks_wait_count_last<D, WR>(1)>(); break;
    case 2: wait_vmcnt_barrier<halo_ks_wait_count_last<D, WR>(2)>(); break;
    case 3: wait_vmcnt_barrier<halo_ks_wait_count_last<D, WR>(3)>(); break;
    case 4: wait_vmcnt_barrier<halo_ks_wait_count_last<D, WR>(4)>(); break;
    case 5: wait_vmcnt_barrier<halo_ks_wait_count_last<D, WR>(5)>(); break;
    case 6: wait_vmcnt_barrier<halo_ks_wait_count_last<D, WR>(6)>(); break;
    default: wait_vmcnt_barrier<halo_ks_wait_count_last<D, WR>(7)>(); break;
  }
}

}  // namespace

}  // namespace sd

// ---- statements the halo kernels share as TEXT ----
// Statement macros, not functions: by-value force-inlined helpers changed the generated code of 14 of tile 7's 16 instantiations
// (LAB_NOTES.md round 35); as text every kernel compiles to what its own copy compiled to.  The epilogue of tiles 7 / 21 / 25 is
// shared the same way: halo_epilogue.inc.

// Workgroup placement (all four kernels): blockIdx.x -> a contiguous range of tiles per XCD (workgroups go to the eight XCDs round
// robin), then -> (bn_idx, mt) in the order the launcher chose.  Reads nwg, n_tiles, m_tiles, a.n_fast; declares bid, bn_idx, mt.
#define HALO_PLACE_WG                                                                                                      \
  int bid = blockIdx.x;                                                                                                    \
  {                                                                                                                        \
    int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;                                                          \
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;                                                    \
    bid = base + idx;                                                                                                      \
  }                                                                                                                        \
  const int bn_idx = a.n_fast ? bid % n_tiles : bid / m_tiles, mt = a.n_fast ? bid / n_tiles : bid % m_tiles;

// The halo of one channel chunk (tiles 7 and 18): which of the two concatenated sources it comes from is decided once per chunk.
// Declares rs / off[] / soff for chunk `ch` as plain locals; reads a, xpix, hoff0[], hoff1[].  `single`: a compile-time switch - the
// kernel has one source only (tile 7's GroupNorm loader: 6 VGPRs of offsets less).  (Tile 25 forms its offsets per piece: its own macro.)
#define HALO_SRC(single, rs, off, soff, ch)                                                                                \
  const bool rs##_second = !(single) && (ch) * BK >= a.C0; /* wave-uniform */                                              \
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(                                                     \
      const_cast<half_t*>(rs##_second ? a.x1 : a.x0), 0, (int)(xpix * (rs##_second ? a.C1 : a.C0) * 2), 0x00020000);       \
  const int soff = (rs##_second ? (ch) * BK - a.C0 : (ch) * BK) * 2;                                                       \
  unsigned off[HALO_PPW];                                                                                                  \
  _Pragma("unroll") for (int j_ = 0; j_ < HALO_PPW; ++j_) off[j_] = rs##_second ? hoff1[j_] : hoff0[j_];

// The walk over a K range of nine-step chunks (tiles 7, 18 and 25): chunk(par, last, ch) with PAR = parity of the chunk's first step
// and LAST = the final chunk as compile-time arguments - two chunks per trip, so the register set a chunk starts in is static.
// (Tile 21's chunks have four steps, an even number: its own walk.)
#define HALO_WALK_CHUNKS(chunk, ch_begin, ch_end)                                                                          \
  {                                                                                                                        \
    using T = std::true_type;                                                                                              \
    using F = std::false_type;                                                                                             \
    using P0 = std::integral_constant<int, 0>;                                                                             \
    using P1 = std::integral_constant<int, 1>;                                                                             \
    int ch = ch_begin;                                                                                                     \
    for (; ch + 2 < ch_end; ch += 2) {                                                                                     \
      chunk(P0{}, F{}, ch);                                                                                                \
      chunk(P1{}, F{}, ch + 1);                                                                                            \
    }                                                                                                                      \
    if (ch + 2 == ch_end) {                                                                                                \
      chunk(P0{}, F{}, ch);                                                                                                \
      chunk(P1{}, T{}, ch + 1);                                                                                            \
    } else if (ch + 1 == ch_end) {                                                                                         \
      chunk(P0{}, T{}, ch);                                                                                                \
    }                                                                                                                      \
  }
