// The tap-step schedule shared by the 3x3 / stride-1 halo kernels (conv3x3_halo.hip plan tile 7, conv3x3_halo_i8.hip plan tile 18):
// halo geometry, which halo pieces a wave issues in which tap step, and the counted waits that follow from that order.
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
