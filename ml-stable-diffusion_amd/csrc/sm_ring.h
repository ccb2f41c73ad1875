// Counted waits of the whole-LDS-ring kernels (smgemm.hip, smgeglu.hip and their int8 forms, sm_i8_ring.h): a wave issues the same
// number of LDS-DMA pieces in every ring stage, so one s_waitcnt vmcnt immediate says "the stage to consume has landed" for it.  Where
// that number differs between the waves of a workgroup (smgeglu.hip, tiles 20 and 22: the first FULL waves issue one piece more) each
// wave counts its own, behind a wave-uniform branch.
#pragma once

namespace sd {

// counted wait + raw barrier in one statement (no LDS access moves across).  LGKM: the LDS counter is drained in front of the barrier
// too - the int8 kernels' one barrier per stage also says "every wave has its fragments of the previous stage in registers"
template <int N, bool LGKM = false>
__device__ __forceinline__ void sm_wait_barrier() {
  if constexpr (LGKM) asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
  else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// counted wait for the stage to consume: `ahead` newer ring stages in flight (PPW pieces each), plus E epilogue loads issued after
// it (the immediate must be a literal, hence the ladder)
template <int PPW, int E, int A, bool LGKM = false>
__device__ __forceinline__ void sm_wait(int ahead) {
  if constexpr (A > 0) {
    if (ahead == A) {
      sm_wait_barrier<PPW * A + E, LGKM>();
      return;
    }
    sm_wait<PPW, E, A - 1, LGKM>(ahead);
  } else {
    sm_wait_barrier<E, LGKM>();
  }
}

}  // namespace sd
