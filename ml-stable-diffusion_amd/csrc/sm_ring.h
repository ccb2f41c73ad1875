// Counted waits of the whole-LDS-ring kernels (smgemm.hip, smgeglu.hip): every wave issues the same number of LDS-DMA pieces per
// ring stage, so one s_waitcnt vmcnt immediate says "the stage to consume has landed" for all of them.
#pragma once

namespace sd {

template <int N>
__device__ __forceinline__ void sm_wait_barrier() {   // counted wait + raw barrier in one statement (no LDS access moves across)
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// counted wait for the stage to consume: `ahead` newer ring stages in flight (PPW pieces each), plus E epilogue loads issued after
// it (the immediate must be a literal, hence the ladder)
template <int PPW, int E, int A>
__device__ __forceinline__ void sm_wait(int ahead) {
  if constexpr (A > 0) {
    if (ahead == A) {
      sm_wait_barrier<PPW * A + E>();
      return;
    }
    sm_wait<PPW, E, A - 1>(ahead);
  } else {
    sm_wait_barrier<E>();
  }
}

}  // namespace sd
