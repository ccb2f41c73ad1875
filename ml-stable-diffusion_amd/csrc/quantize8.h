// The W8A8 activation quantizer of the int8 kernels (wstream.hip plan tile 17, conv3x3_halo_i8.hip plan tile 18): one function, so
// a layer is the same function of its inputs whichever of the two runs it.
#pragma once
#include "sd_common.h"

namespace sd {

namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx16 __attribute__((ext_vector_type(16)));

// x_q = clip(rint(fp32(x) * inv_s), -127, 127): one product, v_rndne_f32, a clamp.  NaN -> 0 (it compares false with everything, the
// select keeps 0); +-inf -> +-127 (the clamp saturates them like any large value).  Eight channels -> 8 bytes.
__device__ __forceinline__ uintx2 ws_quantize8(const half8& x, float inv_s) {
  unsigned b[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = __builtin_rintf((float)x[e] * inv_s);
    const float c = v == v ? fminf(fmaxf(v, -127.f), 127.f) : 0.f;
    b[e] = (unsigned)(int)c & 0xffu;
  }
  return uintx2{b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24), b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24)};
}

}  // namespace

}  // namespace sd
