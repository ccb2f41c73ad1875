// Host-side weight layout rules, stated once: the UNet builder (unet.cpp) and the operator entry points (capi_ops.cpp) both
// call these, so an operator test checks the layout the step runs.  Plain host C++: no HIP call, no allocation.
#pragma once
#include <cstddef>

#include "sd_common.h"

namespace sd {

// GEGLU (ff.net.0.proj, unet.py:613-617): destination row of output row o of an n-row [values | gates] matrix.  Value and gate
// channels interleave in blocks of 32, so the GEMM epilogue multiplies them in registers (the device-side twin of this rule is
// conv_generic_kernel's, conv_small.hip).
inline int geglu_row(int o, int n) {
  const int half_n = n / 2;
  const bool gate = o >= half_n;
  const int j = gate ? o - half_n : o;
  return (j / 32) * 64 + (gate ? 32 : 0) + (j % 32);
}

// [Cout][Cin][k][k] (or Linear [Cout][Cin], k = 1) -> [Cout][k][k][Cin]; geglu: rows move through geglu_row
template <typename S, typename D>
void retile_ohwi(const S* src, int cout, int cin, int k, bool geglu, D* dst) {
  const int kk = k * k;
  for (int o = 0; o < cout; ++o) {
    const int dst_o = geglu ? geglu_row(o, cout) : o;
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < kk; ++t) dst[((size_t)dst_o * kk + t) * cin + c] = (D)src[((size_t)o * cin + c) * kk + t];
  }
}

// LayerNorm folded into the projection behind it, one projection w [cout][cin] (+ bias or NULL):
//   y = LN(x) . W^T + b  ==  rstd*(x . (W*gamma)^T) - rstd*mean*colsum(W*gamma) + (b + W.beta)
// Writes rows row0 + o (geglu: geglu_row(o, cout)) of w_out [..][cin], colsum and bias_out.  gamma == beta == NULL: the weights
// are copied unchanged and the bias passes through.  colsum sums what the MFMA actually multiplies: the fp16-rounded values.
template <typename W>
void fold_layernorm_rows(const W* w, const float* bias, const float* gamma, const float* beta, int cout, int cin, int row0,
                         bool geglu, half_t* w_out, float* colsum, float* bias_out) {
  for (int o = 0; o < cout; ++o) {
    const int dst = geglu ? geglu_row(o, cout) : row0 + o;
    double cs = 0.0, bb = bias ? (double)bias[o] : 0.0;
    for (int c = 0; c < cin; ++c) {
      const float wv = (float)w[(size_t)o * cin + c];
      const half_t h = gamma ? (half_t)(wv * gamma[c]) : (half_t)w[(size_t)o * cin + c];
      w_out[(size_t)dst * cin + c] = h;
      cs += (double)(float)h;
      if (beta) bb += (double)wv * (double)beta[c];
    }
    colsum[dst] = (float)cs;
    bias_out[dst] = (float)bb;
  }
}

}  // namespace sd
