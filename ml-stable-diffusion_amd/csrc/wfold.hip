// Weight fold of two back-to-back linear maps with nothing non-linear between them (the tail of a SpatialTransformer:
// ff.net.2 + residual -> proj_out + residual, unet.py:553-563, :594-617):
//   out = Wp (W2 g + b2 + h2) + bp + x  ==  [Wp W2 | Wp] [g | h2] + (Wp b2 + bp) + x
// so the two GEMM launches become one GEMM over the K-concatenation of g and h2 (UNet::transformer_block).  This file builds the
// merged operands, once per handle:
//   merged[n][0 .. K)      = fp16( sum_j Wp[n][j] * W2[j][k] )   fp32 products and accumulation, j ascending, one rounding (RNE)
//   merged[n][K .. K + J)  = Wp[n][:]                            unchanged
//   bm[n]                  = bp[n] + sum_j Wp[n][j] * b2[j]      accumulated in fp64, one rounding to fp32
// A plain LDS-tiled FMA kernel: 8.4 GFLOP per 1280-channel block, a few milliseconds, never on the step's path.  No atomics: the
// result is a function of the inputs alone.
#include "kernels.h"

namespace sd {

namespace {

constexpr int WF_T = 64;    // output tile (n x k) per workgroup: 256 threads, 4 x 4 outputs each
constexpr int WF_J = 16;    // j per LDS stage

__global__ __launch_bounds__(256) void wfold_kernel(const half_t* __restrict__ wp, const half_t* __restrict__ w2, half_t* __restrict__ out,
                                                    int N, int J, int K, int ldo) {
  __shared__ float As[WF_J][WF_T + 4];   // Wp tile, j-major
  __shared__ float Bs[WF_J][WF_T + 4];   // W2 tile
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int n0 = blockIdx.y * WF_T, k0 = blockIdx.x * WF_T;
  float acc[4][4] = {};
  for (int j0 = 0; j0 < J; j0 += WF_J) {
    {   // Wp[n0 + tid / 4][j0 + 4 (tid % 4) ..]
      const int n = n0 + (tid >> 2), jj = (tid & 3) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + jj + e;
        As[jj + e][tid >> 2] = (n < N && j < J) ? (float)wp[(size_t)n * J + j] : 0.f;
      }
    }
    {   // W2[j0 + tid / 16][k0 + 4 (tid % 16) ..]
      const int j = j0 + ty;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 4 * tx + e;
        Bs[ty][4 * tx + e] = (j < J && k < K) ? (float)w2[(size_t)j * K + k] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WF_J; ++j) {
      float a[4], b[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] = As[j][4 * ty + e];
        b[e] = Bs[j][4 * tx + e];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(a[r], b[c], acc[r][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + 4 * ty + r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = k0 + 4 * tx + c;
      if (n < N && k < K) out[(size_t)n * ldo + k] = (half_t)acc[r][c];
    }
  }
}

// one 64-lane workgroup per output row: the Wp copy behind the folded columns, and the folded bias (lane-strided fp64 partial
// sums, combined in a fixed tree)
__global__ __launch_bounds__(64) void wfold_row_kernel(const half_t* __restrict__ wp, const float* __restrict__ bp, const float* __restrict__ b2,
                                                       half_t* __restrict__ out, float* __restrict__ bm, int J, int K, int ldo) {
  __shared__ double red[64];
  const int n = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int j = lane; j < J; j += 64) {
    const half_t w = wp[(size_t)n * J + j];
    out[(size_t)n * ldo + K + j] = w;
    s += (double)(float)w * (double)b2[j];
  }
  red[lane] = s;
  __syncthreads();
  for (int d = 32; d > 0; d >>= 1) {
    if (lane < d) red[lane] += red[lane + d];
    __syncthreads();
  }
  if (lane == 0) bm[n] = (float)((double)bp[n] + red[0]);
}

}  // namespace

void launch_wfold(const half_t* wp, const float* bp, const half_t* w2, const float* b2, half_t* merged, float* bm, int N, int J, int K,
                  hipStream_t s) {
  SD_REQUIRE(wp && bp && w2 && b2 && merged && bm && N > 0 && J > 0 && K > 0, kInvalidArgument, "weight fold: N=%d J=%d K=%d", N, J, K);
  const int ldo = K + J;
  hipLaunchKernelGGL(wfold_kernel, dim3(cdiv(K, WF_T), cdiv(N, WF_T)), dim3(256), 0, s, wp, w2, merged, N, J, K, ldo);
  hipLaunchKernelGGL(wfold_row_kernel, dim3(N), dim3(64), 0, s, wp, bp, b2, merged, bm, J, K, ldo);
  SD_HIP(hipGetLastError());
}

}  // namespace sd
