// Direct convolutions for the shapes off the MFMA tiles (tiny / odd channel counts, the 4-channel input conv, N <= 8 outputs):
// one thread or one wavefront per output, fp32 accumulation.  Arguments and the shared tile epilogue: igemm_device.h.
#include "igemm_device.h"

namespace sd {

namespace {

// ---- generic direct convolution: any shape, one thread per output element (tiny/odd layers) ----
__global__ __launch_bounds__(256) void conv_generic_kernel(IgemmArgs a, int silu_out) {
  const bool geglu = a.out_mode == kOutGeglu;
  const int NO = geglu ? a.N / 2 : a.N;
  const size_t total = (size_t)a.M * NO;
  const int Hup = a.Hi * a.up, Wup = a.Wi * a.up, upshift = a.up >> 1;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int m = (int)(idx / NO), no = (int)(idx - (size_t)m * NO);
    const int b = m / a.HoWo;
    const int rem = m - b * a.HoWo;
    const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
    auto dot = [&](int n) {
      float acc = 0.f;
      for (int ky = 0; ky < a.ksize; ++ky)
        for (int kx = 0; kx < a.ksize; ++kx) {
          const int iy = oy * a.stride - a.pad + ky, ix = ox * a.stride - a.pad + kx;
          if (iy < 0 || iy >= Hup || ix < 0 || ix >= Wup) continue;
          const size_t pix = (size_t)b * a.Hi * a.Wi + (size_t)(iy >> upshift) * a.Wi + (ix >> upshift);
          const half_t* wrow = a.w + (size_t)n * a.K + (size_t)(ky * a.ksize + kx) * a.Ctot;
          const half_t* p0 = a.x0 + pix * a.C0;
          for (int c = 0; c < a.C0; ++c) acc += (float)p0[c] * (float)wrow[c];
          if (a.C1) {
            const half_t* p1 = a.x1 + pix * a.C1;
            for (int c = 0; c < a.C1; ++c) acc += (float)p1[c] * (float)wrow[a.C0 + c];
          }
        }
      return acc + (a.bias ? a.bias[n] : 0.f);
    };
    if (geglu) {   // interleaved rows: 32 value channels then their 32 gate channels
      const int nv = (no / 32) * 64 + (no % 32);
      a.out[idx] = (half_t)(dot(nv) * gelu_erf(dot(nv + 32)));
      continue;
    }
    float acc = dot(no);
    if (a.temb) acc += a.temb[(size_t)b * a.temb_stride + no];
    if (a.res) acc += (float)a.res[idx];
    if (silu_out) acc = acc / (1.f + __expf(-acc));
    if (a.out_mode == kOutHalfT)
      a.out[((size_t)b * a.N + no) * a.ldT + rem] = (half_t)acc;
    else
      a.out[idx] = (half_t)acc;
  }
}

// ---- tiny input-channel count (conv_in 4->320, K = 36): 16 output pixels per workgroup, the
// im2col patches live in LDS (broadcast reads), each thread keeps one output channel's K weights
// in registers.  Replaces the generic one-thread-per-output kernel (95 us -> a few us).
constexpr int SC_PIX = 16, SC_KMAX = 72;
__global__ __launch_bounds__(256) void conv_small_cin_kernel(IgemmArgs a, int silu_out) {
  __shared__ float patch[SC_PIX][SC_KMAX];
  const int m0 = blockIdx.x * SC_PIX;
  const int Hup = a.Hi * a.up, Wup = a.Wi * a.up, upshift = a.up >> 1;
  // every column of a patch row is written - K .. SC_KMAX - 1 with zeros: the dot product below runs over all SC_KMAX columns against
  // zero weights there, and 0 * (whatever the LDS held: NaN bit patterns on a fresh box) is NaN (round 6: the tiny test UNet's
  // K = 48 to_k projection failed as the first launch of a process, tools/ubench/poison.hip + SD_NAN_TRACE)
  for (int idx = threadIdx.x; idx < SC_PIX * SC_KMAX; idx += blockDim.x) {
    const int p = idx / SC_KMAX, k = idx - p * SC_KMAX;
    const int m = m0 + p;
    float v = 0.f;
    if (m < a.M && k < a.K) {
      const int b = m / a.HoWo;
      const int rem = m - b * a.HoWo;
      const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
      const int tap = k / a.Ctot, c = k - tap * a.Ctot;
      const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
      const int iy = oy * a.stride - a.pad + ky, ix = ox * a.stride - a.pad + kx;
      if (iy >= 0 && iy < Hup && ix >= 0 && ix < Wup) {
        const size_t pix = (size_t)b * a.Hi * a.Wi + (size_t)(iy >> upshift) * a.Wi + (ix >> upshift);
        v = (c < a.C0) ? (float)a.x0[pix * a.C0 + c] : (float)a.x1[pix * a.C1 + (c - a.C0)];
      }
    }
    patch[p][k] = v;
  }
  __syncthreads();
  for (int n = threadIdx.x; n < a.N; n += blockDim.x) {
    float w[SC_KMAX];
#pragma unroll
    for (int k = 0; k < SC_KMAX; ++k) w[k] = (k < a.K) ? (float)a.w[(size_t)n * a.K + k] : 0.f;
    const float bv = a.bias ? a.bias[n] : 0.f;
    for (int p = 0; p < SC_PIX; ++p) {
      const int m = m0 + p;
      if (m >= a.M) break;
      float acc = bv;
#pragma unroll
      for (int k = 0; k < SC_KMAX; ++k) acc += w[k] * patch[p][k];   // (columns beyond K: zero weights x zero patch)
      if (a.temb) acc += a.temb[(size_t)(m / a.HoWo) * a.temb_stride + n];
      if (a.res) acc += (float)a.res[(size_t)m * a.N + n];
      if (silu_out) acc = acc / (1.f + __expf(-acc));
      a.out[(size_t)m * a.N + n] = (half_t)acc;
    }
  }
}

// ---- 4 input channels (conv_in 4->320, VAE conv_in 4->512): K = 36 on the MFMA ----
// The scalar kernel above spends 30-40 us on SD2.1's conv_in (profiles/r02_final_op_profile.txt) for 0.2 GFLOP.  Here a
// workgroup builds the im2col rows of 128 output pixels (9 taps x 4 channels = 72 B each, zero-padded to three 16-deep
// MFMA steps) and 64 weight rows in LDS - same row swizzle as igemm_kernel - runs 6 MFMAs per wave and leaves through
// the shared tile epilogue (bias, residual = the ControlNet conditioning embedding, coalesced fp16 stores).
__global__ __launch_bounds__(256) void conv3x3_cin4_kernel(IgemmArgs a) {
  constexpr int BM = 128, BN = 64, ROWB = BK * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Xs = smem;                       // [BM][64 halves]; only k < 48 is read
  char* const Ws = smem + BM * ROWB;           // [BN][64 halves]
  float* sconst = reinterpret_cast<float*>(smem + (BM + BN) * ROWB);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nbm = (a.M + BM - 1) / BM;
  const int bn_idx = blockIdx.x / nbm, bm_idx = blockIdx.x % nbm;
  const int m_blk = bm_idx * BM, n_blk = bn_idx * BN;
  typedef unsigned long long u64;
  // one thread per LDS row: threads 0..127 an im2col row, 128..191 a weight row; 8-B pieces at k = 4t, t = 0..11
  if (tid < BM + BN) {
    const bool is_x = tid < BM;
    const int r = is_x ? tid : tid - BM;
    char* row = (is_x ? Xs : Ws) + r * ROWB;
    const int sw = (r >> 1) & 7;
    u64 v[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) v[t] = 0ull;
    if (is_x) {
      const int m = m_blk + r;
      if (m < a.M) {
        const int b = m / a.HoWo, rem = m - b * a.HoWo;
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int iy = oy - 1 + t / 3, ix = ox - 1 + t % 3;
          if (iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi)
            v[t] = *reinterpret_cast<const u64*>(a.x0 + ((size_t)(b * a.Hi + iy) * a.Wi + ix) * 4);
        }
      }
    } else {
      const int n = n_blk + r;
      if (n < a.N) {
#pragma unroll
        for (int t = 0; t < 9; ++t) v[t] = *reinterpret_cast<const u64*>(a.w + (size_t)n * 36 + t * 4);
      }
    }
#pragma unroll
    for (int t = 0; t < 12; ++t)   // logical 16-B chunk t/2 lives in physical slot (t/2) ^ sw
      *reinterpret_cast<u64*>(row + (((t >> 1) ^ sw) * 16) + (t & 1) * 8) = v[t];
  }
  float const_b = 0.f;
  if (tid < BN && n_blk + tid < a.N && a.bias) const_b = a.bias[n_blk + tid];
  __syncthreads();
  const int wm = wave >> 1, wn = wave & 1;
  const int frow = lane & 31, hi = lane >> 5, fsw = (frow >> 1) & 7;
  floatx16 acc[2][1];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 3; ++ks) {
    const int koff = ((2 * ks + hi) ^ fsw) * 16;
    const half8 wf = *reinterpret_cast<const half8*>(Ws + (wn * 32 + frow) * ROWB + koff);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const half8 xf = *reinterpret_cast<const half8*>(Xs + ((wm * 2 + i) * 32 + frow) * ROWB + koff);
      acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, xf, acc[i][0], 0, 0, 0);
    }
  }
  const float ln0[2] = {0.f, 0.f};
  tile_epilogue<BM, BN, 2, 2, 2, 1, false>(a, acc, ln0, ln0, smem, sconst, const_b, 0.f, 0.f, m_blk, n_blk, wave, 0, false);
}

// ---- N <= 8 output channels (conv_out 320->4): one wavefront per output pixel ----
template <int NMAX>
__global__ __launch_bounds__(256) void conv_small_n_kernel(IgemmArgs a, float* out_nchw) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= a.M) return;
  const int b = m / a.HoWo;
  const int rem = m - b * a.HoWo;
  const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
  const int Hup = a.Hi * a.up, Wup = a.Wi * a.up, upshift = a.up >> 1;
  float acc[NMAX];
#pragma unroll
  for (int n = 0; n < NMAX; ++n) acc[n] = 0.f;
  const int chunks = a.Ctot >> 3;
  for (int tap = 0; tap < a.ksize * a.ksize; ++tap) {
    const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
    const int iy = oy * a.stride - a.pad + ky, ix = ox * a.stride - a.pad + kx;
    if (iy < 0 || iy >= Hup || ix < 0 || ix >= Wup) continue;   // wave-uniform
    const size_t pix = (size_t)b * a.Hi * a.Wi + (size_t)(iy >> upshift) * a.Wi + (ix >> upshift);
    for (int ch = lane; ch < chunks; ch += 64) {
      const int c = ch * 8;
      half8 xv = (c < a.C0) ? *reinterpret_cast<const half8*>(a.x0 + pix * a.C0 + c)
                            : *reinterpret_cast<const half8*>(a.x1 + pix * a.C1 + (c - a.C0));
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        if (n < a.N) {
          half8 wv = *reinterpret_cast<const half8*>(a.w + (size_t)n * a.K + (size_t)tap * a.Ctot + c);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[n] += (float)xv[e] * (float)wv[e];
        }
      }
    }
  }
#pragma unroll
  for (int n = 0; n < NMAX; ++n) {
    float v = acc[n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    acc[n] = v;
  }
  if (lane == 0) {
    for (int n = 0; n < a.N; ++n) {
      float v = acc[n] + (a.bias ? a.bias[n] : 0.f);
      if (out_nchw)
        out_nchw[((size_t)b * a.N + n) * a.HoWo + rem] = v;
      else
        a.out[(size_t)m * a.N + n] = (half_t)v;
    }
  }
}

// ---- N <= 4 output channels, 3x3 / stride 1 (the UNet's conv_out 320 -> 4, the VAE decoder's 128 -> 3): FOUR pixels of a row per
// lane group (round 5).  The one-wave-per-pixel kernel above walks its nine taps as nine dependent load -> FMA rounds (32 us for
// 8192 pixels: pure latency); here a group of LPC lanes (one per 8-channel chunk) requests the 3 x 6 input patch of four
// neighbouring pixels and the 9 x N weight chunks up front - 18 + 9 N independent 16-byte loads in flight per lane -, multiplies
// with v_dot2_f32_f16 and folds the LPC partial sums by butterfly.  64 / LPC groups per wave (C = 128: four groups of 16 lanes).
template <int LPC>
__global__ __launch_bounds__(256) void conv3x3_small_n_rows_kernel(IgemmArgs a, float* out_nchw) {
  constexpr int PG = 64 / LPC, PX = 4, NMAX = 4;
  const int lane = threadIdx.x & 63;
  const int sub = lane / LPC, cl = lane % LPC;
  const int gpr = a.Wo / PX;                                   // pixel groups per row
  const int total = a.B * a.Ho * gpr;
  const int g = (blockIdx.x * 4 + (threadIdx.x >> 6)) * PG + sub;
  const bool live = g < total && cl < (a.Ctot >> 3);
  const int gg = g < total ? g : total - 1;
  const int row = gg / gpr, gx = gg - row * gpr;
  const int b = row / a.Ho, oy = row - b * a.Ho, ox0 = gx * PX;
  const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  half8 xv[3][PX + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int iy = oy - 1 + r;
#pragma unroll
    for (int c = 0; c < PX + 2; ++c) {
      const int ix = ox0 - 1 + c;
      const bool ok = live && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
      xv[r][c] = ok ? *reinterpret_cast<const half8*>(a.x0 + (((size_t)b * a.Hi + iy) * a.Wi + ix) * a.C0 + cl * 8) : z;
    }
  }
  half8 wv[NMAX][9];
#pragma unroll
  for (int n = 0; n < NMAX; ++n)
#pragma unroll
    for (int t = 0; t < 9; ++t)
      wv[n][t] = (live && n < a.N) ? *reinterpret_cast<const half8*>(a.w + (size_t)n * a.K + (size_t)t * a.Ctot + cl * 8) : z;
  float acc[NMAX][PX];
#pragma unroll
  for (int n = 0; n < NMAX; ++n)
#pragma unroll
    for (int px = 0; px < PX; ++px) acc[n][px] = 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
      for (int px = 0; px < PX; ++px)
#pragma unroll
        for (int n = 0; n < NMAX; ++n)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const half2v x2 = {xv[r][px + kx][2 * e], xv[r][px + kx][2 * e + 1]};
            const half2v w2 = {wv[n][r * 3 + kx][2 * e], wv[n][r * 3 + kx][2 * e + 1]};
            acc[n][px] = __builtin_amdgcn_fdot2(x2, w2, acc[n][px], false);
          }
#pragma unroll
  for (int n = 0; n < NMAX; ++n)
#pragma unroll
    for (int px = 0; px < PX; ++px) {
      float v = acc[n][px];
#pragma unroll
      for (int o = LPC / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
      acc[n][px] = v;
    }
  // lanes 0-15 of the group store one (channel, pixel) each
  const int sel = cl & 15;
  float v = 0.f;
#pragma unroll
  for (int n = 0; n < NMAX; ++n)
#pragma unroll
    for (int px = 0; px < PX; ++px) v = (sel == n * PX + px) ? acc[n][px] : v;
  const int n = sel >> 2, px = sel & 3;
  if (g < total && cl < 16 && n < a.N) {
    v += a.bias ? a.bias[n] : 0.f;
    const int rem = oy * a.Wo + ox0 + px;
    if (out_nchw)
      out_nchw[((size_t)b * a.N + n) * a.HoWo + rem] = v;
    else
      a.out[((size_t)b * a.HoWo + rem) * a.N + n] = (half_t)v;
  }
}

}  // namespace

int launch_conv_generic(const ConvDesc& d, int act_silu_out, hipStream_t s) {
  IgemmArgs a = make_args(d);
  if (a.ksize == 3 && a.stride == 1 && a.up == 1 && a.Ctot == 4 && !d.x1 && d.pad < 0 && d.out_mode == kOutHalf && a.N % 8 == 0 &&
      !d.temb && !act_silu_out) {
    // (+ room for the GroupNorm statistics scratch of the shared tile epilogue behind the staged 128 x 64 tile)
    const size_t lds = std::max((size_t)(128 + 64) * BK * 2 + 2 * 64 * sizeof(float),
                                (size_t)128 * (64 + 8) * 2 + 16 + (kGnScratchFloats + 2 * 64) * sizeof(float));
    a.splitk = 1;
    const int gn_entries = setup_gn_stats(d, a, 128);
    hipLaunchKernelGGL(conv3x3_cin4_kernel, dim3(cdiv(a.M, 128) * cdiv(a.N, 64)), dim3(256), lds, s, a);
    SD_HIP(hipGetLastError());
    return gn_entries;
  }
  if (a.K <= SC_KMAX && d.out_mode == kOutHalf && a.N >= 64) {
    hipLaunchKernelGGL(conv_small_cin_kernel, dim3(cdiv(a.M, SC_PIX)), dim3(256), 0, s, a, act_silu_out);
    SD_HIP(hipGetLastError());
    return 0;
  }
  SD_REQUIRE(d.out_mode != kOutGeglu || d.N % 64 == 0, kUnsupported, "generic GEGLU needs N %% 64 == 0 (N=%d)", d.N);
  size_t total = (size_t)a.M * a.N;
  int blocks = (int)std::min<size_t>((total + 255) / 256, 65535);
  hipLaunchKernelGGL(conv_generic_kernel, dim3(blocks), dim3(256), 0, s, a, act_silu_out);
  SD_HIP(hipGetLastError());
  return 0;
}

void launch_conv_small_n(const ConvDesc& d, float* out_nchw_f32, hipStream_t s) {
  IgemmArgs a = make_args(d);
  SD_REQUIRE(a.N <= 8 && a.Ctot % 8 == 0 && a.C0 % 8 == 0, kInvalidArgument, "conv_small_n: N=%d Ctot=%d", a.N,
             a.Ctot);
  // 3x3 / stride 1 / N <= 4: four pixels of a row per lane group, every load in flight at once (conv3x3_small_n_rows_kernel);
  // SD_CONV_OUT_ROWS=0 (with SD_TUNE) keeps the one-wave-per-pixel kernel: A/B
  static const int rows_mode = tune_env_int("SD_CONV_OUT_ROWS", 1);
  const int chunks = a.Ctot / 8;
  const int lpc = chunks <= 16 ? 16 : (chunks <= 32 ? 32 : 64);
  if (rows_mode != 0 && a.ksize == 3 && a.stride == 1 && a.up == 1 && a.pad == 1 && !d.x1 && a.N <= 4 && chunks <= 64 &&
      a.Wo % 4 == 0 && a.Hi == a.Ho && a.Wi == a.Wo) {
    const int pg = 64 / lpc;
    const int groups = a.B * a.Ho * (a.Wo / 4);
    const dim3 grid(cdiv(cdiv(groups, pg), 4));
    if (lpc == 16) hipLaunchKernelGGL(conv3x3_small_n_rows_kernel<16>, grid, dim3(256), 0, s, a, out_nchw_f32);
    else if (lpc == 32) hipLaunchKernelGGL(conv3x3_small_n_rows_kernel<32>, grid, dim3(256), 0, s, a, out_nchw_f32);
    else hipLaunchKernelGGL(conv3x3_small_n_rows_kernel<64>, grid, dim3(256), 0, s, a, out_nchw_f32);
    SD_HIP(hipGetLastError());
    return;
  }
  hipLaunchKernelGGL(conv_small_n_kernel<8>, dim3(cdiv(a.M, 4)), dim3(256), 0, s, a, out_nchw_f32);
  SD_HIP(hipGetLastError());
}

}  // namespace sd
