// K8/K9 and boundary helpers: timestep sinusoid, weight-streaming GEMV for the time-embedding
// MLPs, layout conversions at the 4-channel model boundary, and the device-resident
// classifier-free-guidance + scheduler step (pipeline.py:500-573 without host round trips).
#include <cmath>
#include <cstdint>

#include "kernels.h"

namespace sd {
namespace {

// unet.py:703-728: freq_i = exp(-ln(10000) * i / (half - freq_shift)); arg = float32(t) * freq_i;
// [sin | cos] flipped to [cos | sin] (flip_sin_to_cos=True).  fp32 throughout (unet.py:719).  The
// frequency table is computed on the host (correctly rounded float32 of the double value) so the
// argument t*freq matches the reference's torch.exp table to the last bit wherever torch's own
// float32 exp is correctly rounded.
__global__ void timestep_embedding_kernel(const float* __restrict__ t, const float* __restrict__ freq,
                                          float* __restrict__ out, int n, int dim) {
  const int half = dim / 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * half) return;
  const int row = idx / half, i = idx - row * half;
  const float arg = t[row] * freq[i];
  out[(size_t)row * dim + i] = cosf(arg);
  out[(size_t)row * dim + half + i] = sinf(arg);
}

__device__ __forceinline__ float silu_f(float v) {   // v * sigmoid(v) on the native exp2 / rcp units
  return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
}

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
// sum over the 64 lanes, result in every lane: 4 DPP steps inside each 16-lane row, then the
// gfx950 v_permlane16_swap / v_permlane32_swap exchanges across rows and wave halves
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  const unsigned u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const unsigned r0 = r[0], r1 = r[1];   // scalars first (bit-casting a vector-element lvalue reads lane 0 twice)
  v = __uint_as_float(r0) + __uint_as_float(r1);
  const unsigned u2 = __float_as_uint(v);
  const auto q = __builtin_amdgcn_permlane32_swap(u2, u2, false, false);
  const unsigned q0 = q[0], q1 = q[1];
  return __uint_as_float(q0) + __uint_as_float(q1);
}

// out[b][n] (+)= act_out( sum_k W[n][k] * act_in(x[b][k]) + bias[n] ), B <= BMAX rows of x.
// Weight-streaming (HBM-bound, M <= 8: an LDS round trip would be pure overhead).  Each wavefront owns
// ROWS output rows: ALL of its weight rows are requested up front (ROWS x KITERS 16-B loads in flight
// per lane - one exposed HBM round trip per wave), its slice of x arrives by unconditional 16-B loads
// (row / column indices clamped, out-of-range values zeroed by select - a per-element branchy load
// costs a dependent memory round trip each) with the optional SiLU applied once, then one wave
// reduction per (row, batch) pair.
template <int BMAX, int GEMV_KITERS, int ROWS>   // K <= 64 lanes * 8 halves * GEMV_KITERS, K % 8 == 0
__global__ __launch_bounds__(256) void gemv_kernel(const half_t* __restrict__ w, const float* __restrict__ bias,
                                                   const float* __restrict__ x, int ldx, float* __restrict__ out,
                                                   int ldo, int B, int N, int K, int silu_in, int silu_out,
                                                   int accumulate) {
  const int lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS;
  if (n0 >= N) return;
  half8 wv[ROWS][GEMV_KITERS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const half_t* wr = w + (size_t)min(n0 + r, N - 1) * K;   // clamped rows are computed and dropped
#pragma unroll
    for (int i = 0; i < GEMV_KITERS; ++i) {
      const int k = (lane + 64 * i) * 8;
      wv[r][i] = *reinterpret_cast<const half8*>(wr + min(k, K - 8));
    }
  }
  float xr[BMAX][GEMV_KITERS][8];
#pragma unroll
  for (int b = 0; b < BMAX; ++b) {
    const float* xb = x + (size_t)min(b, B - 1) * ldx;
#pragma unroll
    for (int i = 0; i < GEMV_KITERS; ++i) {
      const int k = (lane + 64 * i) * 8;
      const bool in = k < K;                      // out-of-range chunks contribute x = 0
      const floatx4 lo = *reinterpret_cast<const floatx4*>(xb + min(k, K - 8));
      const floatx4 hi = *reinterpret_cast<const floatx4*>(xb + min(k, K - 8) + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = e < 4 ? lo[e] : hi[e - 4];
        if (silu_in) v = silu_f(v);
        xr[b][i][e] = in ? v : 0.f;
      }
    }
  }
  float acc[ROWS][BMAX];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int b = 0; b < BMAX; ++b) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < GEMV_KITERS; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf((float)wv[r][i][e], xr[b][i][e], s);
      acc[r][b] = s;
    }
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int b = 0; b < BMAX; ++b) acc[r][b] = wave_sum(acc[r][b]);
  // every lane now holds every sum: lane r*BMAX+b keeps result (r, b) and runs the one epilogue
  float mine = 0.f;
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int b = 0; b < BMAX; ++b) mine = (lane == r * BMAX + b) ? acc[r][b] : mine;
  const int n = n0 + lane / BMAX, b = lane % BMAX;
  if (lane < ROWS * BMAX && n < N && b < B) {
    float v = mine + (bias ? bias[n] : 0.f);
    if (silu_out) v = silu_f(v);
    float* dst = out + (size_t)b * ldo + n;
    *dst = accumulate ? (*dst + v) : v;
  }
}

__global__ void nchw_to_nhwc_kernel(const void* __restrict__ src, int src_is_f32, half_t* __restrict__ dst, int B,
                                    int C, int HW) {
  const size_t total = (size_t)B * C * HW;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const size_t bp = idx / C;
    const int p = (int)(bp % HW);
    const int b = (int)(bp / HW);
    const size_t s = ((size_t)b * C + c) * HW + p;
    dst[idx] = src_is_f32 ? (half_t) reinterpret_cast<const float*>(src)[s] : reinterpret_cast<const half_t*>(src)[s];
  }
}

__global__ void nhwc_to_nchw_f32_kernel(const half_t* __restrict__ src, float* __restrict__ dst, int B, int C, int HW) {
  const size_t total = (size_t)B * C * HW;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int p = (int)(idx % HW);
    const size_t bc = idx / HW;
    const int c = (int)(bc % C);
    const int b = (int)(bc / C);
    dst[idx] = (float)src[((size_t)b * HW + p) * C + c];
  }
}

__global__ void half_to_float_kernel(const half_t* __restrict__ s, float* __restrict__ d, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    d[i] = (float)s[i];
}
__global__ void float_to_half_kernel(const float* __restrict__ s, half_t* __restrict__ d, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    d[i] = (half_t)s[i];
}
__global__ void add_half_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, half_t* __restrict__ y,
                                size_t n8) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const half8 x = reinterpret_cast<const half8*>(a)[i], z = reinterpret_cast<const half8*>(b)[i];
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)x[e] + (float)z[e]);
    reinterpret_cast<half8*>(y)[i] = o;
  }
}
// y = a + r0 (+ r1 + r2): ControlNet residual hand-off (unet.py:1009-1022) with the multi-ControlNet sum
// of pipeline.py:269-282 folded in; fp32 accumulation, one fp16 rounding
struct SumSrc {
  const half_t* p[4];
};
__global__ void sum_half_kernel(SumSrc src, int nsrc, half_t* __restrict__ y, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    float acc[8];
    const half8 x = reinterpret_cast<const half8*>(src.p[0])[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (float)x[e];
    for (int k = 1; k < nsrc; ++k) {
      const half8 z = reinterpret_cast<const half8*>(src.p[k])[i];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += (float)z[e];
    }
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)acc[e];
    reinterpret_cast<half8*>(y)[i] = o;
  }
}
// (B, C, 1, S) -> [B][S][C]
__global__ void bc1s_to_tokens_kernel(const half_t* __restrict__ src, half_t* __restrict__ dst, int B, int C, int S) {
  const size_t total = (size_t)B * C * S;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const size_t bs = idx / C;
    const int s = (int)(bs % S);
    const int b = (int)(bs / S);
    dst[idx] = src[((size_t)b * C + c) * S + s];
  }
}

// pipeline.py:502-511: duplicate the latents for CFG, cast to fp16, timestep [t, t]
__global__ void loop_prep_kernel(const float* __restrict__ latents, half_t* __restrict__ sample,
                                 float* __restrict__ tbuf, LoopTables t, int Bimg, int C, int HW, int cfg) {
  const int step = *t.step;
  const size_t per = (size_t)C * HW;
  const size_t total = (size_t)Bimg * per;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const size_t bp = idx / C;
    const int p = (int)(bp % HW);
    const int b = (int)(bp / HW);
    // scheduler.scale_model_input (:504-505; identity for DDIM / PNDM / DPM-Solver++), then the fp16 cast at
    // the UNet boundary (:532)
    const half_t v = (half_t)(latents[((size_t)b * C + c) * HW + p] * (t.in_scale ? t.in_scale[step] : 1.0f));
    for (int r = 0; r < cfg; ++r) sample[((size_t)(r * Bimg + b) * HW + p) * C + c] = v;   // [uncond..., cond...]
  }
  if (blockIdx.x == 0 && threadIdx.x < cfg * Bimg) tbuf[threadIdx.x] = t.timesteps[step];
  if (t.temb_tab) {   // this step's time_emb_proj rows (unet.py:703-728 + :454-456 for every resnet), computed before the loop
    const size_t rowsz = (size_t)t.temb_ld, blk = (size_t)t.temb_rows * rowsz;
    const float* src = t.temb_tab + (size_t)step * blk;
    const size_t n4 = (size_t)t.temb_rows * (t.temb_n / 4);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
      const size_t r = i / (t.temb_n / 4), c = i - r * (t.temb_n / 4);
      reinterpret_cast<floatx4*>(t.temb_dst + r * rowsz)[c] = reinterpret_cast<const floatx4*>(src + r * rowsz)[c];
    }
  }
}

// pipeline.py:539, 561-569.  noise_pred fp32 NCHW [cfg*Bimg][CHW]; rows [0,Bimg) uncond, [Bimg,2Bimg) text.
// Generic linear-multistep update on the device (DDIM / PLMS / DPM-Solver++ 2M are all instances):
//   eps = u + g*(c-u);  m = a*x + b*eps;  x <- cx*x + cm*m + sum_j ch[j]*hist[j] [+ noise_tab[step]];  hist <- [m, hist[0..]]
// coef row: [cx, cm, ch0, ch1, ch2, a, b, flags]; flags != 0: m is NOT pushed into the history (the second
// evaluation of the PLMS warm-up, Scheduler.swift:228-236).  The workgroup that arrives last at the ticket
// advances the device step counter (every workgroup read it before arriving), so the step needs no second
// launch; the ticket only orders that one store, the arithmetic stays atomics-free and deterministic.
// De-noised tap (t.denoised != null; the previews of StableDiffusionPipeline.swift:332-349): one more linear form of the same x,
// eps and history, stored to its own buffer from inside a run-time branch - the update's own expressions are untouched, so the
// latents, the history and the step counter come out bit for bit as without it.
__global__ __launch_bounds__(256) void cfg_sched_step_kernel(const float* __restrict__ noise_pred,
                                                              float* __restrict__ latents, float* __restrict__ eps_hist,
                                                              LoopTables t, float guidance, int Bimg, int CHW, int cfg,
                                                              int hist) {
  const int step = *t.step;
  const float* cf = t.coef + (size_t)step * 8;
  const float cx = cf[0], cm = cf[1], ma = cf[5], mb = cf[6];
  const bool push = cf[7] == 0.f;
  const size_t total = (size_t)Bimg * CHW;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    float eps = noise_pred[idx];
    if (cfg == 2) {
      const float c = noise_pred[total + idx];
      eps = eps + guidance * (c - eps);
    }
    const float x0 = latents[idx];
    if (t.denoised) {   // reads the history before this step's push below; every lane touches its own idx only
      const float* pr = t.pred + (size_t)step * 8;
      // spelled the way m below is contracted (one product rounded, then one fma): where the row is m's own (a, b) - DPM-Solver++ -
      // the estimate is m bit for bit (tests/test_progress_gpu.py holds the two together)
      float d = fmaf(pr[0], x0, pr[1] * eps);
      for (int j = 0; j < hist; ++j) d = fmaf(pr[2 + j], eps_hist[(size_t)j * total + idx], d);
      t.denoised[idx] = d;
    }
    const float m = ma * x0 + mb * eps;
    float x = cx * x0 + cm * m;
    // history slot j holds the converted model output of j+1 pushes ago
    for (int j = hist - 1; j >= 0; --j) {
      const float old = eps_hist[(size_t)j * total + idx];
      x += cf[2 + j] * old;
      if (push && j + 1 < hist) eps_hist[(size_t)(j + 1) * total + idx] = old;
    }
    if (push && hist > 0) eps_hist[idx] = m;
    if (t.noise_tab) x += t.noise_tab[(size_t)step * total + idx];   // ancestral step: + sigma_up * fresh noise
    latents[idx] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned arrived = __hip_atomic_fetch_add(t.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived == gridDim.x - 1) {
      *t.ticket = 0;
      *t.step = step + 1;
    }
  }
}

// Image-to-image start: the posterior sample of the VAE encoder's moments (Encoder.swift:68-77: logvar clamped to [-30, 20],
// std = exp(0.5 * logvar)), the scale factor (:78-89) and the scheduler's addNoise (Scheduler.swift:83-102) in one pass.  The
// arithmetic is spelled out in fmaf / products so that the vector and the scalar form round alike: std * eps + mean in one
// rounding, times scale, then sa * z + (sb * noise).  expf is the accurate library function (the std spans e^-15 .. e^10).
__device__ __forceinline__ float posterior_latent(float mean, float logvar, float eps, float scale) {
  const float lv = fminf(fmaxf(logvar, -30.0f), 20.0f);
  return fmaf(expf(0.5f * lv), eps, mean) * scale;
}
// moments [mean (n) | logvar (n)], eps (n), noise / out (n_images, n).  VEC: n % 4 == 0 and every pointer 16-byte aligned - one
// 16-byte load / store per lane and tensor; else one float per lane (any n, any alignment).  Grid-stride: any grid is in bounds.
template <bool VEC>
__global__ __launch_bounds__(256) void posterior_noise_kernel(const float* __restrict__ moments, const float* __restrict__ eps,
                                                               const float* __restrict__ noise, float* __restrict__ out, size_t n,
                                                               int n_images, float scale, float sa, float sb) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  if (VEC) {
    const size_t n4 = n / 4;
    const floatx4* mean4 = reinterpret_cast<const floatx4*>(moments);
    const floatx4* logvar4 = reinterpret_cast<const floatx4*>(moments + n);
    const floatx4* eps4 = reinterpret_cast<const floatx4*>(eps);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
      const floatx4 m = mean4[i], lv = logvar4[i], e = eps4[i];
      floatx4 z;
#pragma unroll
      for (int k = 0; k < 4; ++k) z[k] = posterior_latent(m[k], lv[k], e[k], scale);
      for (int b = 0; b < n_images; ++b) {
        const floatx4 nz = reinterpret_cast<const floatx4*>(noise + (size_t)b * n)[i];
        floatx4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fmaf(sa, z[k], sb * nz[k]);
        reinterpret_cast<floatx4*>(out + (size_t)b * n)[i] = o;
      }
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const float z = posterior_latent(moments[i], moments[n + i], eps[i], scale);
      for (int b = 0; b < n_images; ++b) out[(size_t)b * n + i] = fmaf(sa, z, sb * noise[(size_t)b * n + i]);
    }
  }
}

inline int grid_for(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 2048); }

}  // namespace

std::vector<float> timestep_freq_table(int dim, float freq_shift) {
  const int half = dim / 2;
  std::vector<float> f(half);
  for (int i = 0; i < half; ++i) {
    const float exponent = (-9.210340371976184f * (float)i) / ((float)half - freq_shift);   // fp32 like torch
    f[i] = (float)std::exp((double)exponent);
  }
  return f;
}

void launch_timestep_embedding(const float* t, const float* freq, float* out, int n, int dim, hipStream_t s) {
  const int total = n * (dim / 2);
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, t, freq, out, n, dim);
  SD_HIP(hipGetLastError());
}

void launch_gemv(const half_t* w, const float* bias, const float* x, int ldx, float* out, int ldo, int B, int N,
                 int K, int silu_in, int silu_out, int accumulate, hipStream_t s) {
  SD_REQUIRE(K % 8 == 0 && K <= 64 * 8 * 6, kUnsupported, "gemv: K=%d must be a multiple of 8 and <= 3072", K);
  // up to 4 x-rows per pass (register footprint); the CFG batch of 2 gets its own instantiation
  for (int b0 = 0; b0 < B; b0 += 4) {
    const int nb = std::min(4, B - b0);
    const float* xp = x + (size_t)b0 * ldx;
    float* op = out + (size_t)b0 * ldo;
    if (K <= 64 * 8 * 3) {   // 8 rows x 3 chunks = 96 weight VGPRs in flight
      if (nb <= 2)
        hipLaunchKernelGGL((gemv_kernel<2, 3, 8>), dim3(cdiv(N, 4 * 8)), dim3(256), 0, s, w, bias, xp, ldx, op, ldo, nb, N, K,
                           silu_in, silu_out, accumulate);
      else
        hipLaunchKernelGGL((gemv_kernel<4, 3, 8>), dim3(cdiv(N, 4 * 8)), dim3(256), 0, s, w, bias, xp, ldx, op, ldo, nb, N, K,
                           silu_in, silu_out, accumulate);
    } else {
      hipLaunchKernelGGL((gemv_kernel<4, 6, 4>), dim3(cdiv(N, 4 * 4)), dim3(256), 0, s, w, bias, xp, ldx, op, ldo, nb, N, K,
                         silu_in, silu_out, accumulate);
    }
  }
  SD_HIP(hipGetLastError());
}

void launch_nchw_to_nhwc(const void* src, int src_is_f32, half_t* dst, int B, int C, int H, int W, hipStream_t s) {
  const size_t n = (size_t)B * C * H * W;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, src_is_f32, dst, B, C, H * W);
  SD_HIP(hipGetLastError());
}
void launch_nhwc_to_nchw_f32(const half_t* src, float* dst, int B, int C, int H, int W, hipStream_t s) {
  const size_t n = (size_t)B * C * H * W;
  hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, dst, B, C, H * W);
  SD_HIP(hipGetLastError());
}
void launch_half_to_float(const half_t* src, float* dst, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(half_to_float_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, dst, n);
  SD_HIP(hipGetLastError());
}
void launch_float_to_half(const float* src, half_t* dst, size_t n, hipStream_t s) {
  hipLaunchKernelGGL(float_to_half_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, dst, n);
  SD_HIP(hipGetLastError());
}
void launch_add_half(const half_t* a, const half_t* b, half_t* y, size_t n, hipStream_t s) {
  SD_REQUIRE(n % 8 == 0, kInvalidArgument, "add_half: n %% 8 != 0");
  hipLaunchKernelGGL(add_half_kernel, dim3(grid_for(n / 8)), dim3(256), 0, s, a, b, y, n / 8);
  SD_HIP(hipGetLastError());
}
void launch_sum_half(const half_t* const* srcs, int nsrc, half_t* y, size_t n, hipStream_t s) {
  SD_REQUIRE(n % 8 == 0 && nsrc >= 1 && nsrc <= 4, kInvalidArgument, "sum_half: n %% 8 != 0 or %d sources", nsrc);
  SumSrc src{};
  for (int i = 0; i < nsrc; ++i) src.p[i] = srcs[i];
  hipLaunchKernelGGL(sum_half_kernel, dim3(grid_for(n / 8)), dim3(256), 0, s, src, nsrc, y, n / 8);
  SD_HIP(hipGetLastError());
}
void launch_bc1s_to_tokens(const half_t* src, half_t* dst, int B, int C, int S, hipStream_t s) {
  const size_t n = (size_t)B * C * S;
  hipLaunchKernelGGL(bc1s_to_tokens_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, dst, B, C, S);
  SD_HIP(hipGetLastError());
}

void launch_loop_prep(const float* latents, half_t* sample, float* tbuf, LoopTables t, int Bimg, int C, int H, int W,
                      int cfg, hipStream_t s) {
  const size_t n = (size_t)Bimg * C * H * W;
  hipLaunchKernelGGL(loop_prep_kernel, dim3(grid_for(n)), dim3(256), 0, s, latents, sample, tbuf, t, Bimg, C, H * W,
                     cfg);
  SD_HIP(hipGetLastError());
}

void launch_cfg_sched_step(const float* noise_pred, float* latents, float* eps_hist, LoopTables t, float guidance,
                           int Bimg, int CHW, int cfg, int hist, hipStream_t s) {
  const size_t n = (size_t)Bimg * CHW;
  hipLaunchKernelGGL(cfg_sched_step_kernel, dim3(std::min(grid_for(n), 64)), dim3(256), 0, s, noise_pred, latents,
                     eps_hist, t, guidance, Bimg, CHW, cfg, hist);
  SD_HIP(hipGetLastError());
}

void launch_posterior_noise(const float* moments, const float* eps, const float* noise, float* out, size_t n, int n_images,
                            float scale, float sa, float sb, hipStream_t s) {
  SD_REQUIRE(n >= 1 && n_images >= 1, kInvalidArgument, "posterior_noise: %zu elements x %d images", n, n_images);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(moments) | reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(noise) |
                         reinterpret_cast<uintptr_t>(out);
  if (n % 4 == 0 && bits % 16 == 0)
    hipLaunchKernelGGL(posterior_noise_kernel<true>, dim3(grid_for(n / 4)), dim3(256), 0, s, moments, eps, noise, out, n, n_images,
                       scale, sa, sb);
  else
    hipLaunchKernelGGL(posterior_noise_kernel<false>, dim3(grid_for(n)), dim3(256), 0, s, moments, eps, noise, out, n, n_images,
                       scale, sa, sb);
  SD_HIP(hipGetLastError());
}

// Debug (SD_POISON_LDS=1 with SD_TUNE): fill the LDS of every CU with NaN bit patterns before a launch.  A kernel that reads LDS it
// never wrote behind a zero weight is right on benign leftovers and wrong on a fresh box (0 * NaN); with this in front of every
// launch the GPU suite finds such reads (round 6: conv_small_cin_kernel's patch columns beyond K).
__global__ __launch_bounds__(1024) void lds_poison_kernel(unsigned* sink) {
  extern __shared__ unsigned lds_words[];
  const int n = 160 * 1024 / 4;
  for (int i = threadIdx.x; i < n; i += blockDim.x) lds_words[i] = (i & 1) ? 0x7e007e00u : (0x7fc00000u ^ (unsigned)(threadIdx.x << 3));
  __syncthreads();
  unsigned acc = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc ^= lds_words[i];
  if (acc == 0x12345u) sink[0] = acc;   // (never true: keeps the stores)
}
void launch_lds_poison(hipStream_t s) {
  static unsigned* sink = [] {
    unsigned* p = nullptr;
    (void)hipMalloc(&p, 256);
    return p;
  }();
  static DynLdsOnce once;
  once.set(lds_poison_kernel, 160 * 1024);
  hipLaunchKernelGGL(lds_poison_kernel, dim3(512), dim3(1024), 160 * 1024, s, sink);
  SD_HIP(hipGetLastError());
}

// Debug scan (SD_NAN_TRACE): how many fp16 values of a buffer are Inf / NaN (exponent all ones).
__global__ void count_nonfinite_half_kernel(const unsigned short* __restrict__ p, size_t n, unsigned long long* __restrict__ out) {
  unsigned long long c = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    c += (p[i] & 0x7c00u) == 0x7c00u;
  if (c) atomicAdd(out, c);
}
void launch_count_nonfinite_half(const void* p, size_t bytes, unsigned long long* out, hipStream_t s) {
  hipLaunchKernelGGL(count_nonfinite_half_kernel, dim3(1024), dim3(256), 0, s, reinterpret_cast<const unsigned short*>(p), bytes / 2, out);
  SD_HIP(hipGetLastError());
}

// Activation calibration (W8A8, activation_quantization.py:141-203): max |x| over one or two fp16 tensors, folded into *slot - the bit
// pattern of a non-negative fp32, whose unsigned order is its numeric order, so the running maximum is one atomicMax per wave.  NaN
// elements are skipped (fmaxf keeps the other operand); +-inf gives +inf.  Grid-stride, eight halves per load where the size allows.
__global__ __launch_bounds__(256) void absmax_half_kernel(const half_t* __restrict__ x0, size_t n0, const half_t* __restrict__ x1, size_t n1,
                                                          unsigned* __restrict__ slot) {
  float m = 0.f;
  const size_t step = (size_t)gridDim.x * blockDim.x, t0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  for (int src = 0; src < 2; ++src) {
    const half_t* x = src ? x1 : x0;
    const size_t n = src ? n1 : n0, n8 = n / 8;
    if (!x) continue;
    for (size_t i = t0; i < n8; i += step) {
      const half8 v = *reinterpret_cast<const half8*>(x + i * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)v[e]));
    }
    for (size_t i = n8 * 8 + t0; i < n; i += step) m = fmaxf(m, fabsf((float)x[i]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(slot, __float_as_uint(m));
}
void launch_absmax_half(const half_t* x0, size_t n0, const half_t* x1, size_t n1, float* slot, hipStream_t s) {
  const size_t n = std::max(n0, x1 ? n1 : 0);
  const unsigned blocks = (unsigned)std::min<size_t>((n / 8 + 255) / 256 + 1, 256);
  hipLaunchKernelGGL(absmax_half_kernel, dim3(blocks), dim3(256), 0, s, x0, n0, x1, x1 ? n1 : 0, reinterpret_cast<unsigned*>(slot));
  SD_HIP(hipGetLastError());
}

}  // namespace sd
