// AutoencoderKL mid-block attention as one streaming kernel: out = softmax(Q K^T / sqrt(C)) V, one head, head dim D = C, any number of
// tokens S >= 1, the batch in the grid, no S x S buffer.
//
// Math (reference): diffusers' mid-block attention of AutoencoderKL, which the reference converts inside its VAE wrappers
// (python_coreml_stable_diffusion/torch2coreml.py:584-594 decoder, :739-749 encoder; Decoder.swift, Encoder.swift).
//
// The form is vit_attention_kernel's (vit.hip) at head dims up to 512.  One workgroup = (batch, 64 queries); its four waves own 16
// queries each.  Keys stream through LDS in tiles of 64:
//   Ks [key][d]  as loaded                   -> A operand of S^T = K Q^T   (v_mfma_f32_16x16x32_f16: 16 keys x 16 queries, k = d)
//   Vt [d][key]  transposed while stored     -> A operand of O^T = V^T P^T (16 d x 16 queries, k = key)
// Both products put the QUERY on the lane (column lane & 15): a lane's score registers, its running max / sum and its D / 4 output
// registers belong to one query.  A score block leaves the MFMA with keys 4 g + r (g = lane >> 4, r = register) in lane group g; two
// blocks side by side are the eight k-elements lane group g feeds the second MFMA with, and the V^T fragment is read in that same key
// order (two 8-byte LDS reads).  Per lane at D = 512: 128 fp32 output accumulators, 64 registers of Q fragments, 16 of scores; the K
// and V^T tiles take 65 KB + 72 KB of the 160 KB of LDS, single-buffered - one workgroup per CU.
// Numerics: fp32 running max / sum / output, exp2 with log2(e) / sqrt(C) folded into the logits in fp32, P rounded to fp16 only as the
// second MFMA's operand, one normalisation at the end.  The output is rescaled only in tiles where some query of the wave met a new
// maximum (a wave-uniform branch; multiplying by exp2(0) = 1 is exact, so skipping it changes no bit).
// Ragged S: rows past S are loaded as zeros (K, V, Q alike - every LDS element the products read is written every tile), keys past S
// get the finite score -1e30 and the probability 0 (a select, not an exponential), queries past S are computed on zeros and not stored.
#include "kernels.h"

namespace sd {
namespace {

constexpr int VA_TQ = 64, VA_TK = 64;
constexpr int VA_LDV = VA_TK + 8;   // V^T row stride in halves: 144 B, 16-B aligned, rows 36 banks apart

template <int D>
constexpr int va_ldk() { return D + 8; }   // K row stride in halves: 16-B aligned, rows 4 (D = 64: 36) banks apart
template <int D>
constexpr size_t va_lds_bytes() { return ((size_t)VA_TK * va_ldk<D>() + (size_t)D * VA_LDV) * sizeof(half_t); }

template <int D>
__global__ __launch_bounds__(256) void vae_attention_kernel(const half_t* __restrict__ q, const half_t* __restrict__ k,
                                                            const half_t* __restrict__ v, half_t* __restrict__ out, int S,
                                                            float scale_log2e) {
  constexpr int LDK = va_ldk<D>();
  constexpr int NKS = D / 32;   // k-steps of the first product
  constexpr int NDB = D / 16;   // 16-row output blocks of the second
  constexpr int NLD = D / 32 < 8 ? D / 32 : 8;   // 16-byte loads a thread keeps in flight while it fills a tile (D / 32 per tile)
  extern __shared__ __attribute__((aligned(16))) half_t va_lds[];
  half_t* Ks = va_lds;
  half_t* Vt = va_lds + VA_TK * LDK;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c = lane & 15, g = lane >> 4;
  const size_t base = (size_t)blockIdx.y * S * D;   // this image's rows
  const int qi = blockIdx.x * VA_TQ + wave * 16 + c;   // this lane's query

  half8 qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    qf[ks] = (half8)(half_t)0;
    if (qi < S) qf[ks] = *reinterpret_cast<const half8*>(q + base + (size_t)qi * D + 32 * ks + 8 * g);
  }
  floatx4 o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) o[db] = (floatx4)0.f;
  float m = -1e30f, l = 0.f;   // running max (log2 domain) of the query, this lane's share of its running sum

  const int ntiles = (S + VA_TK - 1) / VA_TK;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int k0 = kt * VA_TK;
    __syncthreads();   // the previous tile has been read
    for (int i0 = t; i0 < VA_TK * (D / 8); i0 += 256 * NLD) {   // K: D / 8 threads per key row, contiguous bytes; NLD loads in flight
      half8 x[NLD];
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        const int i = i0 + 256 * u, key = i / (D / 8), ch = (i % (D / 8)) * 8;
        x[u] = *reinterpret_cast<const half8*>(k + base + (size_t)min(k0 + key, S - 1) * D + ch);   // always in bounds: no branch
      }
      __builtin_amdgcn_sched_barrier(0);   // every load is issued before the first one is waited for
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        const int i = i0 + 256 * u, key = i / (D / 8), ch = (i % (D / 8)) * 8;
        *reinterpret_cast<half8*>(Ks + key * LDK + ch) = k0 + key < S ? x[u] : (half8)(half_t)0;
      }
    }
    for (int i0 = t; i0 < VA_TK * (D / 8); i0 += 256 * NLD) {   // V: a wave stores 64 consecutive keys of one d row (no bank conflict)
      half8 x[NLD];
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        const int i = i0 + 256 * u, key = i & 63, ch = (i >> 6) * 8;
        x[u] = *reinterpret_cast<const half8*>(v + base + (size_t)min(k0 + key, S - 1) * D + ch);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < NLD; ++u) {
        const int i = i0 + 256 * u, key = i & 63, ch = (i >> 6) * 8;
        const half8 y = k0 + key < S ? x[u] : (half8)(half_t)0;
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(ch + e) * VA_LDV + key] = y[e];
      }
    }
    __syncthreads();

    // s[kb][r]: key k0 + 16 kb + 4 g + r against query c
    floatx4 s[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) s[kb] = (floatx4)0.f;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const half8 a = *reinterpret_cast<const half8*>(Ks + (16 * kb + c) * LDK + 32 * ks + 8 * g);
        s[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[ks], s[kb], 0, 0, 0);
      }
    float mx = m;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool valid = k0 + 16 * kb + 4 * g + r < S;
        s[kb][r] = valid ? s[kb][r] * scale_log2e : -1e30f;
        mx = fmaxf(mx, s[kb][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));   // key k0 is valid in every tile: mx is a real score from the first tile on
    if (__any(mx > m)) {                  // some query of this wave has a new maximum
      const float alpha = exp2f(m - mx);  // first tile: exp2(-1e30 - mx) = 0 exactly, on l = 0 and o = 0
      l *= alpha;
#pragma unroll
      for (int db = 0; db < NDB; ++db) o[db] *= alpha;
    }
    m = mx;
    half4 p[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool valid = k0 + 16 * kb + 4 * g + r < S;
        const float e = valid ? exp2f(s[kb][r] - mx) : 0.f;
        l += e;
        p[kb][r] = (half_t)e;
      }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      half8 pb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pb[j] = p[2 * ks][j];
        pb[4 + j] = p[2 * ks + 1][j];
      }
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const half_t* row = Vt + (16 * db + c) * VA_LDV + 32 * ks + 4 * g;
        const half4 lo = *reinterpret_cast<const half4*>(row), hi = *reinterpret_cast<const half4*>(row + 16);
        half8 a;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = lo[j];
          a[4 + j] = hi[j];
        }
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb, o[db], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qi < S) {
    const float inv = 1.0f / l;   // l >= 1: the key that holds the maximum contributes exp2(0)
    half_t* dst = out + base + (size_t)qi * D + 4 * g;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {   // o[db][r] = O[query c][d = 16 db + 4 g + r]
      half4 y;
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = (half_t)(o[db][r] * inv);
      *reinterpret_cast<half4*>(dst + 16 * db) = y;
    }
  }
}

template <int D>
void launch_d(const half_t* q, const half_t* k, const half_t* v, half_t* out, int B, int S, float scale_log2e, hipStream_t s) {
  static DynLdsOnce once;   // 137 KB at D = 512: above the 64 KB a kernel gets without asking
  once.set(vae_attention_kernel<D>, va_lds_bytes<D>());
  hipLaunchKernelGGL(vae_attention_kernel<D>, dim3(cdiv(S, VA_TQ), B), dim3(256), va_lds_bytes<D>(), s, q, k, v, out, S, scale_log2e);
}

}  // namespace

bool vae_attention_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

void launch_vae_attention(const half_t* q, const half_t* k, const half_t* v, half_t* out, int B, int S, int C, hipStream_t s) {
  SD_REQUIRE(vae_attention_ok(C), kUnsupported, "vae_attention: head dim %d (the kernel is built for 64, 128, 256 and 512)", C);
  SD_REQUIRE(B >= 1 && B <= 65535 && S >= 1, kInvalidArgument, "vae_attention: B=%d S=%d", B, S);
  const float scale_log2e = 1.4426950408889634f / sqrtf((float)C);
  switch (C) {
    case 64: launch_d<64>(q, k, v, out, B, S, scale_log2e, s); break;
    case 128: launch_d<128>(q, k, v, out, B, S, scale_log2e, s); break;
    case 256: launch_d<256>(q, k, v, out, B, S, scale_log2e, s); break;
    default: launch_d<512>(q, k, v, out, B, S, scale_log2e, s); break;
  }
  SD_HIP(hipGetLastError());
}

}  // namespace sd
