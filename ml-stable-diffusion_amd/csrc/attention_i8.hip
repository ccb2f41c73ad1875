// W8A8 self-attention einsums (activation_quantization.py:205-215 collects every Einsum beside every Conv2d; unet.py:45-59 is the
// module): Q.K^T and P.V on the int8 MFMAs for the shapes attention8.hip runs in fp16 - head dim 64, S_q = S_k = S, S % 64 == 0.
// Symmetric, per tensor, the project's own scheme: parity with coremltools' quantizer is unpinned, as for every W8A8 layer here.
//
// THE FUNCTION (kernel and test oracle alike; r_q, r_k, r_v the three ranges of the einsum, s_x = fp32(r_x / 127)):
//   1. x_q = clip(rint(fp32(x) * fp32(127 / r_x)), -127, 127), NaN -> 0, +-inf -> +-127 (einsum_quantize_kernel below; a handle's
//      queries arrive multiplied by attention_q_prescale(d), so their factor is fp32(127 / (r_q * prescale)): r_q always means the
//      un-scaled q the reference's Einsum sees);
//   2. t[q][k] = fp32(int32 sum_c q_q k_q) * c, c = fp32(s_q * s_k * d^-0.5 * log2 e): ONE fp32 product per score, the sum exact;
//   3. m[q] = max_k t (the TRUE row max), p_q = rint(127 * exp2(t - m)) in 0 .. 127: the largest key of a row is exactly 127;
//   4. N[q][c] = int32 sum_k p_q v_q and L[q] = sum_k p_q, exact (127^2 S < 2^31 up to S = kAttnI8MaxS);
//   5. out = fp16(fp32(N) * (s_v / fp32(L))), every operation rounded to fp32 on its own.
// Everything after step 3 is a sum of integers: the result does not depend on the tile walk, the ring depth or the wave count, and
// the only inexact step is the hardware exp2.
//
// Why the true max and not attention8's streaming form: with a running max p_q would depend on where the max moved - on the
// schedule - so no oracle could state the function (and a balanced grid could not merge partial sums exactly).  The price is two
// passes over the keys: pass 1 runs the int8 Q.K^T MFMAs and an integer max (t is monotone in the int32 sum, c > 0: no exp, no
// conversion), pass 2 recomputes the scores.
// Why not the reference's literal "quantize the normalised softmax output over [0, 1]": at 4096 keys nearly every probability
// is below 1 / 254 and rounds to zero.  Quantizing relative to the row max never resolves worse than that scheme.
//
// The kernel, after attention8.hip:
//   * 8 or 4 waves per workgroup, 32 queries per wave, one workgroup per query tile (the classic grid only);
//   * key-major score tile (K.Q^T): a lane owns ONE query column, so max and sum run over registers and one half-wave exchange;
//     v_mfma_i32_32x32x32_i8 takes 32 channels per instruction: two per 32-key block, four per key tile (attention8: eight);
//   * P goes from the accumulator registers into the P.V MFMA as a packed-byte operand without touching LDS: register r of a
//     32-key block is key (r & 3) + 8 (r >> 2) + 4 hi, byte r of the operand is k-slot 16 hi + r, so V^T arrives with position p of
//     every 32 keys holding key (p & 3) + 8 ((p >> 2) & 3) + 4 (p >> 4) (AttnDesc::vt_perm == 2: attention_i8_vt_key; written by
//     einsum_quantize_kernel and the host packer sd_op_w8a8_pack_vt);
//   * L is a byte dot product of the packed P against ones (v_dot4_u32_u8);
//   * K and V^T tiles are 4 KiB each per 64 keys and go HBM -> LDS by LDS-DMA through a ring of D stages of 8 KiB behind ONE raw
//     s_barrier per step and counted vmcnt waits; the bank swizzle lives on the DMA's source address (physical 16-B chunk p of row r
//     holds logical chunk p ^ ((r >> 1) & 3)).  Pass 1 streams K only: a stage holds two K tiles.  Every LDS byte a wave reads was
//     written by a DMA of the same pass (a dead tile of an odd tile count is never read).
#include "kernels.h"
#include "quantize8.h"

#include <climits>
#include <cmath>
#include <cstdio>

// every fp32 operation of the function is rounded on its own: no product may fuse with the subtraction or the sum behind it
#pragma clang fp contract(off)

namespace sd {
namespace {

constexpr int KT = 64;                    // keys per tile
constexpr int HALF_BYTES = KT * 64;       // one int8 K (or V^T) tile: 64 rows x 64 B
constexpr int STAGE_BYTES = 2 * HALF_BYTES;

struct AttnI8Args {
  const int8_t* q;
  const int8_t* k;
  const int8_t* vt;
  half_t* out;
  int heads, S;
  int ldq, ldk, ldv, ldo;   // bytes / bytes / bytes / halves
  float c;                  // fp32(s_q * s_k * d^-0.5 * log2 e)
  float s_v;
  int q_tiles;
};

__device__ __forceinline__ void dma16(const __amdgpu_buffer_rsrc_t& rs, char* lds, unsigned voffset, int soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 16, voffset, soffset, 0, 0);
#endif
}
template <int N>
__device__ __forceinline__ void wait_vmcnt_barrier() {   // counted wait + raw barrier in one statement: no LDS access moves across
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}
__device__ __forceinline__ int xor32_imax(int v) {
  const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
  const unsigned r0 = r[0], r1 = r[1];
  return max((int)r0, (int)r1);
}
__device__ __forceinline__ unsigned xor32_usum(unsigned v) {
  const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  const unsigned r0 = r[0], r1 = r[1];
  return r0 + r1;
}

template <int WAVES, int D>
__global__ __launch_bounds__(WAVES * 64) void attn_i8_kernel(AttnI8Args a) {
  static_assert(WAVES == 4 || WAVES == 8, "4 or 8 waves");
  static_assert(D >= 3, "ring depth");
  constexpr int PPT = 8 / WAVES;             // LDS-DMA pieces (1 KiB = 16 rows) per wave per stage: pieces 0-3 the first half, 4-7 the second
  static_assert(PPT * (D - 2) <= 63, "vmcnt range");
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [D][K tile | V^T tile]  (pass 1: [D][K tile 2i | K tile 2i + 1])

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  int bid = blockIdx.x;
  {   // XCD-contiguous walk (attention8.hip): the query tiles of one (sample, head) share its K / V^T in one XCD's L2
    const int nwg = gridDim.x;
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = ((xcd < r8) ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  }
  const int nt = a.S / KT;
  const int qtile = bid % a.q_tiles, bh = bid / a.q_tiles;
  const int b = bh / a.heads, h = bh - b * a.heads;
  const int q = (qtile * WAVES + wave) * 32 + l31;
  const int8_t* qbase = a.q + (size_t)b * a.S * a.ldq + (size_t)h * 64;
  const int8_t* kbase = a.k + (size_t)b * a.S * a.ldk + (size_t)h * 64;
  const int8_t* vbase = a.vt + ((size_t)b * a.heads + h) * 64 * (size_t)a.ldv;

  // ---- Q fragments (B operand of K.Q^T): lane (query l31, half hi) holds channels 32 kk + 16 hi + 0..15 of MFMA step kk ----
  intx4 qf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const intx4 z = {0, 0, 0, 0};
    qf[kk] = (q < a.S) ? *reinterpret_cast<const intx4*>(qbase + (size_t)q * a.ldq + kk * 32 + hi * 16) : z;
  }

  // ---- LDS-DMA: loop-invariant per-lane byte offsets (K rows / V^T rows), scalar running offsets ----
  const unsigned k_bytes = (unsigned)((size_t)(a.S - 1) * a.ldk + 64);
  const unsigned v_bytes = (unsigned)((size_t)63 * a.ldv + a.S);
  unsigned voff_k[PPT], voff_v[PPT];
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int pp = (wave + i * WAVES) & 3;                   // piece = rows 16 pp .. 16 pp + 15 of its half
    const int r = 16 * pp + (lane >> 2);
    const int c = (lane & 3) ^ ((r >> 1) & 3);               // logical 16-B chunk this lane fetches (bank swizzle)
    voff_k[i] = (unsigned)(r * a.ldk + c * 16);
    voff_v[i] = (unsigned)(r * a.ldv + c * 16);
  }
  const int k_step = KT * a.ldk;                             // bytes between consecutive K tiles
  int it_stage = 0;
  // stage `idx` of pass 1 (two K tiles) or pass 2 (K tile | V^T tile); past the end: zero-sized resources (the counted waits stay
  // uniform, nothing is fetched)
  auto issue = [&](bool pass2, int idx) {
    char* st = smem + it_stage * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int piece = wave + i * WAVES;                    // wave-uniform
      const int hf = piece >> 2, pp = piece & 3;
      const int tile = pass2 ? idx : 2 * idx + hf;
      const bool live = tile < nt;
      const bool isv = pass2 && hf;
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(isv ? vbase : kbase), 0,
                                                                         (int)(live ? (isv ? v_bytes : k_bytes) : 0u), 0x00020000);
      dma16(rs, st + hf * HALF_BYTES + pp * 1024, isv ? voff_v[i] : voff_k[i], isv ? tile * KT : tile * k_step);
    }
    it_stage = (it_stage + 1 == D) ? 0 : it_stage + 1;
  };

  // ---- fragment addressing: row l31 (+ 32 per key block / channel tile), logical 16-B chunk x = 2 s + hi; the same offsets serve
  //      the K tile (s = MFMA step: 32 channels) and the permuted V^T tile (s = key block: 32 keys) ----
  const int fsw = (l31 >> 1) & 3;
  int foff[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) foff[s] = l31 * 64 + (((s * 2 + hi) ^ fsw) * 16);

  auto scores = [&](intx16 (&s)[2], const char* kt) {        // s[sub] = K.Q^T of the 32-key block sub
    intx4 kf[2][2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) kf[sub][kk] = *reinterpret_cast<const intx4*>(kt + foff[kk] + sub * 2048);
    intx16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) s[sub] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf[sub][0], qf[0], z, 0, 0, 0);
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) s[sub] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf[sub][1], qf[1], s[sub], 0, 0, 0);
  };

  // ================= pass 1: the true row max, in integers (K only: two tiles per stage) =================
  int imax = INT_MIN;
  {
    const int n1 = (nt + 1) >> 1;
#pragma unroll
    for (int p = 0; p < D - 1; ++p) {
      asm volatile("" ::: "memory");                         // keep the DMA issue order: the counted waits rely on it
      issue(false, p);
    }
    int st_cur = 0;
    for (int i = 0; i < n1; ++i) {
      // this wave's pieces of stage i have landed (loads of one wave return in order: the D - 2 younger stages may be outstanding);
      // behind the barrier every wave's have, and every wave is through stage i - 1, which the DMA issued next overwrites
      wait_vmcnt_barrier<PPT * (D - 2)>();
      issue(false, i + D - 1);
      const char* st = smem + st_cur * STAGE_BYTES;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        if (2 * i + hf < nt) {                               // (workgroup-uniform)
          intx16 s[2];
          scores(s, st + hf * HALF_BYTES);
#pragma unroll
          for (int r = 0; r < 16; ++r) imax = max(imax, max(s[0][r], s[1][r]));
        }
      }
      st_cur = (st_cur + 1 == D) ? 0 : st_cur + 1;
    }
    // every DMA of pass 1 done (the zero-sized tail ones too) and every wave through its last stage before pass 2 refills the ring
    wait_vmcnt_barrier<0>();
  }
  imax = xor32_imax(imax);                                   // the other half-wave holds the other 32 keys of every tile
  const float m = __fmul_rn((float)imax, a.c);               // == max_k t: t is monotone in the int32 sum

  // ================= pass 2: scores again, p_q, P.V and L =================
  intx16 oacc[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    oacc[0][r] = 0;
    oacc[1][r] = 0;
  }
  unsigned lsum = 0;
  {
    it_stage = 0;
#pragma unroll
    for (int p = 0; p < D - 1; ++p) {
      asm volatile("" ::: "memory");
      issue(true, p);
    }
    int st_cur = 0;
    for (int j = 0; j < nt; ++j) {
      wait_vmcnt_barrier<PPT * (D - 2)>();                   // K and V^T of tile j have landed for every wave; tile j - 1's stage is free
      issue(true, j + D - 1);
      const char* st = smem + st_cur * STAGE_BYTES;
      intx16 s[2];
      scores(s, st);
      intx4 vf[2][2];                                        // [sub][ct]
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) vf[sub][ct] = *reinterpret_cast<const intx4*>(st + HALF_BYTES + foff[sub] + ct * 2048);
      intx4 pf[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          unsigned pk = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float t = __fmul_rn((float)s[sub][4 * w + e], a.c);
            const float p = __builtin_rintf(__fmul_rn(127.f, __builtin_amdgcn_exp2f(__fsub_rn(t, m))));
            pk |= ((unsigned)(int)p) << (8 * e);             // 0 .. 127
          }
          pf[sub][w] = (int)pk;
          lsum = __builtin_amdgcn_udot4(pk, 0x01010101u, lsum, false);
        }
      }
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) oacc[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(vf[sub][ct], pf[sub], oacc[ct], 0, 0, 0);
      st_cur = (st_cur + 1 == D) ? 0 : st_cur + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the zero-sized tail DMAs too, before the workgroup retires
  }

  // ---- out = fp16(fp32(N) * (s_v / fp32(L))): lane (query l31) has channels ct * 32 + 8 g + 4 hi + 0..3 (attention8's store) ----
  const float rinv = __fdiv_rn(a.s_v, (float)xor32_usum(lsum));
  half_t* orow = a.out + ((size_t)b * a.S + q) * a.ldo + (size_t)h * 64;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      // widen the stores: the two half-waves trade 8-byte groups so that each lane ends up with 16 contiguous bytes
      unsigned w[2][2];
#pragma unroll
      for (int u2 = 0; u2 < 2; ++u2) {
        const half2v lo = {(half_t)__fmul_rn((float)oacc[ct][4 * (g + u2)], rinv), (half_t)__fmul_rn((float)oacc[ct][4 * (g + u2) + 1], rinv)};
        const half2v hh = {(half_t)__fmul_rn((float)oacc[ct][4 * (g + u2) + 2], rinv), (half_t)__fmul_rn((float)oacc[ct][4 * (g + u2) + 3], rinv)};
        w[u2][0] = __builtin_bit_cast(unsigned, lo);
        w[u2][1] = __builtin_bit_cast(unsigned, hh);
      }
      unsigned o4[4];
#pragma unroll
      for (int dw = 0; dw < 2; ++dw) {
        const auto r = __builtin_amdgcn_permlane32_swap(w[0][dw], w[1][dw], false, false);
        const unsigned r0 = r[0], r1 = r[1];
        o4[dw] = r0;         // lower half: own group g              | upper half: the lower half's group g + 1
        o4[2 + dw] = r1;     // lower half: the upper half's group g | upper half: own group g + 1
      }
      if (q < a.S) {
        const uintx4 ov = {o4[0], o4[1], o4[2], o4[3]};
        out_store(reinterpret_cast<uintx4*>(orow + ct * 32 + 8 * g + 8 * hi), ov);
      }
    }
}

// ---- the quantizer in front of it: qk (B S, 2C) fp16 -> qk_q int8 (q columns by inv_q, k columns by inv_k), V^T (B, C, ldv) fp16 in
//      the key order vt_perm_in (0 natural, 1 attention8's) -> vt_q (B, C, S) int8 in attention_i8_vt_key's order, by inv_v.  One
//      thread per eight q | k elements, then one per four V^T elements (a 4-key block is contiguous in all three orders) ----
struct EinsumQuantArgs {
  const half_t* qk;
  const half_t* vt;
  int8_t* qk_q;
  int8_t* vt_q;
  int S, C, ldv, vt_perm_in;
  size_t n_qk8, n_vt4;
  float inv_q, inv_k, inv_v;
};
__global__ __launch_bounds__(256) void einsum_quantize_kernel(EinsumQuantArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_qk8) {
    const int per_row = a.C / 4;                              // groups of eight in a row of 2C
    const int g = (int)(i % per_row);
    const half8 x = *reinterpret_cast<const half8*>(a.qk + i * 8);
    *reinterpret_cast<uintx2*>(a.qk_q + i * 8) = ws_quantize8(x, g * 8 < a.C ? a.inv_q : a.inv_k);
    return;
  }
  const size_t j = i - a.n_qk8;
  if (j >= a.n_vt4) return;
  const int per_row = a.S / 4;
  const size_t row = j / per_row;                            // (sample, channel)
  const int p = (int)(j % per_row) * 4;                      // first output position of the group
  const int key = (p & ~31) + attention_i8_vt_key(p & 31);   // a multiple of 4
  int src = key;
  if (a.vt_perm_in == 1) {                                   // attention8's order: the middle 4-key blocks of every 16 keys swapped
    const int o = key & 15;
    src = (o >= 4 && o < 12) ? key + (o < 8 ? 4 : -4) : key;
  }
  const half4 v = *reinterpret_cast<const half4*>(a.vt + row * a.ldv + src);
  const half8 x = {v[0], v[1], v[2], v[3], (half_t)0, (half_t)0, (half_t)0, (half_t)0};
  *reinterpret_cast<unsigned*>(a.vt_q + row * a.S + p) = ws_quantize8(x, a.inv_v)[0];
}

// ---- the observer of a calibrating handle: max |q|, max |k| (the columns of qk) and max |V^T| (the S live columns of every row)
//      folded into slots[0..2] (non-negative fp32: atomicMax on the bit pattern, as launch_absmax_half) ----
__global__ __launch_bounds__(256) void einsum_absmax_kernel(const half_t* qk, const half_t* vt, int S, int C, int ldv, size_t n_qk8, size_t n_vt4,
                                                            float* slots) {
  float mq = 0.f, mk = 0.f, mv = 0.f;
  const size_t stride = (size_t)gridDim.x * 256;
  const int per_row_qk = C / 4, per_row_v = S / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_qk8 + n_vt4; i += stride) {
    if (i < n_qk8) {
      const half8 x = *reinterpret_cast<const half8*>(qk + i * 8);
      float mx = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = fabsf((float)x[e]);
        mx = v > mx ? v : mx;                                // (NaN compares false: ignored, as launch_absmax_half does)
      }
      if ((int)(i % per_row_qk) * 8 < C) mq = fmaxf(mq, mx);
      else mk = fmaxf(mk, mx);
    } else {
      const size_t j = i - n_qk8;
      const half4 x = *reinterpret_cast<const half4*>(vt + (j / per_row_v) * ldv + (j % per_row_v) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = fabsf((float)x[e]);
        mv = v > mv ? v : mv;
      }
    }
  }
  float m3[3] = {mq, mk, mv};
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    float v = m3[t];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0 && v > 0.f) atomicMax(reinterpret_cast<unsigned*>(slots + t), __float_as_uint(v));
  }
}

template <int WAVES, int D>
void launch_i8(AttnI8Args a, int B, hipStream_t s) {
  a.q_tiles = cdiv(a.S, WAVES * 32);
  constexpr size_t lds = (size_t)D * STAGE_BYTES;
  auto k = attn_i8_kernel<WAVES, D>;
  static DynLdsOnce once;
  once.set(k, lds);
  hipLaunchKernelGGL(k, dim3(a.q_tiles * a.heads * B), dim3(WAVES * 64), lds, s, a);
}

}  // namespace

// The shape rule, in one place: what attention8.hip runs in fp16 as a self-attention, inside the exact int32 sums of step 4.
bool attention_i8_shape_ok(int d, int Sq, int Sk) { return d == 64 && Sq == Sk && Sk >= KT && Sk % KT == 0 && Sk <= kAttnI8MaxS; }

float attention_i8_score_scale(float q_absmax, float k_absmax, int d) {
  const float s_q = q_absmax / 127.0f, s_k = k_absmax / 127.0f;
  return (float)((((double)s_q * (double)s_k) * (1.0 / std::sqrt((double)d))) * 1.4426950408889634);
}

AttnKernel attention_i8_kernel(const AttnI8Desc& d) {
  SD_REQUIRE(attention_i8_shape_ok(64, d.S, d.S) && d.B > 0 && d.heads > 0, kInvalidArgument, "attention_i8: S = %d (B %d, heads %d) is off the shape rule",
             d.S, d.B, d.heads);
  AttnKernel c;
  c.family = kAttnFamilyI8;
  c.waves = attention_waves(d.B, d.heads, d.S);   // attention8's rule
  return c;
}

void launch_attention_i8(const AttnI8Desc& d, hipStream_t s) {
  const size_t lim = (size_t)1 << 31;
  const AttnKernel c = attention_i8_kernel(d);
  SD_REQUIRE(d.ldq % 16 == 0 && d.ldk % 16 == 0 && d.ldv % 16 == 0 && d.ldo % 8 == 0 && (size_t)d.S * d.ldk < lim && (size_t)64 * d.ldv < lim,
             kInvalidArgument, "attention_i8: strides %d %d %d %d", d.ldq, d.ldk, d.ldv, d.ldo);
  AttnI8Args a{d.q, d.k, d.vt, d.out, d.heads, d.S, d.ldq, d.ldk, d.ldv, d.ldo, attention_i8_score_scale(d.q_absmax, d.k_absmax, 64),
               d.v_absmax / 127.0f, 0};
  if (c.waves == 8) launch_i8<8, 4>(a, d.B, s);
  else launch_i8<4, 4>(a, d.B, s);
  SD_HIP(hipGetLastError());
}

void launch_einsum_quantize(const half_t* qk, const half_t* vt, int B, int S, int C, int ldv, int vt_perm_in, float inv_q, float inv_k,
                            float inv_v, int8_t* qk_q, int8_t* vt_q, hipStream_t s) {
  SD_REQUIRE(B > 0 && S > 0 && C > 0 && S % 32 == 0 && C % 8 == 0 && ldv % 4 == 0 && ldv >= S && (vt_perm_in == 0 || vt_perm_in == 1), kInvalidArgument,
             "einsum_quantize: B %d S %d C %d ldv %d vt_perm_in %d", B, S, C, ldv, vt_perm_in);
  EinsumQuantArgs a{qk, vt, qk_q, vt_q, S, C, ldv, vt_perm_in, (size_t)B * S * (C / 4), (size_t)B * C * (S / 4), inv_q, inv_k, inv_v};
  const size_t n = a.n_qk8 + a.n_vt4;
  hipLaunchKernelGGL(einsum_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  SD_HIP(hipGetLastError());
}

void launch_einsum_absmax(const half_t* qk, const half_t* vt, int B, int S, int C, int ldv, float* slots, hipStream_t s) {
  SD_REQUIRE(B > 0 && S > 0 && C > 0 && S % 4 == 0 && C % 8 == 0 && ldv % 4 == 0 && ldv >= S, kInvalidArgument, "einsum_absmax: B %d S %d C %d ldv %d", B,
             S, C, ldv);
  const size_t n_qk8 = (size_t)B * S * (C / 4), n_vt4 = (size_t)B * C * (S / 4);
  const size_t n = n_qk8 + n_vt4;
  const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(einsum_absmax_kernel, dim3(grid), dim3(256), 0, s, qk, vt, S, C, ldv, n_qk8, n_vt4, slots);
  SD_HIP(hipGetLastError());
}

}  // namespace sd
