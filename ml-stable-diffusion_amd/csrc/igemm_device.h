// Shared by the MFMA conv / GEMM kernel files (igemm.hip, conv3x3_halo.hip, conv_small.hip): the kernel argument block, the device
// helpers and epilogues more than one kernel family uses, and the host helpers that fill the arguments of a planned launch.
// Everything here sits in an unnamed namespace: each kernel file instantiates its own copies, and the kernels keep the symbol names
// they had as one file (profiles and tools match on them).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "conv_plan.h"

namespace sd {

// >= 16 B of device zeros (IgemmArgs::zeros).  device_zero_chunk() (kernels.h) allocates them; a launch only reads the pointer.
const half_t* zero_chunk();

// conv3x3_halo.hip: the launch of plan tile 7; returns the GroupNorm partial entries per (sample, group) its epilogue wrote
int launch_halo_ks(const ConvDesc& d, const ConvPlan& p, float* partial, hipStream_t s);
// conv3x3_halo_i8.hip: the launch of plan tile 18 (d.cw of kind I8Halo), same return
int launch_halo_i8(const ConvDesc& d, const ConvPlan& p, float* partial, hipStream_t s);
// conv3x3_halo_pal.hip: the launch of plan tile 25 (d.cw of kind PalHalo), same return
int launch_halo_pal(const ConvDesc& d, const ConvPlan& p, float* partial, hipStream_t s);
// conv3x3_halo_sp.hip: the launch of plan tile 21 (d.subpix, d.w the folded matrix); writes no GroupNorm statistics (returns 0)
int launch_halo_sp(const ConvDesc& d, const ConvPlan& p, float* partial, hipStream_t s);

namespace {

constexpr int BK = kConvBK;       // K step (halves)
constexpr int LDS_ROW = BK + 8;   // padded row stride in halves (144 B): 16 rows -> 16 distinct 16-B slots

struct IgemmArgs {
  const half_t* x0;
  const half_t* x1;
  const half_t* w;
  const float* bias;
  const float* temb;
  const half_t* res;
  half_t* out;
  float* partial;
  int C0, C1, Ctot;
  int B, Hi, Wi, Ho, Wo, HoWo;
  int ksize, stride, up, pad;
  int M, N, K;
  int temb_stride;
  int nk_total, nk_per_split, splitk;
  int slab;   // 1: the tile leaves as an fp32 slab of a.partial (split-K, or a forced slab for reduce_twin_kernel), no epilogue
  int out_mode, ldT;
  int debug;   // ablation (microbench only): bits 0-1: 1 = loads+barriers only, 2 = compute only; bit 2: timestamps
  long long* prof;
  const half_t* zeros;   // >= 16 B of zeros: source of padding / out-of-range rows
  int tiles_x, tiles_y;  // halo kernel: 8x16-pixel output tiles per image
  // LayerNorm folded into a 1x1 GEMM (LNF kernels): w already carries gamma, bias carries W.beta,
  // colsum[n] = sum_k w[n][k]; the kernel accumulates the row statistics of its A tile on the fly
  const float* ln_colsum;
  float ln_eps;
  // fused q|k|v projection: output columns >= n_trans go, token-transposed, to out_t [B][N-n_trans][ldT]
  // (the V^T operand of attention); columns below it to out with row length ldo
  int n_trans, ldo;
  half_t* out_t;
  int vt_perm;   // 1: out_t rows leave with the two middle 4-token blocks of every 16 tokens swapped (AttnDesc::vt_perm)
  int res_pre;   // 1: igemm_kernel fetches its residual tile at kernel entry (SD_RES_PREFETCH=0 switches it off, A/B)
  // GroupNorm statistics of the OUTPUT tensor from this kernel's epilogue (the consumer is torch.nn.GroupNorm of
  // unet.py:430-451 / :528-531): per (sample, group, m-tile) partial (sum, sumsq) of the fp16-rounded outputs, written to
  // gn_partial [B][G][kGnMaxSlabs][2] at entry mt * 2 + slot (slot 1: the part of a group that began in the previous n-tile).
  // Every entry < 2 * gn_T is written by exactly one workgroup per launch (no atomics: the replay stays bit-reproducible).
  float* gn_partial;
  int gn_G, gn_cpg, gn_T;   // groups, channels per group, m-tiles per sample
  // Tile order inside an XCD's contiguous run of workgroup ids.  0: m fastest - consecutive workgroups share a WEIGHT panel
  // (right when the weights outweigh the activations: the 8x8 / 16x16 levels at small batch).  1: n fastest - consecutive
  // workgroups share an ACTIVATION panel, so each XCD pulls its rows through the fabric once and the other n-tiles hit its L2
  // (round 2 measured 27 MB of fabric reads for a 320->320 GEMM at M = 8192 with 10.6 MB of operands: every n-tile of a row
  // block ran on a different XCD).  Chosen per launch from the operand sizes (launch_conv).
  int n_fast;
  // GroupNorm folded into a 1x1 GEMM (gemm_pipe_kernel GNF): partial (sum, sumsq) entries of the input's producer, affine, eps
  const float* gnf_partial;
  const float* gnf_gamma;
  const float* gnf_beta;
  float gnf_eps;
  int gnf_G, gnf_entries;
  // fused q|k|v: columns [0, q_cols) leave multiplied by q_scale in fp32 (ConvDesc::q_scale); q_cols = 0: off
  float q_scale;
  int q_cols;
};

constexpr int kGnScratchFloats = 256 * 17;   // per-thread (sum[8], sumsq[8]) of the epilogue's store loop, +1 pad

// Per-tile GroupNorm statistics from the store loop of an epilogue.  Thread t owns the 8-channel chunk (t % (BN/8)) of the
// rows it stored; fs / fq are its sums over those rows.  scratch: kGnScratchFloats + 2 * BN floats of LDS that no thread
// reads or writes any more.  Fixed-order reductions only.
template <int BN>
__device__ __forceinline__ void tile_gn_stats(const IgemmArgs& a, float* scratch, const float (&fs)[8], const float (&fq)[8],
                                              int n_blk, int b, int mt) {
  constexpr int OWC = BN / 8;
  const int tid = threadIdx.x;
  float* chan = scratch + kGnScratchFloats;   // [2][BN] per-channel sum | sumsq of this tile
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    scratch[tid * 17 + e] = fs[e];
    scratch[tid * 17 + 8 + e] = fq[e];
  }
  __syncthreads();
  for (int cc = tid; cc < 2 * BN; cc += 256) {
    const int which = cc / BN, ch = cc - which * BN;
    const int cl = ch >> 3, e = ch & 7;
    float s = 0.f;
#pragma unroll 4
    for (int k = 0; k < 256 / OWC; ++k) s += scratch[(k * OWC + cl) * 17 + which * 8 + e];
    chan[cc] = s;
  }
  __syncthreads();
  const int g0 = n_blk / a.gn_cpg;
  const int g = g0 + tid;
  const int n_end = min(n_blk + BN, a.N);
  if (tid < BN && g < a.gn_G && g * a.gn_cpg < n_end) {
    const int gs = g * a.gn_cpg, ge = gs + a.gn_cpg;
    const int lo = max(gs, n_blk), hi = min(ge, n_end);
    float s = 0.f, q = 0.f;
    for (int c = lo; c < hi; ++c) {
      s += chan[c - n_blk];
      q += chan[BN + c - n_blk];
    }
    float* dst = a.gn_partial + (((size_t)b * a.gn_G + g) * kGnMaxSlabs + (size_t)mt * 2) * 2;
    if (gs < n_blk) {            // the group began in the previous n-tile, which wrote slot 0
      dst[2] = s;
      dst[3] = q;
    } else {
      dst[0] = s;
      dst[1] = q;
      if (ge <= n_end) {         // the group ends inside this tile: nobody else writes slot 1
        dst[2] = 0.f;
        dst[3] = 0.f;
      }
    }
  }
}

// exact-GELU (erf form, unet.py:613-617 via F.gelu) with erf from Abramowitz-Stegun 7.1.26:
// |erf error| < 6.1e-7 in fp32, |gelu error| < 3.7e-7 absolute and < 1.7e-4 relative wherever
// |gelu| > 1e-3 - below the fp16 rounding of the output - at a third of the VALU cost of the
// libm erff: with K only 320-1280 deep the epilogue is a visible share of a GEGLU GEMM
// (measured 610 -> 501 us per UNet step over the 16 GEGLU launches, tools/geglu_bench.py).
__device__ __forceinline__ float gelu_erf(float x) {
  const float z = x * 0.70710678118654752f;
  const float az = fabsf(z);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.0f));
  float p = 1.061405429f;
  p = fmaf(p, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(-az * az * 1.4426950408889634f);
  const float erf_abs = fmaf(-p * t, e, 1.0f);
  return 0.5f * x * (1.0f + copysignf(erf_abs, z));
}

// v + (value of lane ^ 32): one v_permlane32_swap instead of a ds_bpermute round trip
__device__ __forceinline__ float xor32_sum(float v) {
  const unsigned u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const unsigned r0 = r[0], r1 = r[1];   // scalars first: bit-casting the vector-element lvalue reads lane 0 twice
  return __uint_as_float(r0) + __uint_as_float(r1);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
#include "gn_body.inc"   // groupnorm_apply_body / groupnorm_fused_body (the stand-alone launches are in norm.hip)

// buffer_load_dwordx4 ... lds (16 bytes per lane straight into LDS; M0 carries the wave-uniform LDS base).  hipcc's HOST pass
// checks the 16-byte form against a target without the gfx950 feature and then silently drops the enclosing kernel's stub,
// so the builtin is only visible to the device pass.
__device__ __forceinline__ void dma16_to_lds(const __amdgpu_buffer_rsrc_t& rs, char* lds, unsigned voffset, int soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 16, voffset, soffset, 0, 0);
#endif
}

// Tile epilogue shared by the GEMM kernels: acc[i][j] is the 32x32 block (pixel block (wm*TM+i), channel block (wn*TN+j)) of
// a BM x BN tile owned by wave (wm, wn) of a WGM x WGN wave grid, in the transposed MFMA layout
// n = n0 + (r&3) + 8*(r>>2) + 4*hi ; m = m0 + (lane&31).  Split-K slabs, or bias / timestep embedding / LayerNorm fold /
// GEGLU / residual / fused q|k|v write-out staged through LDS (`smem` is free: the caller's K loop is over and every wave
// has passed a barrier after its last fragment read - this function starts with its own barrier for that).
// resv (NRES > 0, use_resv): the residual chunks of the final store loop, fetched by the caller at kernel entry - read here, a
// residual tile costs every workgroup one exposed memory round trip after its K loop.
template <int BM, int BN, int WGM, int WGN, int TM, int TN, bool LNF, int NRES = 0>
__device__ __forceinline__ void tile_epilogue(const IgemmArgs& a, floatx16 (&acc)[TM][TN], const float (&ln_a)[TM],
                                              const float (&ln_b)[TM], char* smem, float* sconst, float const_b, float const_t,
                                              float const_c, int m_blk, int n_blk, int wave, int split, bool temb_uniform,
                                              const half8* resv = nullptr, bool use_resv = false) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wm = wave / WGN, wn = wave % WGN;
  const int frow = lane & 31, hi = lane >> 5;
  // acc[i][j][r]: n = n0 + (r&3) + 8*(r>>2) + 4*hi ; m = m0 + (lane&31)
  if (a.slab) {   // fp32 partial slabs; bias/temb/residual are applied by splitk_reduce_kernel / reduce_twin_kernel
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m_blk + (wm * TM + i) * 32 + frow;
      if (m >= a.M) continue;
      float* prow = a.partial + ((size_t)split * a.M + m) * a.N;
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n_blk + (wn * TN + j) * 32 + 8 * q + 4 * hi;
          if (n < a.N) {
            floatx4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
            out_store(reinterpret_cast<floatx4*>(prow + n), v);
          }
        }
    }
  } else {
    // Stage the finished tile through LDS (free after the K loop) so that the global stores - and
    // the residual loads - are whole 16-B-per-lane row segments instead of 32 scattered 16-B pieces
    // per instruction (the scattered form cost ~11k cycles per 128x128 tile, prof_conv).
    const bool geglu = a.out_mode == kOutGeglu;
    constexpr int OW = BN;                 // staged tile width in halves (GEGLU uses the first BN/2)
    constexpr int OROW = OW + 8;           // +16 B pad: conflict-free 16-B reads
    constexpr int TROW = BM + 8;           // transposed staging (fused q|k|v: the V^T columns), [BN][TROW]
    half_t* ot = reinterpret_cast<half_t*>(smem);   // [BM][OROW] or [BN][TROW]  (<= the K-loop buffers)
    const bool tblock = n_blk >= a.n_trans;         // block-uniform
    if (tid < BN) {
      sconst[tid] = const_b + const_t;
      if constexpr (LNF) sconst[BN + tid] = const_c;
    }
    __syncthreads();                       // every wave is done with its last fragment reads; sconst is visible
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int ml = (wm * TM + i) * 32 + frow;
      const int m = m_blk + ml;
      const int b = (m < a.M) ? m / a.HoWo : 0;
      if (geglu) {
        if constexpr (TN % 2 == 0) {
#pragma unroll
          for (int j = 0; j < TN; j += 2)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int nl = (wn * TN + j) * 32 + 8 * q + 4 * hi;          // value rows (interleaved W)
              half4 o;
              const floatx4 bv4 = *reinterpret_cast<const floatx4*>(sconst + nl);        // 0 beyond N
              const floatx4 bg4 = *reinterpret_cast<const floatx4*>(sconst + nl + 32);
              floatx4 cv4 = {0.f, 0.f, 0.f, 0.f}, cg4 = {0.f, 0.f, 0.f, 0.f};
              if constexpr (LNF) {
                cv4 = *reinterpret_cast<const floatx4*>(sconst + BN + nl);
                cg4 = *reinterpret_cast<const floatx4*>(sconst + BN + nl + 32);
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                float v, g;
                if constexpr (LNF) {
                  v = fmaf(acc[i][j][4 * q + e], ln_a[i], fmaf(ln_b[i], cv4[e], bv4[e]));
                  g = fmaf(acc[i][j + 1][4 * q + e], ln_a[i], fmaf(ln_b[i], cg4[e], bg4[e]));
                } else {
                  v = acc[i][j][4 * q + e] + bv4[e];
                  g = acc[i][j + 1][4 * q + e] + bg4[e];
                }
                o[e] = (half_t)(v * gelu_erf(g));
              }
              *reinterpret_cast<half4*>(ot + ml * OROW + (wn * TN + j) * 16 + 8 * q + 4 * hi) = o;
            }
        }
      } else {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int nl = (wn * TN + j) * 32 + 8 * q + 4 * hi;
            const int n = n_blk + nl;
            float v[4] = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
            const floatx4 bb = *reinterpret_cast<const floatx4*>(sconst + nl);            // bias (+ temb), 0 beyond N
            if constexpr (LNF) {
              const floatx4 cs = *reinterpret_cast<const floatx4*>(sconst + BN + nl);
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], ln_a[i], fmaf(ln_b[i], cs[e], bb[e]));
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] += bb[e];
            }
            if (n < a.q_cols) {   // queries for attention8: softmax scale and log2(e) before the rounding to fp16
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] *= a.q_scale;
            }
            if (a.temb && !temb_uniform && n < a.N) {   // tile straddles samples (HoWo < BM): per-row sample index
              floatx4 tt = *reinterpret_cast<const floatx4*>(a.temb + (size_t)b * a.temb_stride + n);
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] += tt[e];
            }
            half4 o = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            if (tblock) {   // V^T columns: staged [n][m] so the write-out rows are token-contiguous
#pragma unroll
              for (int e = 0; e < 4; ++e) ot[(nl + e) * TROW + ml] = o[e];
            } else {
              *reinterpret_cast<half4*>(ot + ml * OROW + nl) = o;
            }
          }
      }
    }
    __syncthreads();
    if (tblock) {   // out_t[b][n - n_trans][s]: 8 consecutive tokens of one image per 16-B store
      const int NV = a.N - a.n_trans;
      for (int idx = tid; idx < BN * (BM / 8); idx += 256) {
        const int r = idx / (BM / 8), c = idx - r * (BM / 8);
        const int nv = n_blk + r - a.n_trans, m = m_blk + c * 8;
        if (nv < NV && m < a.M) {
          const int b = m / a.HoWo, sp = m - b * a.HoWo;
          half8 v;
          if (a.vt_perm) {   // 16-B chunk c of the row = tokens 16 j + 4 o + {0..3} and 16 j + 8 + 4 o + {0..3}  (j = c >> 1, o = c & 1)
            const half_t* src = ot + r * TROW + (c >> 1) * 16 + (c & 1) * 4;
            const half4 lo = *reinterpret_cast<const half4*>(src), up = *reinterpret_cast<const half4*>(src + 8);
            v = half8{lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
          } else {
            v = *reinterpret_cast<const half8*>(ot + r * TROW + c * 8);
          }
          out_store(reinterpret_cast<half8*>(a.out_t + ((size_t)b * NV + nv) * a.ldT + sp), v);
        }
      }
      return;
    }
    const int NO = geglu ? (a.N >> 1) : a.ldo;            // output row length
    const int nb0 = geglu ? (n_blk >> 1) : n_blk;         // first output column of this tile
    constexpr int OWC = OW / 8;                           // 16-B chunks per staged row (GEGLU: first half used)
    const int wc = geglu ? OWC / 2 : OWC;
    // GroupNorm statistics of what this tile stores (block-uniform; launch_conv checks: rows of one sample, N % 8 == 0)
    const bool gn = a.gn_partial != nullptr && !geglu;
    float fs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, fq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool stored = false;
    if constexpr (NRES > 0) {
      if (use_resv) {   // (never GEGLU: wc == OWC, BM * OWC == NRES * 256)
#pragma unroll
        for (int it = 0; it < NRES; ++it) {
          const int idx = tid + it * 256;
          const int r = idx / OWC, c = idx - r * OWC;
          const int m = m_blk + r, n = nb0 + c * 8;
          if (m < a.M && n < NO) {
            half8 v = *reinterpret_cast<const half8*>(ot + r * OROW + c * 8);
            half_t* dst = a.out + (size_t)m * NO + n;
            if (n + 8 <= NO) {
              const half8 rr = resv[it];
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] + (float)rr[e]);
              out_store(reinterpret_cast<half8*>(dst), v);
              if (gn) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                  const float f = (float)v[e];
                  fs[e] += f;
                  fq[e] = fmaf(f, f, fq[e]);
                }
              }
            } else {
              for (int e = 0; e < NO - n; ++e) dst[e] = (half_t)((float)v[e] + (float)a.res[(size_t)m * NO + n + e]);
            }
          }
        }
        stored = true;
      }
    }
    if (!stored) {
      for (int idx = tid; idx < BM * wc; idx += 256) {
        const int r = idx / wc, c = idx - r * wc;
        const int m = m_blk + r, n = nb0 + c * 8;
        if (m < a.M && n < NO) {
          half8 v = *reinterpret_cast<const half8*>(ot + r * OROW + c * 8);
          half_t* dst = a.out + (size_t)m * NO + n;
          if (n + 8 <= NO) {
            if (a.res) {
              const half8 rr = *reinterpret_cast<const half8*>(a.res + (size_t)m * NO + n);
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] + (float)rr[e]);
            }
            out_store(reinterpret_cast<half8*>(dst), v);
            if (gn) {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float f = (float)v[e];
                fs[e] += f;
                fq[e] = fmaf(f, f, fq[e]);
              }
            }
          } else {   // ragged last chunk (N % 8 == 4)
            for (int e = 0; e < NO - n; ++e) dst[e] = a.res ? (half_t)((float)v[e] + (float)a.res[(size_t)m * NO + n + e]) : v[e];
          }
        }
      }
    }
    if (gn) {   // scratch behind the staged tile (launch_variant sizes the LDS for it)
      float* scratch = reinterpret_cast<float*>(smem + (((size_t)BM * OROW * sizeof(half_t) + 15) & ~(size_t)15));
      tile_gn_stats<BN>(a, scratch, fs, fq, n_blk, m_blk / a.HoWo, (m_blk % a.HoWo) / BM);
    }
  }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt_barrier() {   // counted wait + raw barrier in one statement (no LDS access moves across)
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

IgemmArgs make_args(const ConvDesc& d) {
  IgemmArgs a{};
  a.x0 = d.x0;
  a.x1 = d.x1;
  a.w = d.w;
  a.bias = d.bias;
  a.temb = d.temb;
  a.res = d.res;
  a.out = d.out;
  a.partial = nullptr;
  a.C0 = d.C0;
  a.C1 = d.x1 ? d.C1 : 0;
  a.Ctot = a.C0 + a.C1;
  a.B = d.B;
  a.Hi = d.Hi;
  a.Wi = d.Wi;
  a.Ho = d.Ho;
  a.Wo = d.Wo;
  a.HoWo = d.Ho * d.Wo;
  a.ksize = d.ksize;
  a.stride = d.stride;
  a.up = d.up;
  a.pad = d.pad >= 0 ? d.pad : d.ksize / 2;
  a.M = d.B * d.Ho * d.Wo;
  a.N = d.N;
  a.K = d.ksize * d.ksize * a.Ctot;
  a.temb_stride = d.temb_stride;
  a.nk_total = a.K / BK;
  a.nk_per_split = a.nk_total;
  a.splitk = 1;
  a.slab = 0;
  a.out_mode = d.out_mode;
  a.ldT = d.ldT;
  a.debug = d.debug;
  a.prof = d.prof;
  a.zeros = zero_chunk();
  a.tiles_x = cdiv(d.Wo, 16);   // halo kernels: stride 1, so output = (upsampled) input extent
  a.tiles_y = cdiv(d.Ho, 8);
  a.ln_colsum = d.ln_colsum;
  a.ln_eps = d.ln_eps;
  a.n_trans = d.out_t ? d.n_trans : 0x7fffffff;
  a.ldo = d.out_t ? d.n_trans : d.N;
  a.out_t = d.out_t;
  a.vt_perm = d.out_t ? d.vt_perm : 0;
  static const int res_pre = tune_env_int("SD_RES_PREFETCH", 1) != 0;
  a.res_pre = res_pre;
  a.gn_partial = nullptr;
  a.gn_G = a.gn_cpg = a.gn_T = 0;
  a.gnf_partial = d.gnf_partial;
  a.gnf_gamma = d.gnf_gamma;
  a.gnf_beta = d.gnf_beta;
  a.gnf_eps = d.gnf_eps;
  a.gnf_G = d.gnf_groups;
  a.gnf_entries = d.gnf_entries;
  a.q_scale = d.q_scale;
  a.q_cols = d.out_t ? d.q_cols : 0;
  return a;
}

// tile order (IgemmArgs::n_fast) from the operand sizes: choose_tile_order (conv_plan.h).  halo: m-tiles are the 8x16-pixel tiles
void set_tile_order(IgemmArgs& a, int bm, int bn, bool halo = false) {
  const double nbn = (double)cdiv(a.N, bn);
  const double nbm = halo ? (double)a.B * a.tiles_x * a.tiles_y : (double)cdiv(a.M, bm);
  a.n_fast = choose_tile_order(2.0 * a.B * a.Hi * a.Wi * a.Ctot, 2.0 * a.N * a.K, nbm, nbn, true);
}

// the arguments of a planned launch: split-K range (no empty splits: conv_plan resolved it) and slab pointer; the launcher of
// the tile adds the tile order (set_tile_order)
IgemmArgs planned_args(const ConvDesc& d, const ConvPlan& p, float* partial) {
  IgemmArgs a = make_args(d);
  a.splitk = p.splitk;
  a.slab = p.slab ? 1 : 0;
  a.partial = p.slab ? partial : nullptr;
  // (the weight stream has its own arguments: these then only feed the slab combine; the halo kernel splits whole 64-channel chunks)
  if (p.kernel != ConvKernel::Wstream && p.kernel != ConvKernel::WstreamPal && p.kernel != ConvKernel::WstreamI8)
    a.nk_per_split = cdiv(p.kernel == ConvKernel::HaloKs || p.kernel == ConvKernel::HaloI8 || p.kernel == ConvKernel::HaloPal ? a.Ctot / BK : a.nk_total, p.splitk);
  return a;
}

// GroupNorm statistics from the epilogue: fills a.gn_* and returns the entries per (sample, group) the launch will write,
// or 0 when this launch cannot produce them (bm: rows per m-tile of an igemm tile, 0 for the 8x16-pixel halo tiles)
int setup_gn_stats(const ConvDesc& d, IgemmArgs& a, int bm) {
  a.gn_partial = nullptr;
  if (!d.gn_partial || d.gn_groups < 1 || a.splitk > 1 || a.slab || d.out_mode != kOutHalf || d.out_t || d.debug) return 0;
  if (a.N % d.gn_groups != 0 || a.N % 8 != 0) return 0;
  const int cpg = a.N / d.gn_groups;
  if (cpg > 64) return 0;                       // a group may span two 64-column n-tiles, not three
  int T;
  if (bm == 0) {
    T = a.tiles_x * a.tiles_y;
  } else {
    if (a.HoWo % bm != 0) return 0;             // every m-tile inside one sample
    T = a.HoWo / bm;
  }
  if (2 * T > kGnMaxSlabs) return 0;
  a.gn_partial = d.gn_partial;
  a.gn_G = d.gn_groups;
  a.gn_cpg = cpg;
  a.gn_T = T;
  return 2 * T;
}

}  // namespace

}  // namespace sd
