// K4/K5 - implicit-GEMM convolution (3x3 / 1x1, stride 1/2, fused nearest-x2 gather, fused
// channel-concat) on gfx950 MFMA (v_mfma_f32_32x32x16_f16), fp16 in / fp32 accumulate.
//
// Math (reference): nn.Conv2d calls of python_coreml_stable_diffusion/unet.py:74-84 (q/k/v/out
// 1x1), :435-468 (resnet 3x3 + 1x1 shortcut), :496-510 (up/down-sample), :533-551 (proj_in/out),
// :601-617 (GEGLU feed-forward), and the torch.cat([h, skip], dim=1) of :213-216 which we never
// materialise (second K-source).
//
// Mapping: out[m][n] = sum_k X[m][k] W[n][k]; m = (b, oy, ox) output pixel, n = output channel,
// k = tap * Ctot + c.  Both operands are K-contiguous in HBM (NHWC activations, [N][taps][C]
// weights re-laid-out at load), which is exactly the MFMA A/B fragment shape (8 consecutive k
// per lane), so tiles go HBM -> VGPR (16-B coalesced) -> LDS (padded rows, conflict-free
// ds_read_b128) -> MFMA with a register-staged double buffer (one barrier per 64-deep K step).
// The tile is computed TRANSPOSED (rows = n, cols = m) so each lane owns 4 consecutive output
// channels of one pixel: bias / timestep-embedding / residual adds and the fp16 store are 8-byte
// vector accesses with no cross-lane traffic.
//
// This file: igemm_kernel (im2col tiles), gemm_pipe_kernel (software-pipelined 1x1 GEMM), the GroupNorm + side GEMM kernels, the
// split-K combines, their launchers and launch_conv, the dispatch on the plan of conv_plan.cpp.  The 3x3 halo conv is in
// conv3x3_halo.hip, the direct convs in conv_small.hip; the three share igemm_device.h.
#include "igemm_device.h"

namespace sd {

namespace {

// One 256-thread workgroup = 4 wavefronts laid out WGM x WGN over a BM x BN tile.
// GLDS = true: tiles go HBM -> LDS directly (global_load_lds_dwordx4, no VGPR round trip and no
// ds_write pass: the write pass was ~60 % of the LDS-pipe time of the register-staged version).
// The DMA writes lane-linear 1-KiB pieces (8 rows x 128 B), so the bank swizzle lives on the
// per-lane SOURCE address: physical 16-B chunk p of row r holds logical chunk p ^ ((r >> 1) & 7),
// and fragment reads apply the same XOR (conflict-free ds_read_b128, cdna guide rule 21).
// KG = 2 (round 5): IN-WORKGROUP split-K.  The small-M GEMMs of the 16x16 / 8x8 levels (1280 -> 1280 at M = 512: 160 tiles of
// 64 x 64, 20 K steps each) expose their serial K loop - 0.45 us per barrier-separated step - on 160 of 256 CUs; a split-K over
// workgroups costs a dependent reduce launch (measured: it loses).  Here a workgroup is TWO groups of four waves, each with its
// own LDS ring, walking one half of the K range in lockstep (the s_barrier is workgroup-wide; the shorter half pads with one
// barrier-only step); group 1 hands its accumulators over through LDS and retires (s_barrier only waits for surviving
// waves), group 0 adds them and runs the epilogue.  Same loop body, half as many steps, no HBM slabs, no extra launch.
template <int BM, int BN, int WGM, int WGN, bool TRANS_OUT, bool GLDS, int NST, int DBG = 0, bool LNF = false, int KG = 1>
__global__ __launch_bounds__(256 * KG) void igemm_kernel(IgemmArgs a) {
  static_assert(WGM * WGN == 4, "4 waves");
  static_assert(KG == 1 || (KG == 2 && GLDS && NST >= 3 && !LNF && !TRANS_OUT && DBG == 0), "in-workgroup split-K: ring variants of the plain epilogue");
  static_assert(!(LNF && TRANS_OUT), "LayerNorm fold uses the in-lane row layout of the non-transposed tile");
  constexpr int TM = BM / WGM / 32;   // 32x32 MFMA tiles per wave along m
  constexpr int TN = BN / WGN / 32;
  constexpr int XR = BM / 32;         // 16-B chunks each thread stages per K step (X tile)
  constexpr int WR = BN / 32;
  constexpr int ROW = GLDS ? BK : LDS_ROW;   // LDS row stride in halves

  // DBG (compile-time, microbench-only instantiations): bits 0-1: 1 = loads+barriers only, 2 = compute only;
  // bit 2: phase timestamps; bit 3: no LDS reads; bit 4: no MFMAs.  Production kernels have DBG == 0.
  const bool prof = (DBG & 4) && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;
  long long prof_t[4];
  long long prof_w0 = 0;
  if (prof) { prof_t[0] = clock64(); prof_w0 = wall_clock64(); }
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int kg = KG > 1 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8) : 0;   // K group of this wave
  half_t* Xs = reinterpret_cast<half_t*>(smem) + (size_t)kg * NST * (BM + BN) * ROW;   // [NST][BM][ROW] of this K group
  half_t* Ws = Xs + NST * BM * ROW;                             // [NST][BN][ROW]
  // behind the ring: per-column epilogue constants [BN] bias (+ timestep-embedding row when the tile lies in
  // one sample) | [BN] LayerNorm colsum.  Loaded once per workgroup next to the first tile's DMA, so the
  // epilogue reads them from LDS instead of issuing dependent global loads per accumulator fragment
  // (those cost the 128x128 tile ~9k cycles, profiles/r01_prof_conv_phases.log).
  float* sconst = reinterpret_cast<float*>(smem + (size_t)KG * NST * (BM + BN) * ROW * sizeof(half_t));

  const int tid = threadIdx.x & 255;   // thread inside its K group
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform (LDS-DMA base -> M0)
  const int wm = wave / WGN, wn = wave % WGN;

  // XCD-aware tile order: the dispatcher round-robins consecutive block ids over the 8 XCDs
  // (MI355X_MICROARCH: block b -> XCD b % 8).  Remap so that each XCD walks a contiguous run of
  // tiles that share the same weight panel (n-tile) -> the panel stays in that XCD's L2.
  int nbm = (a.M + BM - 1) / BM, nbn = (a.N + BN - 1) / BN;
  int nwg = nbm * nbn;
  int bid = blockIdx.x;
  {
    int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    bid = base + idx;   // bijective for any nwg
  }
  const int bn_idx = a.n_fast ? bid % nbn : bid / nbm, bm_idx = a.n_fast ? bid / nbn : bid % nbm;   // IgemmArgs::n_fast
  const int m_blk = bm_idx * BM, n_blk = bn_idx * BN;

  const int split = blockIdx.y;
  int kt_begin = split * a.nk_per_split;
  int kt_end = kt_begin + a.nk_per_split;
  if (kt_end > a.nk_total) kt_end = a.nk_total;
  int kg_steps = kt_end - kt_begin;   // barrier-separated steps every K group goes through (KG == 2: the longer half)
  if constexpr (KG == 2) {
    const int half0 = (kt_end - kt_begin + 1) >> 1;
    kg_steps = half0;
    if (kg == 0) kt_end = kt_begin + half0;
    else kt_begin += half0;
  }

  // ---- per-thread staging coordinates (loop invariant) ----
  const int pchunk = tid & 7;       // physical 16-B slot of the 128-B K row this thread fills
  const int lrow = tid >> 3;        // 0..31  (= wave * 8 + lane / 8)
  int x_pix[XR];                    // b*Hi*Wi (or -1 when the row is past M)
  int x_iy0[XR], x_ix0[XR];
#pragma unroll
  for (int i = 0; i < XR; ++i) {
    int m = m_blk + lrow + 32 * i;
    if (m < a.M) {
      int b = m / a.HoWo;
      int rem = m - b * a.HoWo;
      int oy = rem / a.Wo;
      int ox = rem - oy * a.Wo;
      x_pix[i] = b * a.Hi * a.Wi;
      x_iy0[i] = oy * a.stride - a.pad;
      x_ix0[i] = ox * a.stride - a.pad;
    } else {
      x_pix[i] = -1;
      x_iy0[i] = 0;
      x_ix0[i] = 0;
    }
  }
  const int Hup = a.Hi * a.up, Wup = a.Wi * a.up;
  const int upshift = a.up >> 1;    // up in {1,2}
  // logical chunk this thread fetches for its rows: rows lrow+32*i share (row >> 1) & 7 == (lrow >> 1) & 7
  const int chunk = GLDS ? (pchunk ^ ((lrow >> 1) & 7)) : pchunk;

  half8 xr[GLDS ? 1 : XR], wr[GLDS ? 1 : WR];

  // K-tile iterator.  Tiles are visited in order, so every staged row just walks a pointer:
  // per K step the loader is one 64-bit add per row.  The im2col source (3x3 tap shift, zero
  // padding, nearest-x2 upsample, which of the two concat sources) is re-derived only when the
  // tap or the source changes (every Ctot/64 or C0/64 steps) - a wave-uniform, rarely taken branch.
  int it_tap = (kt_begin * BK) / a.Ctot;
  int it_cc = kt_begin * BK - it_tap * a.Ctot;
  bool retarget = true;
  const half_t* const zeros = a.zeros;
  const half_t* xp[XR];             // where this thread's 16 bytes of row i come from for the next tile
  int xstep[XR];                    // halves to advance per K step: BK, or 0 while the row reads zeros
  const half_t* wp[WR];
  int wstep[WR];
#pragma unroll
  for (int i = 0; i < WR; ++i) {
    int n = n_blk + lrow + 32 * i;
    wp[i] = (n < a.N) ? a.w + (size_t)n * a.K + (size_t)kt_begin * BK + chunk * 8 : zeros;
    wstep[i] = (n < a.N) ? BK : 0;
  }

  auto load_tile = [&](int stage) {
    if constexpr ((DBG & 3) == 2) return;
    if (retarget) {                   // wave-uniform
      const int ky = (a.ksize == 3) ? it_tap / 3 : 0;
      const int kx = (a.ksize == 3) ? it_tap - ky * 3 : 0;
      int cc = it_cc;
      const half_t* src = a.x0;
      int Csrc = a.C0;
      if (cc >= a.C0) {
        src = a.x1;
        cc -= a.C0;
        Csrc = a.C1;
      }
      src += cc + chunk * 8;
#pragma unroll
      for (int i = 0; i < XR; ++i) {
        int iy = x_iy0[i] + ky, ix = x_ix0[i] + kx;
        bool ok = (x_pix[i] >= 0) && (iy >= 0) && (iy < Hup) && (ix >= 0) && (ix < Wup);
        int pix = x_pix[i] + (iy >> upshift) * a.Wi + (ix >> upshift);
        xp[i] = ok ? src + (size_t)pix * Csrc : zeros;
        xstep[i] = ok ? BK : 0;
      }
    }
    it_cc += BK;                      // advance the iterator for the next call
    if (it_cc >= a.Ctot) {
      it_cc = 0;
      ++it_tap;
    }
    retarget = (it_cc == 0) || (it_cc == a.C0);
    if constexpr (GLDS) {
      char* xs = reinterpret_cast<char*>(Xs + stage * BM * ROW) + wave * 1024;   // wave-uniform piece base
      char* ws = reinterpret_cast<char*>(Ws + stage * BN * ROW) + wave * 1024;
#pragma unroll
      for (int i = 0; i < XR; ++i) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)xp[i],
                                         (__attribute__((address_space(3))) void*)(xs + i * 4096), 16, 0, 0);
        xp[i] += xstep[i];
      }
#pragma unroll
      for (int i = 0; i < WR; ++i) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)wp[i],
                                         (__attribute__((address_space(3))) void*)(ws + i * 4096), 16, 0, 0);
        wp[i] += wstep[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < XR; ++i) {
        xr[i] = *reinterpret_cast<const half8*>(xp[i]);
        xp[i] += xstep[i];
      }
#pragma unroll
      for (int i = 0; i < WR; ++i) {
        wr[i] = *reinterpret_cast<const half8*>(wp[i]);
        wp[i] += wstep[i];
      }
    }
  };
  auto store_tile = [&](int buf) {   // register-staged variant only
    if constexpr (!GLDS) {
      half_t* xs = Xs + buf * BM * ROW;
      half_t* ws = Ws + buf * BN * ROW;
#pragma unroll
      for (int i = 0; i < XR; ++i)
        *reinterpret_cast<half8*>(xs + (lrow + 32 * i) * ROW + chunk * 8) = xr[i];
#pragma unroll
      for (int i = 0; i < WR; ++i)
        *reinterpret_cast<half8*>(ws + (lrow + 32 * i) * ROW + chunk * 8) = wr[i];
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int frow = lane & 31;           // fragment row (m or n within the 32-tile)
  const int fk = (lane >> 5) * 8;       // k offset of this half-wave inside a 16-deep MFMA step
  const int fsw = (frow >> 1) & 7;      // GLDS: swizzle of this lane's fragment rows (tile bases are multiples of 32)

  // K-step body, split so the next tile's address math + DMA issue can sit in the shadow of the MFMAs:
  //   read_frags(buf)  - all 16 ds_read_b128 of the step up front (with one wave per SIMD a
  //                      read->wait->4 MFMA chain exposes the LDS latency four times per step)
  //   [load_tile(next)] - scheduled by the compiler between / behind the MFMAs
  //   mfma_step()      - 16 back-to-back MFMAs
  half8 xf[BK / 16][TM] = {}, wf[BK / 16][TN] = {};
  // LNF: per-lane partial sum / sum of squares of activation row (lane & 31) of each m-tile, over the
  // k chunks this half-wave reads (v_dot2_f32_f16: exact fp16 products, fp32 accumulation)
  float ln_s1[TM] = {}, ln_s2[TM] = {};
  auto read_frags = [&](int buf) {
    if constexpr ((DBG & 3) == 1) return;
    if constexpr ((DBG & 8) != 0) {   // ablation: no LDS reads (fragments = loop-invariant garbage kept live)
#pragma unroll
      for (int kk = 0; kk < BK / 16; ++kk) {
#pragma unroll
        for (int i = 0; i < TM; ++i) asm volatile("" : "+v"(xf[kk][i]));
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(wf[kk][j]));
      }
      return;
    }
    const half_t* xs = Xs + buf * BM * ROW + (wm * TM * 32 + frow) * ROW;
    const half_t* ws = Ws + buf * BN * ROW + (wn * TN * 32 + frow) * ROW;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      const int koff = GLDS ? (((kk * 2 + (lane >> 5)) ^ fsw) * 8) : (kk * 16 + fk);
#pragma unroll
      for (int i = 0; i < TM; ++i) xf[kk][i] = *reinterpret_cast<const half8*>(xs + i * 32 * ROW + koff);
#pragma unroll
      for (int j = 0; j < TN; ++j) wf[kk][j] = *reinterpret_cast<const half8*>(ws + j * 32 * ROW + koff);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the reads ahead (the scheduler would sink them back to their uses)
  };
  auto mfma_step = [&]() {
    if constexpr ((DBG & 3) == 1) return;
    if constexpr ((DBG & 16) != 0) {  // ablation: no MFMAs (fragments consumed so the reads stay)
#pragma unroll
      for (int kk = 0; kk < BK / 16; ++kk) {
#pragma unroll
        for (int i = 0; i < TM; ++i) asm volatile("" ::"v"(xf[kk][i]));
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(wf[kk][j]));
      }
      return;
    }
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr (TRANS_OUT)   // rows = m, cols = n
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xf[kk][i], wf[kk][j], acc[i][j], 0, 0, 0);
          else                       // rows = n, cols = m
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[kk][j], xf[kk][i], acc[i][j], 0, 0, 0);
        }
      if constexpr (LNF) {           // VALU work that fits the issue slots between the MFMAs
        const half2v one2 = {(half_t)1.f, (half_t)1.f};
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const half2v p2 = {xf[kk][i][2 * e], xf[kk][i][2 * e + 1]};
            ln_s2[i] = __builtin_amdgcn_fdot2(p2, p2, ln_s2[i], false);
            ln_s1[i] = __builtin_amdgcn_fdot2(p2, one2, ln_s1[i], false);
          }
      }
    }
  };

  // the tile lies inside one sample -> its timestep-embedding row is a per-column constant too
  const bool temb_uniform = a.temb != nullptr && (a.HoWo % BM) == 0;
  // issued before the first tile's DMA (oldest VMEM ops of the wave, so the counted vmcnt waits of the ring
  // are unaffected); first used after the K loop, where they are written to LDS ahead of the epilogue barrier
  float const_b = 0.f, const_t = 0.f, const_c = 0.f;   // combined only at the store: no early use, no early wait
  const bool use_consts = !TRANS_OUT && !a.slab;
  if (use_consts && tid < BN) {
    const int n = n_blk + tid;
    if (n < a.N) {
      if (a.bias) const_b = a.bias[n];
      if (temb_uniform) const_t = a.temb[(size_t)(m_blk / a.HoWo) * a.temb_stride + n];
      if constexpr (LNF) const_c = a.ln_colsum[n];
    }
  }

  // residual tile of the final store loop, requested now (oldest VMEM ops: the ring's counted waits are unaffected)
  constexpr int RIT = BM * BN / 8 / 256;
  constexpr bool RES_PRE = !TRANS_OUT && GLDS && RIT <= 4 && DBG == 0;
  half8 resv[RES_PRE ? RIT : 1];
  const bool use_resv = RES_PRE && a.res_pre && a.res != nullptr && !a.slab && a.out_mode == kOutHalf && n_blk < a.n_trans && kg == 0;
  if constexpr (RES_PRE) {
    if (use_resv) {
#pragma unroll
      for (int it = 0; it < RIT; ++it) {
        const int idx = tid + it * 256;
        const int r = idx / (BN / 8), c = idx - r * (BN / 8);
        const int m = m_blk + r, n = n_blk + c * 8;
        const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        resv[it] = (m < a.M && n + 8 <= a.ldo) ? *reinterpret_cast<const half8*>(a.res + (size_t)m * a.ldo + n) : z;
      }
    }
  }
  if (prof) prof_t[1] = clock64();
  if constexpr (GLDS && NST >= 3) {
    // NST-stage ring: the DMA of tile kt+NST-1 is issued while tile kt is computed and tiles
    // kt+1 .. kt+NST-2 are still in flight (weight-streaming layers need the bytes in flight: at the
    // 8x8 / 16x16 levels every K step of a two-stage loop is one exposed HBM round trip).
    // Raw s_barrier + COUNTED vmcnt (a __syncthreads() would drain vmcnt(0) and serialise the ring,
    // cdna guide section 5 "Pipelining across barriers"); wait + barrier sit in one asm statement
    // with a memory clobber so no LDS access is scheduled across them.
    constexpr int PER_TILE = XR + WR;    // LDS-DMA instructions per wave per tile
    constexpr int DEPTH = NST - 2;       // tiles that may still be in flight while tile kt is computed
    static_assert(DEPTH * PER_TILE <= 63, "vmcnt range");
#pragma unroll
    for (int p = 0; p < NST - 1; ++p)
      if (kt_begin + p < kt_end) load_tile(p);
    for (int rel = 0; rel < kg_steps; ++rel) {
      const int kt = kt_begin + rel;
      if (KG == 2 && kt >= kt_end) {       // the shorter K half: keep the workgroup-wide barrier count (wave-uniform branch)
        asm volatile("s_barrier" ::: "memory");
        continue;
      }
      const int ahead = kt_end - 1 - kt;   // tiles after this one that are already issued (capped below)
      // wait until at most min(ahead, DEPTH) newer tiles are outstanding == tile kt has landed (loads of one
      // wave return in order); the immediate must be a literal, hence the ladder
      const int fly = ahead < DEPTH ? ahead : DEPTH;
      if (DEPTH >= 6 && fly == 6) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((DEPTH >= 6 ? 6 : 0) * PER_TILE) : "memory");
      else if (DEPTH >= 5 && fly == 5) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((DEPTH >= 5 ? 5 : 0) * PER_TILE) : "memory");
      else if (DEPTH >= 4 && fly == 4) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((DEPTH >= 4 ? 4 : 0) * PER_TILE) : "memory");
      else if (DEPTH >= 3 && fly == 3) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((DEPTH >= 3 ? 3 : 0) * PER_TILE) : "memory");
      else if (DEPTH >= 2 && fly == 2) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((DEPTH >= 2 ? 2 : 0) * PER_TILE) : "memory");
      else if (fly == 1) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(PER_TILE) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      read_frags(rel % NST);
      if (kt + NST - 1 < kt_end) load_tile((rel + NST - 1) % NST);
      mfma_step();
    }
  } else if constexpr (GLDS) {
    if (kt_begin < kt_end) load_tile(0);
    for (int kt = kt_begin; kt < kt_end; ++kt) {
      const int buf = (kt - kt_begin) & 1;
      // vmcnt(0) + barrier: this tile's DMA has landed for every wave, and every wave is done
      // reading the other stage, which the next DMA may now overwrite
      __syncthreads();
      read_frags(buf);
      if (kt + 1 < kt_end) load_tile(buf ^ 1);
      mfma_step();
    }
  } else {
    if (kt_begin < kt_end) {
      load_tile(0);
      store_tile(0);
    }
    __syncthreads();
    for (int kt = kt_begin; kt < kt_end; ++kt) {
      const int buf = (kt - kt_begin) & 1;
      const bool more = (kt + 1) < kt_end;
      read_frags(buf);
      if (more) load_tile(0);     // HBM/L2 latency hides under this tile's MFMAs
      mfma_step();
      if (more) store_tile(buf ^ 1);
      __syncthreads();
    }
  }

  if (prof) prof_t[2] = clock64();
  if constexpr (KG == 2) {
    // K group 1 hands its accumulators to group 0 through LDS (its own ring: every read of it is behind the barrier) and retires
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    floatx4* hx = reinterpret_cast<floatx4*>(smem + (size_t)NST * (BM + BN) * ROW * sizeof(half_t));   // group 1's ring
    static_assert((size_t)TM * TN * 4 * 256 * sizeof(floatx4) <= (size_t)NST * (BM + BN) * ROW * sizeof(half_t), "hand-over fits one ring");
    if (kg == 1) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            hx[((i * TN + j) * 4 + q) * 256 + tid] = floatx4{acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
    }
    __syncthreads();
    if (kg == 1) return;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const floatx4 v = hx[((i * TN + j) * 4 + q) * 256 + tid];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] += v[e];
        }
  }
  // ---------------------------------- epilogue ----------------------------------
  const int hi = lane >> 5;
  // LNF: y = rstd*(x.W') - rstd*mean*colsum + bias'  ->  out = acc*ln_a + ln_b*colsum[n] + bias[n]
  float ln_a[TM] = {}, ln_b[TM] = {};
  if constexpr (LNF) {
    const float inv_k = 1.0f / (float)a.K;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float s1 = xor32_sum(ln_s1[i]), s2 = xor32_sum(ln_s2[i]);   // the two k halves of the wave
      const float mean = s1 * inv_k;
      const float var = fmaxf(s2 * inv_k - mean * mean, 0.f);
      ln_a[i] = rsqrtf(var + a.ln_eps);
      ln_b[i] = -ln_a[i] * mean;
    }
  }
  if constexpr (TRANS_OUT) {
    // acc[i][j][r]: m = m0 + (r&3) + 8*(r>>2) + 4*hi ; n = n0 + (lane&31).  out[b][n][s]
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int n = n_blk + (wn * TN + j) * 32 + frow;
        const int m0 = m_blk + (wm * TM + i) * 32 + 4 * hi;
        if (n >= a.N) continue;
        const float bv = a.bias ? a.bias[n] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int m = m0 + 8 * q;
          if ((a.HoWo & 3) == 0 && (a.ldT & 3) == 0 && m + 3 < a.M) {   // 4 tokens of one image, 8-B aligned
            const int b = m / a.HoWo;
            const int s = m - b * a.HoWo;
            half4 o = {(half_t)(acc[i][j][4 * q] + bv), (half_t)(acc[i][j][4 * q + 1] + bv),
                       (half_t)(acc[i][j][4 * q + 2] + bv), (half_t)(acc[i][j][4 * q + 3] + bv)};
            *reinterpret_cast<half4*>(a.out + ((size_t)b * a.N + n) * a.ldT + s) = o;
            continue;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            int mm = m + e;
            if (mm < a.M) {
              int b = mm / a.HoWo;
              int s = mm - b * a.HoWo;
              a.out[((size_t)b * a.N + n) * a.ldT + s] = (half_t)(acc[i][j][4 * q + e] + bv);
            }
          }
        }
      }
    return;
  } else {
    tile_epilogue<BM, BN, WGM, WGN, TM, TN, LNF, (RES_PRE ? RIT : 0)>(a, acc, ln_a, ln_b, smem, sconst, const_b, const_t, const_c, m_blk,
                                                                      n_blk, wave, split, temb_uniform, resv, use_resv);
  }
  if (prof) {
    prof_t[3] = clock64();
    a.prof[0] = prof_t[0];
    a.prof[1] = prof_t[1];
    a.prof[2] = prof_t[2];
    a.prof[3] = prof_t[3];
    a.prof[4] = wall_clock64() - prof_w0;
  }
}

// ---------------------------------------------------------------------------------------------
// Software-pipelined 1x1 GEMM (every Linear / 1x1 conv of the transformer blocks and the resnet shortcuts at stride 1;
// unet.py:62-118, :566-617).  igemm_kernel above reads the 16 fragments of a K step, waits for them, then issues its 16
// MFMAs: with one wave per SIMD the LDS latency and the barrier are exposed once per step and the matrix pipe idles
// 50-75 % of the loop (245-520 TFLOP/s at UNet batch 16, profiles/r03_op_profile_b16_before.txt).  Here the loop body is the
// one of the K-split halo conv kernel:
//   * fragments are double-buffered in registers - between the MFMAs of step s the wave issues the ds_read_b128 of
//     step s+1 and the LDS-DMA of step s+D; the body is ONE basic block (no conditionals: tiles past the end of K go
//     through a zero-sized buffer resource), so sched_group_barrier fixes the interleaving MFMA / 2 reads ... MFMA / DMA;
//   * operands come HBM -> LDS by buffer_load_dwordx4 ... lds with loop-invariant per-lane offsets and a scalar K offset
//     (no vector address arithmetic in the loop; rows past M read zeros through the buffer range check; the second
//     source of a skip concat is a second resource selected per tile on the scalar unit);
//   * one raw s_barrier per step behind counted waits: lgkmcnt(0) (this wave holds step s in registers, so after the
//     barrier nobody reads ring stage s % D any more) and vmcnt((D-2) tiles) (tile s+1 has landed).
// Before the epilogue re-uses the LDS the wave drains vmcnt(0): an LDS-DMA still in flight when a workgroup hands its
// LDS back would land in whatever workgroup is dispatched there next.
// Accumulator layout, swizzle and epilogue are igemm_kernel's (tile_epilogue: bias / timestep embedding / LayerNorm fold /
// GEGLU / residual / fused q|k|v / GroupNorm statistics / split-K slabs).
// ---------------------------------------------------------------------------------------------
// DBG (ablation builds, tools/r5_gemm_ablation.py; results are garbage): bit 0 = no weight DMA, bit 1 = no activation DMA
// GNF (round 5): GroupNorm of the input folded in (SpatialTransformer.norm -> proj_in, unet.py:528-531 + :553-556: eps 1e-6, no
// SiLU).  The producer of x left (sum, sumsq) partials per (sample, group); every workgroup folds the ones of its sample (its M
// tile lies inside one sample) into a per-channel scale / shift table in LDS - requested as the oldest VMEM ops of the wave, in
// flight beside the first tiles' DMA - and each wave applies it to its activation fragments with v_pk_fma_f16 between the LDS
// read and the MFMA: what the GroupNorm kernel would have stored as fp16 is formed in registers instead, the launch and the
// activation round trip are gone.
// (the body is a device function so that gn_*_side_kernel can run it beside a GroupNorm in one launch: bid_in / split are what the
// stand-alone kernel takes from blockIdx.x / .y)
template <int BM, int BN, int WGM, int WGN, int D, bool LNF, int DBG = 0, bool GNF = false>
__device__ __forceinline__ void gemm_pipe_body(const IgemmArgs& a, int bid_in, int split) {
  static_assert(!(GNF && LNF), "one fold at a time");   // D = 2: 64 KB of LDS on the 128 x 128 tile, two workgroups per CU
  static_assert(WGM * WGN == 4, "4 waves");
  constexpr int TM = BM / WGM / 32, TN = BN / WGN / 32;
  constexpr int XR = BM / 32, WR = BN / 32, PER = ((DBG & 2) ? 0 : XR) + ((DBG & 1) ? 0 : WR), ROWB = BK * 2, KK = BK / 16;
  static_assert(DBG != 3, "one operand must still arrive");
  static_assert((D - 1) * PER <= 63, "vmcnt range");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Xs = smem;                                   // [D][BM][BK] halves
  char* const Ws = smem + D * BM * ROWB;                   // [D][BN][BK]
  float* sconst = reinterpret_cast<float*>(smem + (size_t)D * (BM + BN) * ROWB);
  // GNF: [64] mean | [64] rstd floats, then [K] mean | [K] scale | [K] shift halves, behind the epilogue constants
  float* gn_stat = sconst + 2 * BN;
  half_t* gn_tab = reinterpret_cast<half_t*>(gn_stat + 128);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int nbm = (a.M + BM - 1) / BM, nbn = (a.N + BN - 1) / BN;
  const int nwg = nbm * nbn;
  int bid = bid_in;
  {   // XCD-aware order (see igemm_kernel): each XCD walks a contiguous run of tiles sharing a weight panel
    int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    bid = base + idx;
  }
  const int bn_idx = a.n_fast ? bid % nbn : bid / nbm, bm_idx = a.n_fast ? bid / nbn : bid % nbm;
  const int m_blk = bm_idx * BM, n_blk = bn_idx * BN;
  const int kt_begin = split * a.nk_per_split;
  int kt_end = kt_begin + a.nk_per_split;
  if (kt_end > a.nk_total) kt_end = a.nk_total;
  const int T = kt_end - kt_begin;                          // K steps of this workgroup (>= 1: launch_conv leaves no empty split)

  constexpr unsigned kOob = 0x80000000u;
  const int pchunk = tid & 7, lrow = tid >> 3;
  const unsigned lchunk = (unsigned)(pchunk ^ ((lrow >> 1) & 7)) * 16u;   // logical 16-B chunk this lane fetches (bank swizzle)
  unsigned xoff0[XR], xoff1[XR], woff[WR];
#pragma unroll
  for (int i = 0; i < XR; ++i) {
    const int m = m_blk + lrow + 32 * i;
    xoff0[i] = m < a.M ? (unsigned)m * (unsigned)a.C0 * 2u + lchunk : kOob;
    xoff1[i] = m < a.M ? (unsigned)m * (unsigned)a.C1 * 2u + lchunk : kOob;
  }
#pragma unroll
  for (int i = 0; i < WR; ++i) {
    int n = n_blk + lrow + 32 * i;
    if (n > a.N - 1) n = a.N - 1;                           // rows past N: clamped (their outputs are never stored)
    woff[i] = (unsigned)n * (unsigned)a.K * 2u + lchunk;
  }
  const unsigned x0_bytes = (unsigned)((size_t)a.M * a.C0 * 2), x1_bytes = (unsigned)((size_t)a.M * a.C1 * 2);
  const unsigned w_bytes = (unsigned)((size_t)a.N * a.K * 2);

  int iw_kt = kt_begin, iw_stage = 0;                       // issue cursor of the ring
  auto issue_tile = [&]() {
    const bool live = iw_kt < kt_end;                       // wave-uniform; past the end: zero-sized resources, nothing is fetched
    const int k = iw_kt * BK;
    const bool second = k >= a.C0;                          // the skip-concat's second source (never with C1 == 0)
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<half_t*>(second ? a.x1 : a.x0), 0, (int)(live ? (second ? x1_bytes : x0_bytes) : 0u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(a.w), 0, (int)(live ? w_bytes : 0u), 0x00020000);
    const int xs_off = (second ? k - a.C0 : k) * 2;
    char* xs = Xs + iw_stage * (BM * ROWB) + wave * 1024;
    char* ws = Ws + iw_stage * (BN * ROWB) + wave * 1024;
    if constexpr ((DBG & 2) == 0) {
#pragma unroll
      for (int i = 0; i < XR; ++i) dma16_to_lds(rs_x, xs + i * 4096, second ? xoff1[i] : xoff0[i], xs_off);
    }
    if constexpr ((DBG & 1) == 0) {
#pragma unroll
      for (int i = 0; i < WR; ++i) dma16_to_lds(rs_w, ws + i * 4096, woff[i], k * 2);
    }
    ++iw_kt;
    iw_stage = (iw_stage + 1 == D) ? 0 : iw_stage + 1;
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float ln_s1[TM] = {}, ln_s2[TM] = {};

  const int frow = lane & 31, hi = lane >> 5;
  const int fsw = (frow >> 1) & 7;
  int foff[KK];                                             // byte offset of this lane's chunk of k sub-step kk inside a row
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) foff[kk] = ((kk * 2 + hi) ^ fsw) * 16;
  const int xrow = (wm * TM * 32 + frow) * ROWB, wrow = (wn * TN * 32 + frow) * ROWB;

  // per-column epilogue constants and the residual tile, requested before the first DMA (oldest VMEM ops of the wave)
  const bool temb_uniform = a.temb != nullptr && (a.HoWo % BM) == 0;
  float const_b = 0.f, const_t = 0.f, const_c = 0.f;
  if (!a.slab && tid < BN) {
    const int n = n_blk + tid;
    if (n < a.N) {
      if (a.bias) const_b = a.bias[n];
      if (temb_uniform) const_t = a.temb[(size_t)(m_blk / a.HoWo) * a.temb_stride + n];
      if constexpr (LNF) const_c = a.ln_colsum[n];
    }
  }
  constexpr int RIT = BM * BN / 8 / 256;
  constexpr bool RES_PRE = RIT <= 4;
  half8 resv[RES_PRE ? RIT : 1];
  const bool use_resv = RES_PRE && a.res_pre && a.res != nullptr && !a.slab && a.out_mode == kOutHalf && n_blk < a.n_trans;
  if constexpr (RES_PRE) {
    if (use_resv) {
#pragma unroll
      for (int it = 0; it < RIT; ++it) {
        const int idx = tid + it * 256;
        const int r = idx / (BN / 8), c = idx - r * (BN / 8);
        const int m = m_blk + r, n = n_blk + c * 8;
        const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        resv[it] = (m < a.M && n + 8 <= a.ldo) ? *reinterpret_cast<const half8*>(a.res + (size_t)m * a.ldo + n) : z;
      }
    }
  }

  struct Frags {
    half8 x[KK][TM];
    half8 w[KK][TN];
    half8 gm[GNF ? KK : 1], gs[GNF ? KK : 1], gh[GNF ? KK : 1];   // GNF: mean / scale / shift of this lane's 8 channels of every k sub-step
  };
  int rd_kt = kt_begin;                         // K step whose fragments the next read_step fetches (GNF table offset)
  auto read_step = [&](Frags& f, int stage) {
    const char* xs = Xs + stage * (BM * ROWB) + xrow;
    const char* ws = Ws + stage * (BN * ROWB) + wrow;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
      for (int i = 0; i < TM; ++i) f.x[kk][i] = *reinterpret_cast<const half8*>(xs + i * 32 * ROWB + foff[kk]);
#pragma unroll
      for (int j = 0; j < TN; ++j) f.w[kk][j] = *reinterpret_cast<const half8*>(ws + j * 32 * ROWB + foff[kk]);
      if constexpr (GNF) {
        const int k0 = rd_kt * BK + (kk * 2 + hi) * 8;
        f.gm[kk] = *reinterpret_cast<const half8*>(gn_tab + k0);
        f.gs[kk] = *reinterpret_cast<const half8*>(gn_tab + a.K + k0);
        f.gh[kk] = *reinterpret_cast<const half8*>(gn_tab + 2 * a.K + k0);
      }
    }
    ++rd_kt;
  };
  auto mfma_step = [&](const Frags& f) {
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        half8 xv = f.x[kk][i];
        // (x - fp16(mean)) * (rstd * gamma) + (beta - (mean - fp16(mean)) * rstd * gamma): the subtraction comes first so that every
        // rounding is relative to |x - mean|, not to |mean| (a group far from zero would otherwise lose digits in the shift)
        if constexpr (GNF) xv = __builtin_elementwise_fma(xv - f.gm[kk], f.gs[kk], f.gh[kk]);
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.w[kk][j], xv, acc[i][j], 0, 0, 0);
      }
      if constexpr (LNF) {   // row statistics of the A tile for the LayerNorm fold: VALU work in the MFMAs' issue shadow
        const half2v one2 = {(half_t)1.f, (half_t)1.f};
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const half2v p2 = {f.x[kk][i][2 * e], f.x[kk][i][2 * e + 1]};
            ln_s2[i] = __builtin_amdgcn_fdot2(p2, p2, ln_s2[i], false);
            ln_s1[i] = __builtin_amdgcn_fdot2(p2, one2, ln_s1[i], false);
          }
      }
    }
  };

  // GNF prologue, part 1 (before the first DMA: oldest VMEM ops of the wave): this sample's partial statistics - eight lanes
  // per group, 16 entries (8 float4) each, entries <= 128 - and gamma / beta of the channels whose table rows this thread writes
  floatx4 gnf_v[GNF ? 8 : 1];
  float gnf_g[GNF ? 8 : 1], gnf_b[GNF ? 8 : 1];
  if constexpr (GNF) {
    const int b = m_blk / a.HoWo;
    const int g = tid >> 3, j = tid & 7;
    const floatx4* src = reinterpret_cast<const floatx4*>(a.gnf_partial + (((size_t)b * a.gnf_G + (g < a.gnf_G ? g : 0)) * kGnMaxSlabs + j * 16) * 2);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int e0 = j * 16 + 2 * k;
      floatx4 v = {0.f, 0.f, 0.f, 0.f};
      if (e0 < a.gnf_entries) v = src[k];
      if (e0 + 1 >= a.gnf_entries) {
        v[2] = 0.f;
        v[3] = 0.f;
      }
      gnf_v[k] = v;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = tid + 256 * i;
      gnf_g[i] = k < a.K ? a.gnf_gamma[k] : 0.f;
      gnf_b[i] = k < a.K ? a.gnf_beta[k] : 0.f;
    }
  }
  Frags fA, fB;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    asm volatile("" ::: "memory");                          // keep the DMA issue order: the counted waits rely on it
    issue_tile();
  }
  if constexpr (GNF) {
    // part 2: fold (fixed order), statistics -> LDS, per-channel scale / shift table -> LDS; the barrier below publishes it
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s += gnf_v[k][0] + gnf_v[k][2];
      q += gnf_v[k][1] + gnf_v[k][3];
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
      s += __shfl_xor(s, o);
      q += __shfl_xor(q, o);
    }
    const int cpg = a.K / a.gnf_G;
    if ((tid & 7) == 0 && (tid >> 3) < a.gnf_G) {
      const float inv_n = 1.0f / ((float)cpg * (float)a.HoWo);
      const float mean = s * inv_n;
      gn_stat[tid >> 3] = mean;
      gn_stat[64 + (tid >> 3)] = rsqrtf(fmaxf(q * inv_n - mean * mean, 0.f) + a.gnf_eps);
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = tid + 256 * i;
      if (k < a.K) {
        const int g = k / cpg;
        const float sc = gnf_g[i] * gn_stat[64 + g];
        const half_t mh = (half_t)gn_stat[g];
        gn_tab[k] = mh;
        gn_tab[a.K + k] = (half_t)sc;
        gn_tab[2 * a.K + k] = (half_t)(gnf_b[i] - (gn_stat[g] - (float)mh) * sc);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  wait_vmcnt_barrier<(D - 1) * PER>();                      // tile 0 has landed for every wave (GNF: and the table is visible)
  read_step(fA, 0);
  int rd_stage = 0;                                         // ring stage of the step being multiplied
  auto body = [&](Frags& cur, Frags& nxt, auto last) {
    constexpr bool LAST = decltype(last)::value;
    if constexpr (LAST) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      mfma_step(cur);
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // this wave's fragments of the current step are in registers
      wait_vmcnt_barrier<(D - 2) * PER>();                  // the next tile has landed; nobody reads stage rd_stage any more
      const int nstage = (rd_stage + 1 == D) ? 0 : rd_stage + 1;
      read_step(nxt, nstage);                               // fragments of the next step -> the other register set
      issue_tile();                                         // tile (step + D) -> the stage just freed
      mfma_step(cur);
      rd_stage = nstage;
      if constexpr (!LNF && !GNF) {
        constexpr int NM = KK * TM * TN, NR = KK * (TM + TN);
        constexpr int RPM = (NR + NM / 2 - 1) / (NM / 2);   // reads behind each MFMA of the first half
#pragma unroll
        for (int g = 0; g < NM / 2; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, RPM, 0);
        }
#pragma unroll
        for (int g = 0; g < NM - NM / 2; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x010, (PER + NM - NM / 2 - 1) / (NM - NM / 2), 0);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  {
    using Tt = std::true_type;
    using Ff = std::false_type;
    int st = 0;
    for (; st + 2 < T; st += 2) {
      body(fA, fB, Ff{});
      body(fB, fA, Ff{});
    }
    if (T - st == 2) {
      body(fA, fB, Ff{});
      body(fB, fA, Tt{});
    } else {
      body(fA, fB, Tt{});
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the zero-sized tail DMAs too: the LDS is about to be re-used

  float ln_a[TM] = {}, ln_b[TM] = {};
  if constexpr (LNF) {
    const float inv_k = 1.0f / (float)a.K;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const float s1 = xor32_sum(ln_s1[i]), s2 = xor32_sum(ln_s2[i]);
      const float mean = s1 * inv_k;
      const float var = fmaxf(s2 * inv_k - mean * mean, 0.f);
      ln_a[i] = rsqrtf(var + a.ln_eps);
      ln_b[i] = -ln_a[i] * mean;
    }
  }
  tile_epilogue<BM, BN, WGM, WGN, TM, TN, LNF, (RES_PRE ? RIT : 0)>(a, acc, ln_a, ln_b, smem, sconst, const_b, const_t, const_c, m_blk,
                                                                    n_blk, wave, split, temb_uniform, resv, use_resv);
}

template <int BM, int BN, int WGM, int WGN, int D, bool LNF, int DBG = 0, bool GNF = false>
__global__ __launch_bounds__(256, D == 2 ? 2 : 1) void gemm_pipe_kernel(IgemmArgs a) {
  gemm_pipe_body<BM, BN, WGM, WGN, D, LNF, DBG, GNF>(a, blockIdx.x, blockIdx.y);
}

// ---------------------------------------------------------------------------------------------
// GroupNorm and an INDEPENDENT 1x1 GEMM side by side in one launch (round 5).  A resnet with a channel change (unet.py:470-489)
// runs norm1 -> conv1 -> norm2 -> conv2 on one chain and conv_shortcut(x) on another that meets it in conv2's residual add; as
// separate launches the 14 shortcut GEMMs of the SD2.1 step cost 10-20 us each and the norm1 launches beside them 8-23 us, each
// on a fraction of the chip (the single-launch GroupNorm runs on 64 workgroups, the shortcut GEMM at M = 512 on 160).  A side
// stream inside the captured graph costs more than it hides (round 4: fork / join pairs, +3.8 %).  Here ONE grid holds both:
// blocks [0, n_gn) run the GroupNorm body (gn_body.inc, the code of the stand-alone launch), blocks [n_gn_pad, ...) the pipelined
// GEMM body on the same input tensors (second reader: L2 / Infinity Cache hits).  No dependence between the two halves, no extra
// synchronisation; the consumer of both (conv1 / conv2) is a later launch as before.
// ---------------------------------------------------------------------------------------------
struct GnSideArgs {
  const half_t* x0;
  const half_t* x1;
  int C0, C1;
  const float* partial;
  int slabs;            // apply: entries to fold
  const float* gamma;
  const float* beta;
  half_t* y;
  int HW, G;
  float eps;
  int silu, pix_per_block;
  int gx, gy;           // the GroupNorm's own grid
  int n_gn_pad;         // first block of the GEMM half (n_gn rounded up to a multiple of 8: keeps the GEMM's XCD mapping)
};

template <int D>
__global__ __launch_bounds__(256) void gn_apply_side_kernel(GnSideArgs g, IgemmArgs a) {
  const int v = blockIdx.x;
  if (v < g.gx * g.gy) {
    groupnorm_apply_body(g.x0, g.C0, g.x1, g.C1, g.partial, g.slabs, g.gamma, g.beta, g.y, g.HW, g.G, g.eps, g.silu, g.pix_per_block,
                         v % g.gx, v / g.gx);
  } else if (v >= g.n_gn_pad) {
    gemm_pipe_body<64, 64, 2, 2, D, false>(a, v - g.n_gn_pad, 0);
  }
}

template <int VW, int D>
__global__ __launch_bounds__(256) void gn_fused_side_kernel(GnSideArgs g, IgemmArgs a) {
  const int v = blockIdx.x;
  if (v < g.gx * g.gy) {
    groupnorm_fused_body<VW, 256>(g.x0, g.C0, g.x1, g.C1, g.gamma, g.beta, g.y, g.HW, g.G, g.eps, g.silu, v % g.gx, v / g.gx);
  } else if (v >= g.n_gn_pad) {
    gemm_pipe_body<64, 64, 2, 2, D, false>(a, v - g.n_gn_pad, 0);
  }
}

// split-K combine + the same epilogue (bias, temb broadcast, residual) -> fp16.
// Round 5: every load of an item - up to eight slabs, bias, timestep embedding, residual - is requested before the first one is
// used (the slab loop with its run-time trip count paid one dependent round trip per slab and another for the epilogue operands:
// 4-6 in a row for 1 MB, 44 launches per step); summed in the slice order as before - bit-identical results.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(IgemmArgs a) {
  constexpr int SB = 8;
  const size_t total4 = (size_t)a.M * a.N / 4;
  const size_t slab = (size_t)a.M * a.N;
  const floatx4 z4 = {0.f, 0.f, 0.f, 0.f};
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total4;
       idx += (size_t)gridDim.x * blockDim.x) {
    const size_t e0 = idx * 4;
    const int m = (int)(e0 / a.N);
    const int n = (int)(e0 - (size_t)m * a.N);
    floatx4 p[SB];
#pragma unroll
    for (int z = 0; z < SB; ++z) p[z] = (z < a.splitk) ? *reinterpret_cast<const floatx4*>(a.partial + (size_t)z * slab + e0) : z4;
    const floatx4 bv = a.bias ? *reinterpret_cast<const floatx4*>(a.bias + n) : z4;
    const floatx4 tv = a.temb ? *reinterpret_cast<const floatx4*>(a.temb + (size_t)(m / a.HoWo) * a.temb_stride + n) : z4;
    const half4 hz = {0, 0, 0, 0};
    const half4 rr = a.res ? *reinterpret_cast<const half4*>(a.res + e0) : hz;
    floatx4 s = z4;
#pragma unroll
    for (int z = 0; z < SB; ++z)
      if (z < a.splitk) s += p[z];
    for (int z = SB; z < a.splitk; ++z) s += *reinterpret_cast<const floatx4*>(a.partial + (size_t)z * slab + e0);
    if (a.bias) s += bv;
    if (a.temb) s += tv;
    if (a.res) {
      s[0] += (float)rr[0];
      s[1] += (float)rr[1];
      s[2] += (float)rr[2];
      s[3] += (float)rr[3];
    }
    half4 o = {(half_t)s[0], (half_t)s[1], (half_t)s[2], (half_t)s[3]};
    out_store(reinterpret_cast<half4*>(a.out + e0), o);
  }
}

// The same combine for a tensor whose consumer is a GroupNorm (8x8 / 16x16 levels: every conv there is split-K or the
// weight-streaming kernel, so its GroupNorm statistics cannot come out of a tile epilogue): one workgroup per (PPB pixels of a
// sample) x all channels, per-(pixel, 4-channel quad) sums of the fp16-rounded outputs through LDS, then one thread per group adds
// its quads in a fixed order and writes entry blockIdx.x of gn_partial [B][G][kGnMaxSlabs][2] - the format the tile epilogues
// write, so the GroupNorm runs its fully parallel apply pass instead of the 64-workgroup two-pass kernel.
__global__ __launch_bounds__(256) void splitk_reduce_stats_kernel(IgemmArgs a, int ppb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* qs = reinterpret_cast<float*>(smem);            // [ppb][N / 4] (sum, sumsq) pairs
  const int NQ = a.N >> 2, t = threadIdx.x, b = blockIdx.y;
  const int p0 = blockIdx.x * ppb;
  const int items = ppb * NQ;
  for (int id = t; id < items; id += 256) {
    const int pl = id / NQ, qd = id - pl * NQ;
    const int p = p0 + pl;
    float fs = 0.f, fq = 0.f;
    if (p < a.HoWo) {
      const int m = b * a.HoWo + p, n = 4 * qd;
      const size_t e0 = (size_t)m * a.N + n;
      floatx4 s = {0.f, 0.f, 0.f, 0.f};
      for (int z = 0; z < a.splitk; ++z) s += *reinterpret_cast<const floatx4*>(a.partial + (size_t)z * a.M * a.N + e0);
      if (a.bias) s += *reinterpret_cast<const floatx4*>(a.bias + n);
      if (a.temb) s += *reinterpret_cast<const floatx4*>(a.temb + (size_t)b * a.temb_stride + n);
      if (a.res) {
        const half4 rr = *reinterpret_cast<const half4*>(a.res + e0);
        s[0] += (float)rr[0];
        s[1] += (float)rr[1];
        s[2] += (float)rr[2];
        s[3] += (float)rr[3];
      }
      const half4 o = {(half_t)s[0], (half_t)s[1], (half_t)s[2], (half_t)s[3]};
      out_store(reinterpret_cast<half4*>(a.out + e0), o);
      const float f0 = (float)o[0], f1 = (float)o[1], f2 = (float)o[2], f3 = (float)o[3];
      fs = (f0 + f1) + (f2 + f3);
      fq = fmaf(f0, f0, fmaf(f1, f1, fmaf(f2, f2, f3 * f3)));
    }
    qs[2 * id] = fs;
    qs[2 * id + 1] = fq;
  }
  __syncthreads();
  if (t < a.gn_G) {
    const int q0 = t * (a.gn_cpg >> 2), q1 = q0 + (a.gn_cpg >> 2);
    float s = 0.f, q = 0.f;
    for (int pl = 0; pl < ppb; ++pl)
      for (int qd = q0; qd < q1; ++qd) {
        s += qs[2 * (pl * NQ + qd)];
        q += qs[2 * (pl * NQ + qd) + 1];
      }
    float* dst = a.gn_partial + (((size_t)b * a.gn_G + t) * kGnMaxSlabs + blockIdx.x) * 2;
    dst[0] = s;
    dst[1] = q;
  }
}


template <int BM, int BN, int WGM, int WGN, bool TRANS, bool GLDS, int NST, bool LNF = false, int KG = 1>
void launch_variant(const IgemmArgs& a, hipStream_t s) {
  const size_t lds = (size_t)KG * NST * (BM + BN) * (GLDS ? BK : LDS_ROW) * sizeof(half_t) + 2 * BN * sizeof(float);
  static_assert(ring_fits(BM, BN, NST, KG), "LDS");
  static_assert((size_t)BN * (BM + 8) <= (size_t)NST * (BM + BN) * (GLDS ? BK : LDS_ROW), "transposed staging fits");
  static_assert((size_t)BM * (BN + 8) * 2 + 16 + (kGnScratchFloats + 2 * BN) * sizeof(float) <=
                    (size_t)NST * (BM + BN) * (GLDS ? BK : LDS_ROW) * sizeof(half_t),
                "GroupNorm statistics scratch fits behind the staged tile");
  dim3 grid(cdiv(a.M, BM) * cdiv(a.N, BN), a.splitk);
  auto k = igemm_kernel<BM, BN, WGM, WGN, TRANS, GLDS, NST, 0, LNF, KG>;
  static DynLdsOnce once;   // per instantiation, per device
  once.set(k, lds);
  hipLaunchKernelGGL(k, grid, dim3(256 * KG), lds, s, a);
}

template <int BM, int BN, int DBG>
void launch_debug(const IgemmArgs& a, hipStream_t s) {
  const size_t lds = (size_t)2 * (BM + BN) * BK * sizeof(half_t) + 2 * BN * sizeof(float);
  dim3 grid(cdiv(a.M, BM) * cdiv(a.N, BN), a.splitk);
  auto k = igemm_kernel<BM, BN, 2, 2, false, true, 2, DBG>;
  SD_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
}
template <int BM, int BN>
bool launch_debug_mode(const IgemmArgs& a, int dbg, hipStream_t s) {
  switch (dbg) {
    case 4: launch_debug<BM, BN, 4>(a, s); return true;
    case 5: launch_debug<BM, BN, 5>(a, s); return true;
    case 6: launch_debug<BM, BN, 6>(a, s); return true;
    case 14: launch_debug<BM, BN, 14>(a, s); return true;
    case 22: launch_debug<BM, BN, 22>(a, s); return true;
    case 30: launch_debug<BM, BN, 30>(a, s); return true;
    default: return false;
  }
}

// the software-pipelined 1x1 GEMM kernel with a ring of D stages (1x1, stride 1, non-transposed output; 32-bit buffer offsets)
template <int BM, int BN, int WGM, int WGN, int D, bool LNF>
void launch_pipe_dbg(const IgemmArgs& a, hipStream_t s) {   // ablation builds (a.debug = 64 + bits)
  constexpr size_t lds = (size_t)D * (BM + BN) * BK * sizeof(half_t) + 2 * BN * sizeof(float);
  dim3 grid(cdiv(a.M, BM) * cdiv(a.N, BN), a.splitk);
  if (a.debug == 65) {
    auto k = gemm_pipe_kernel<BM, BN, WGM, WGN, D, LNF, 1>;
    SD_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
  } else {
    auto k = gemm_pipe_kernel<BM, BN, WGM, WGN, D, LNF, 2>;
    SD_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
  }
}

template <int BM, int BN, int WGM, int WGN, int D, bool LNF>
void launch_pipe(const IgemmArgs& a, hipStream_t s) {
  constexpr size_t lds = (size_t)D * (BM + BN) * BK * sizeof(half_t) + 2 * BN * sizeof(float);
  static_assert(ring_fits(BM, BN, D), "LDS");
  static_assert((size_t)BM * (BN + 8) * 2 + 16 + (kGnScratchFloats + 2 * BN) * sizeof(float) <= (size_t)D * (BM + BN) * BK * sizeof(half_t),
                "staged tile + GroupNorm statistics scratch fit the K-loop buffers");
  static_assert((size_t)BN * (BM + 8) <= (size_t)D * (BM + BN) * BK, "transposed staging fits");
  dim3 grid(cdiv(a.M, BM) * cdiv(a.N, BN), a.splitk);
  if constexpr (D == 2 && !LNF) {   // the ablation builds exist for the 2-stage ring of the plain epilogue only
    if (a.debug == 65 || a.debug == 66) {
      launch_pipe_dbg<BM, BN, WGM, WGN, D, LNF>(a, s);
      return;
    }
  }
  if constexpr (BM == 64 && BN == 64 && !LNF) {   // GroupNorm-folded proj_in: 64 x 64 tile only (launch_conv routes it here)
    if (a.gnf_partial) {
      const size_t lds_g = lds + 128 * sizeof(float) + (size_t)3 * a.K * sizeof(half_t);
      auto kg = gemm_pipe_kernel<BM, BN, WGM, WGN, D, false, 0, true>;
      static DynLdsOnce once_g;
      once_g.set(kg, lds + 128 * sizeof(float) + (size_t)3 * 2048 * sizeof(half_t));   // K <= 2048 (launch_conv)
      hipLaunchKernelGGL(kg, grid, dim3(256), lds_g, s, a);
      return;
    }
  }
  auto k = gemm_pipe_kernel<BM, BN, WGM, WGN, D, LNF>;
  static DynLdsOnce once;
  once.set(k, lds);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, s, a);
}
// The instantiation the plan names (decode_plan resolved kernel, ring depth and K groups against the same ring_fits as the guards
// here): igemm_kernel's LDS-DMA ring of 2 / 3 / 4 / 6 / 8 stages, the same with two K groups of four waves (3 / 4 stages, plain
// epilogue), or gemm_pipe_kernel's ring of 2 / 3 / 4 stages.  false: no such kernel.
template <int BM, int BN, bool LNF, int NST>
bool launch_ring_depth(const IgemmArgs& a, const ConvPlan& p, hipStream_t s) {
  if constexpr (ring_fits(BM, BN, NST)) {
    if (p.kernel == ConvKernel::GemmPipe) {
      if constexpr (NST <= 4) { launch_pipe<BM, BN, 2, 2, NST, LNF>(a, s); return true; }
    } else if (p.kgroups == 2) {
      if constexpr (!LNF && (NST == 3 || NST == 4) && ring_fits(BM, BN, NST, 2)) { launch_variant<BM, BN, 2, 2, false, true, NST, false, 2>(a, s); return true; }
    } else {
      launch_variant<BM, BN, 2, 2, false, true, NST, LNF>(a, s);
      return true;
    }
  }
  return false;
}
template <int BM, int BN, bool LNF>
bool launch_ring(const IgemmArgs& a, const ConvPlan& p, hipStream_t s) {
  switch (p.stages) {
    case 2: return launch_ring_depth<BM, BN, LNF, 2>(a, p, s);
    case 3: return launch_ring_depth<BM, BN, LNF, 3>(a, p, s);
    case 4: return launch_ring_depth<BM, BN, LNF, 4>(a, p, s);
    case 6: return launch_ring_depth<BM, BN, LNF, 6>(a, p, s);
    case 8: return launch_ring_depth<BM, BN, LNF, 8>(a, p, s);
    default: return false;
  }
}

template <int BM, int BN>
void launch_tile(const IgemmArgs& a, const ConvPlan& p, bool trans, hipStream_t s) {
  bool ok = true;
  if (a.ln_colsum) ok = !p.reg_staged && launch_ring<BM, BN, true>(a, p, s);   // LayerNorm-folded 1x1 GEMM
  else if (trans && p.reg_staged) launch_variant<BM, BN, 2, 2, true, false, 2>(a, s);
  else if (trans && p.stages == 3) launch_variant<BM, BN, 2, 2, true, true, 3>(a, s);
  else if (trans) launch_variant<BM, BN, 2, 2, true, true, 2>(a, s);
  else if (p.reg_staged) launch_variant<BM, BN, 2, 2, false, false, 2>(a, s);
  else ok = launch_ring<BM, BN, false>(a, p, s);
  SD_REQUIRE(ok, kInternal, "no %dx%d kernel for plan '%s'", BM, BN, conv_plan_kernel_name(p).c_str());
}

// slab combine of a split-K / weight-streaming launch: plain, or - when the consumer is a GroupNorm over <= 256 pixels per sample -
// with the GroupNorm statistics of the result (returns the entries per (sample, group) it wrote, else 0)
int launch_slab_combine(const ConvDesc& d, IgemmArgs& a, hipStream_t s) {
  a.gn_partial = nullptr;
  if (conv_reduce_stats_on() && d.gn_partial && d.gn_groups >= 1 && d.gn_groups <= 256 && a.N % d.gn_groups == 0 && (a.N / d.gn_groups) % 4 == 0 &&
      a.HoWo <= 256 && d.out_mode == kOutHalf && !d.out_t) {
    int ppb = std::max(1, a.B * a.HoWo / 512);
    const int slabs = cdiv(a.HoWo, ppb);
    const size_t lds = (size_t)ppb * (a.N / 4) * 2 * sizeof(float);
    if (slabs <= kGnMaxSlabs && lds <= 64 * 1024) {
      a.gn_partial = d.gn_partial;
      a.gn_G = d.gn_groups;
      a.gn_cpg = a.N / d.gn_groups;
      a.gn_T = slabs;
      hipLaunchKernelGGL(splitk_reduce_stats_kernel, dim3(slabs, a.B), dim3(256), lds, s, a, ppb);
      return slabs;
    }
  }
  const size_t total4 = (size_t)a.M * a.N / 4;
  const int blocks = (int)std::min<size_t>((total4 + 255) / 256, 2048);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(256), 0, s, a);
  return 0;
}

half_t* g_zero_chunk = nullptr;

}  // namespace

// called where a handle is created (UNet, TextEncoder, the operator entry points' Scratch): never under graph capture
const half_t* device_zero_chunk() {
  if (!g_zero_chunk) {
    SD_HIP(hipMalloc(reinterpret_cast<void**>(&g_zero_chunk), 256));
    SD_HIP(hipMemset(g_zero_chunk, 0, 256));
    SD_HIP(hipDeviceSynchronize());
  }
  return g_zero_chunk;
}

const half_t* zero_chunk() {
  SD_REQUIRE(g_zero_chunk, kInternal, "conv launch before any handle allocated the zero chunk (device_zero_chunk)");
  return g_zero_chunk;
}

int launch_conv(const ConvDesc& d, const ConvWorkspace& ws, hipStream_t s) {
  SD_REQUIRE(conv_fast_path_ok(d), kInvalidArgument, "launch_conv: shape not MFMA-tileable (C0=%d C1=%d N=%d k=%d)",
             d.C0, d.C1, d.N, d.ksize);
  SD_REQUIRE(!d.ln_colsum || (d.ksize == 1 && !d.x1 && d.bias && d.out_mode != kOutHalfT), kInvalidArgument,
             "LayerNorm fold needs a 1x1 single-source GEMM with a (folded) bias");
  SD_REQUIRE(!d.out_t || (d.out_mode == kOutHalf && d.n_trans % 64 == 0 && d.n_trans < d.N && (d.Ho * d.Wo) % 8 == 0 &&
                          d.ldT % 8 == 0 && !d.res && !d.temb),
             kInvalidArgument, "fused q|k|v: n_trans %d N %d HoWo %d ldT %d", d.n_trans, d.N, d.Ho * d.Wo, d.ldT);
  SD_REQUIRE(!d.vt_perm || (d.out_t && (d.Ho * d.Wo) % 16 == 0), kInvalidArgument, "permuted V^T needs the fused q|k|v epilogue and HoWo %% 16 == 0");
  SD_REQUIRE(d.q_cols == 0 || (d.out_t && d.q_cols % 4 == 0 && d.q_cols <= d.n_trans), kInvalidArgument, "pre-scaled queries need the fused q|k|v epilogue (q_cols %d)", d.q_cols);
  const ConvPlan p = conv_plan(d);
  switch (p.kernel) {   // the kernels with their own argument blocks
    case ConvKernel::Wsgemm: launch_wsgemm(d, s); return 0;
    case ConvKernel::Bvgemm: launch_bvgemm(d, p, s); return 0;
    case ConvKernel::Smgemm: launch_smgemm(d, p, s); return 0;
    case ConvKernel::Smgeglu: launch_smgeglu(d, p, s); return 0;
    case ConvKernel::SmgegluPal: launch_smgeglu_pal(d, p, s); return 0;
    case ConvKernel::SmgemmPal: launch_smgemm_pal(d, p, s); return 0;   // (d.gn_partial set: no statistics, 0 entries - the GroupNorm runs its own pass)
    case ConvKernel::SmgemmI8: launch_smgemm_i8(d, p, s); return 0;     // (the same)
    case ConvKernel::SmgegluI8: launch_smgeglu_i8(d, p, s); return 0;
    case ConvKernel::SmgemmQ8: launch_smgemm_q8(d, p, s); return 0;
    case ConvKernel::SmqkvI8: launch_smqkv_i8(d, p, s); return 0;
    default: break;
  }
  IgemmArgs a = planned_args(d, p, ws.partial);
  const bool twins = d.n_twins > 0;
  SD_REQUIRE(!twins || (d.out_mode == kOutHalf && !d.ln_colsum && !d.out_t && !d.debug && reduce_twin_ok(a.HoWo, a.N, d.n_twins, d.twin)),
             kInvalidArgument, "GroupNorm twins need a plain fp16 output and whole (sample, group) slices (HoWo=%d N=%d)", a.HoWo, a.N);
  const bool have_ws = !p.slab || (ws.partial && ws.partial_bytes >= p.workspace_bytes);
  if (p.kernel == ConvKernel::Wstream || p.kernel == ConvKernel::WstreamPal || p.kernel == ConvKernel::WstreamI8) SD_REQUIRE(have_ws, kInternal, "wstream workspace too small (%zu < %zu)", ws.partial_bytes, p.workspace_bytes);
  SD_REQUIRE(have_ws, kInternal, "split-K workspace too small (%zu < %zu)", ws.partial_bytes, p.workspace_bytes);
  conv_plan_log(d, p);
  int gn_entries = 0;
  switch (p.kernel) {
    case ConvKernel::Wstream:      // weight-streaming kernel: slabs, then the group-organised combine (with the consumer's GroupNorm twins) or the plain one
      launch_wstream(d, ws.partial, p.waves, s);
      break;
    case ConvKernel::WstreamPal:   // the same slabs from palettized weights, then the same combine
      launch_wstream_pal(d, ws.partial, p.waves, s);
      break;
    case ConvKernel::WstreamI8:    // int8 weights and activations: exact int32 sums scaled into the same slabs, then the same combine
      launch_wstream_i8(d, ws.partial, p.waves, s);
      break;
    case ConvKernel::HaloKs: gn_entries = launch_halo_ks(d, p, ws.partial, s); break;
    case ConvKernel::HaloI8: gn_entries = launch_halo_i8(d, p, ws.partial, s); break;
    case ConvKernel::HaloPal: gn_entries = launch_halo_pal(d, p, ws.partial, s); break;   // the same body from palettized weights   // the same tiles from int8 weights and activations
    case ConvKernel::HaloSubpix: gn_entries = launch_halo_sp(d, p, ws.partial, s); break;   // the upsampler as four 2x2 phase convs on the low-res halo
    case ConvKernel::Igemm:
    case ConvKernel::GemmPipe: {
      const bool trans = d.out_mode == kOutHalfT;
      set_tile_order(a, p.bm, p.bn);
      if (d.debug && d.debug < 64) {   // ablation builds exist for two tiles only (tools/prof_conv.py)
        const bool ok = p.bm == 128 && p.bn == 128 ? launch_debug_mode<128, 128>(a, d.debug, s) : launch_debug_mode<64, 64>(a, d.debug, s);
        SD_REQUIRE(ok && !trans, kInvalidArgument, "no ablation kernel for debug mode %d", d.debug);
        return 0;
      }
      if (!trans) gn_entries = setup_gn_stats(d, a, p.bm);
      if (p.bm == 128 && p.bn == 128) launch_tile<128, 128>(a, p, trans, s);
      else if (p.bm == 128) launch_tile<128, 64>(a, p, trans, s);
      else if (p.bn == 64) launch_tile<64, 64>(a, p, trans, s);
      else launch_tile<64, 128>(a, p, trans, s);
      break;
    }
    default: SD_REQUIRE(false, kInternal, "launch_conv: plan '%s' has no launcher here", conv_plan_kernel_name(p).c_str());
  }
  if (twins) {
    launch_reduce_twin(a.partial, a.splitk, a.M, a.N, a.HoWo, a.bias, a.temb, a.temb_stride, a.res, a.out, d.n_twins, d.twin, s);
  } else if (a.slab) {
    gn_entries = launch_slab_combine(d, a, s);
  }
  SD_HIP(hipGetLastError());
  return gn_entries;
}

// ---- GroupNorm + independent 1x1 GEMM in one launch (gn_*_side_kernel) ----
bool gn_side_gemm_ok(const ConvDesc& d) {
  if (!(d.ksize == 1 && d.stride == 1 && d.up == 1 && d.out_mode == kOutHalf && !d.ln_colsum && !d.out_t && d.n_twins == 0 && !d.gnf_partial &&
        !d.gn_partial && !d.temb && !d.debug && conv_fast_path_ok(d)))
    return false;
  const int M = d.B * d.Ho * d.Wo, c1 = d.x1 ? d.C1 : 0;
  return gemm_pipe_ok(d.ksize, d.stride, d.up, M, d.N, d.C0 + c1, d.C0, c1) && M >= 256;   // (M = 128: the 8x8 level's shortcut GEMMs are split-K weight streams, a 40-workgroup side GEMM loses)
}

namespace {
constexpr int kSideD = 4;   // ring depth of the side GEMM: 64 KB + constants, the plan most shortcut shapes have stand-alone
IgemmArgs side_args(const ConvDesc& d) {
  SD_REQUIRE(gn_side_gemm_ok(d), kInvalidArgument, "side GEMM: not a plain 1x1 GEMM of the pipelined kernel (C0=%d C1=%d N=%d)", d.C0, d.C1, d.N);
  IgemmArgs a = make_args(d);
  a.splitk = 1;
  a.slab = 0;
  set_tile_order(a, 64, 64);
  return a;
}
constexpr size_t kSideLds = (size_t)kSideD * (64 + 64) * BK * sizeof(half_t) + 2 * 64 * sizeof(float);
}  // namespace

void launch_gn_apply_side(const half_t* x0, int C0, const half_t* x1, int C1, const float* partial, int entries, const float* gamma,
                          const float* beta, half_t* y, int B, int HW, int G, float eps, int silu, int slabs, int ppb, const ConvDesc& side,
                          hipStream_t s) {
  IgemmArgs a = side_args(side);
  GnSideArgs g{x0, x1, C0, x1 ? C1 : 0, partial, entries, gamma, beta, y, HW, G, eps, silu, ppb, slabs, B, 0};
  g.n_gn_pad = (slabs * B + 7) / 8 * 8;
  auto k = gn_apply_side_kernel<kSideD>;
  static DynLdsOnce once;
  once.set(k, kSideLds);
  hipLaunchKernelGGL(k, dim3(g.n_gn_pad + cdiv(a.M, 64) * cdiv(a.N, 64)), dim3(256), kSideLds, s, g, a);
  SD_HIP(hipGetLastError());
}

void launch_gn_fused_side(int vw, const half_t* x0, int C0, const half_t* x1, int C1, const float* gamma, const float* beta, half_t* y, int B,
                          int HW, int G, float eps, int silu, const ConvDesc& side, hipStream_t s) {
  IgemmArgs a = side_args(side);
  GnSideArgs g{x0, x1, C0, x1 ? C1 : 0, nullptr, 0, gamma, beta, y, HW, G, eps, silu, 0, G, B, 0};
  g.n_gn_pad = (G * B + 7) / 8 * 8;
  const dim3 grid(g.n_gn_pad + cdiv(a.M, 64) * cdiv(a.N, 64));
  static DynLdsOnce o8, o4, o2;
  if (vw == 8) {
    auto k = gn_fused_side_kernel<8, kSideD>;
    o8.set(k, kSideLds);
    hipLaunchKernelGGL(k, grid, dim3(256), kSideLds, s, g, a);
  } else if (vw == 4) {
    auto k = gn_fused_side_kernel<4, kSideD>;
    o4.set(k, kSideLds);
    hipLaunchKernelGGL(k, grid, dim3(256), kSideLds, s, g, a);
  } else {
    auto k = gn_fused_side_kernel<2, kSideD>;
    o2.set(k, kSideLds);
    hipLaunchKernelGGL(k, grid, dim3(256), kSideLds, s, g, a);
  }
  SD_HIP(hipGetLastError());
}

}  // namespace sd
