// The epilogue of the fp16-accumulating 3x3 / stride-1 halo kernels - conv3x3_halo_ks_kernel (plan tile 7), conv3x3_halo_sp_kernel
// (plan tile 21), conv3x3_halo_pal_kernel (plan tile 25): the ONE statement of it.  A textual fragment, #included inside the kernel
// body behind the __syncthreads() that ends the K loop - not a function: a force-inlined function template is simplified before it is
// inlined and moved the scalar prologue (and, at D = 4, the tap loop) of every tile-7 instantiation; as text the three kernels compile
// to what their own copies compiled to, instruction for instruction (LAB_NOTES.md round 35, tools/isa_compare.py).
// The int8 kernel (plan tile 18, conv3x3_halo_i8.hip) has its own epilogue: int32 exchange, fp32 staging, one rounding.
//
// Reads from the enclosing kernel:
//   a (IgemmArgs), smem, sconst, acc (floatx16 [2][2]), const_b, const_t, tid, lane, wave, wm, wk, frow, hi, n_blk, b, ty, tx, y0, x0,
//   H, W (the image the 8x16 tile grid lies on), split, BN, BM.
// The includer defines in front of the #include and #undefs behind it:
//   HALO_OUT_PIXEL(y, x)  row of a.out / a.res / a slab that pixel (y, x) of the tile grid's image goes to
//                         (tiles 7 and 25: (b * H + y) * W + x; tile 21: pixel (2 y + pa, 2 x + pb) of the 2H x 2W image).
//                         A product whose first factor is parenthesised, NOT parenthesised as a whole: the store loop widens that
//                         first factor with a (size_t) cast in front of the expansion, as the three copies did.
//   HALO_GN_STATS         true / false: whether the kernel leaves GroupNorm statistics when a.gn_partial is set (tile 21: false)
// LDS (every includer static_asserts that its K-loop buffers cover it): [0, 32 KB) the K-half exchange, later the GroupNorm scratch;
// behind it [BM][BN + 8] halves of output staging; sconst ([BN] floats) outside both.
//
// acc[i][j][r]: n = j*32 + (r&3) + 8*(r>>2) + 4*hi ; pixel block 2*wm + i, pixel frow

  // sum the two K halves: wave (wm, wk) keeps pixel block 2*wm + wk and hands the other one to its partner
  {
    floatx4* red = reinterpret_cast<floatx4*>(smem);      // [4 waves][2 j][4 q][64 lanes] = 32 KB
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        floatx4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = wk ? acc[0][j][4 * q + e] : acc[1][j][4 * q + e];
        red[((wave * 2 + j) * 4 + q) * 64 + lane] = v;
      }
    if (tid < BN) sconst[tid] = const_b + const_t;
    __syncthreads();
  }
  floatx16 fin[2];
  {
    const floatx4* red = reinterpret_cast<const floatx4*>(smem);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const floatx4 v = red[(((wave ^ 1) * 2 + j) * 4 + q) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) fin[j][4 * q + e] = (wk ? acc[1][j][4 * q + e] : acc[0][j][4 * q + e]) + v[e];
      }
  }
  const int ml = (wm * 2 + wk) * 32 + frow;               // tile-local pixel of this lane
  if (a.slab) {
    const int y = y0 + (ml >> 4), x = x0 + (ml & 15);
    if (y < H && x < W) {
      const int m = HALO_OUT_PIXEL(y, x);
      float* prow = a.partial + ((size_t)split * a.M + m) * a.N;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int n = n_blk + j * 32 + 8 * q + 4 * hi;
          if (n < a.N) {
            floatx4 v = {fin[j][4 * q], fin[j][4 * q + 1], fin[j][4 * q + 2], fin[j][4 * q + 3]};
            out_store(reinterpret_cast<floatx4*>(prow + n), v);
          }
        }
    }
    return;
  }
  constexpr int OROW = BN + 8;
  half_t* ot = reinterpret_cast<half_t*>(smem + 32 * 1024);   // [BM][OROW], behind the reduction buffer
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int nl = j * 32 + 8 * q + 4 * hi;
      const floatx4 bb = *reinterpret_cast<const floatx4*>(sconst + nl);   // 0 beyond N
      half4 o = {(half_t)(fin[j][4 * q] + bb[0]), (half_t)(fin[j][4 * q + 1] + bb[1]), (half_t)(fin[j][4 * q + 2] + bb[2]),
                 (half_t)(fin[j][4 * q + 3] + bb[3])};
      *reinterpret_cast<half4*>(ot + ml * OROW + nl) = o;
    }
  __syncthreads();
  constexpr int WC = BN / 8;
  const bool gn = HALO_GN_STATS && a.gn_partial != nullptr;   // block-uniform (launch_conv: N % 8 == 0)
  float fs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, fq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int idx = tid; idx < BM * WC; idx += 256) {
    const int r = idx / WC, c = idx - r * WC;
    const int y = y0 + (r >> 4), x = x0 + (r & 15);
    const int n = n_blk + c * 8;
    if (y < H && x < W && n < a.N) {
      const size_t m = (size_t)HALO_OUT_PIXEL(y, x);
      half8 v = *reinterpret_cast<const half8*>(ot + r * OROW + c * 8);
      half_t* dst = a.out + m * a.N + n;
      if (n + 8 <= a.N) {
        if (a.res) {
          const half8 rr = *reinterpret_cast<const half8*>(a.res + m * a.N + n);
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
      } else {
        for (int e = 0; e < a.N - n; ++e) dst[e] = a.res ? (half_t)((float)v[e] + (float)a.res[m * a.N + n + e]) : v[e];
      }
    }
  }
  // GroupNorm statistics of the stored pixels (only those inside the image); the scratch is the K-half reduction
  // buffer at the start of the LDS, which nobody reads after the barrier above
  if (gn) tile_gn_stats<BN>(a, reinterpret_cast<float*>(smem), fs, fq, n_blk, b, ty * a.tiles_x + tx);
