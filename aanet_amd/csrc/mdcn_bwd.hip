// mdcn_bwd.hip -- the training backward for gfx950: the modulated deformable convolution's data /
// offset / mask gradients (global, channels-last and LDS-window forms), the weight-gradient kernel
// it shares with the plain convolution (aanet_conv2d_wgrad_f32), the deterministic fixed-point
// helpers, and every aanet_*bwd* / workspace-size entry point.
#include "mdcn_common.h"

#include <cstdio>
#include <stdlib.h>

namespace {

using namespace mdcn;  // NT, PT, KC, CP

// the backward's timing switch: a kernel argument in the debug build, a compile-time 0 otherwise
// (so the product kernels carry no branch for it)
__device__ __forceinline__ int bwd_dbg(const MdcnArgs &a) {
#ifdef AANET_DEBUG_SWITCHES
  return a.dbg_noatom;
#else
  (void)a;
  return 0;
#endif
}

// (1) data/coordinate gradients.  Workgroup = (image n, 64-pixel tile, deformable group g);
// groups == 1.  gOut tile [Co][64] is staged in LDS once; per (tap k, <=32-channel chunk)
// colg = W^T gOut is formed by MFMA into LDS (the reference's `columns` never touches HBM),
// then each thread (pixel, channel subset) accumulates grad_mask / grad_offset partials
// (kernel.cu:695-767) and scatters grad_x to the 4 bilinear corners (kernel.cu:635-693,
// float atomics like the reference).
// DET: grad_x is accumulated in 64-bit fixed point (value * scale, scale a power of two chosen
// on the device from a bound on any single contribution, det_scale_kernel).  Integer adds are
// associative, so the sum -- and the fp32 grad_x converted from it -- does not depend on the
// order in which the atomics land: the deterministic backward of torch's
// use_deterministic_algorithms (the reference's col2im atomics, kernel.cu:688, are not).
// NHS (float atomics only): grad_x is scattered into an NHWC workspace [N][H*W][C] with the lanes
// of a wave on 32 consecutive channels of a corner -- each atomic instruction covers two fully used
// 128-byte lines, where the NCHW form (lanes = pixels with data-dependent corners) spreads one
// instruction over a dozen partly used lines; nhwc_to_nchw_kernel then writes grad_x.
template <int DET, int NHS = 0>
__global__ __launch_bounds__(NT) void mdcn_bwd_data_kernel(MdcnArgs a, const float *__restrict__ gout,
                                                           float *__restrict__ gx,
                                                           float *__restrict__ goff,
                                                           float *__restrict__ gmask, int GP,
                                                           int WTP, long long *__restrict__ gxi,
                                                           const double *__restrict__ det_scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int Co = a.Co;
  float *sG = sm;                       // [Co][GP]      gOut tile
  float *sWt = sG + Co * GP;            // [KC][WTP]     W^T chunk
  float *sCg = sWt + KC * WTP;          // [KC][CP]      colg chunk
  float *sRed = sCg + KC * CP;          // [3][4][64]    cross-wave reduction
  float *sS = sRed + 3 * 4 * 64;        // [PT][12]      NHS: per-pixel corners, weights, mask

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long P = (long)a.Ho * a.Wo;
  const int ntiles = (int)((P + PT - 1) / PT);
  const int n = blockIdx.x / ntiles, tile = blockIdx.x % ntiles, g = blockIdx.y;
  const int K = a.kh * a.kw, cpg = a.C / a.dg, C = a.C;
  const long p = (long)tile * PT + lane;
  const bool pvalid = p < P;
  const int ho = pvalid ? (int)(p / a.Wo) : 0, wo = pvalid ? (int)(p % a.Wo) : 0;
  const long HW = (long)a.H * a.W;
  const float *xn = a.x + (long)n * C * HW;
  float *gxn = gx + (long)n * C * HW;
  long long *gxin = DET ? gxi + (long)n * C * HW : nullptr;
  const double scale = DET ? *det_scale : 1.0;
  auto scatter = [&](long idx, float v) {
    if (DET)
      atomicAdd(reinterpret_cast<unsigned long long *>(gxin + idx),
                (unsigned long long)__double2ll_rn((double)v * scale));
    else
      atomicAdd(gxn + idx, v);
  };

  for (int e = tid; e < Co * PT; e += NT) {
    const int co = e / PT, pl = e % PT;
    const long pp = (long)tile * PT + pl;
    sG[co * GP + pl] = pp < P ? gout[((long)n * Co + co) * P + pp] : 0.f;
  }

  const int kr = lane >> 4, jj = lane & 15;
  for (int k = 0; k < K; ++k) {
    Samp s;
    pixel_samp(s, a, n, g, k, pvalid ? p : 0, ho, wo);
    float gm = 0.f, goh = 0.f, gow = 0.f;
    if (NHS && wave == 0) {  // published for the chunk loop (its first barrier orders it)
#pragma clang fp contract(off)
      const bool on = pvalid && s.valid;
      const float hh = 1.f - s.lh, hw = 1.f - s.lw;
      float *q = sS + lane * 12;
      q[0] = __builtin_bit_cast(float, on && (s.ok & 1) ? s.i1 : -1);
      q[1] = __builtin_bit_cast(float, on && (s.ok & 2) ? s.i2 : -1);
      q[2] = __builtin_bit_cast(float, on && (s.ok & 4) ? s.i3 : -1);
      q[3] = __builtin_bit_cast(float, on && (s.ok & 8) ? s.i4 : -1);
      q[4] = hh * hw, q[5] = hh * s.lw, q[6] = s.lh * hw, q[7] = s.lh * s.lw;
      q[8] = s.m;
    }
    for (int c0 = g * cpg; c0 < (g + 1) * cpg; c0 += KC) {
      const int rows = min(KC, (g + 1) * cpg - c0);
      __syncthreads();  // previous chunk's sCg / sWt readers are done
      for (int e = tid; e < KC * Co; e += NT) {
        const int cl = e % KC, co = e / KC;
        sWt[cl * WTP + co] = cl < rows ? a.weight[((long)co * C + c0 + cl) * K + k] : 0.f;
      }
      __syncthreads();
      // colg[c][px] = sum_co W[co][c][k] gOut[co][px]: 2 channel blocks x this wave's 16 px.
      f32x4 cacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      for (int ks = 0; ks < Co / 4; ++ks) {
        const float bv = sG[(4 * ks + kr) * GP + 16 * wave + jj];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          const float av = sWt[(16 * cb + jj) * WTP + 4 * ks + kr];
          cacc[cb] = mfma16x16x4(av, bv, cacc[cb]);
        }
      }
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) sCg[(16 * cb + 4 * kr + r) * CP + 16 * wave + jj] = cacc[cb][r];
      __syncthreads();
      if (pvalid && s.valid) {
#pragma unroll 2
        for (int ii = 0; ii < KC / 4; ++ii) {
          const int cl = wave + 4 * ii;
          if (cl >= rows) break;
          const int c = c0 + cl;
          const float cg = sCg[cl * CP + lane];
          const float *im = xn + (long)c * HW;
          const float v1 = (s.ok & 1) ? im[s.i1] : 0.f, v2 = (s.ok & 2) ? im[s.i2] : 0.f;
          const float v3 = (s.ok & 4) ? im[s.i3] : 0.f, v4 = (s.ok & 8) ? im[s.i4] : 0.f;
          const float hh = 1.f - s.lh, hw = 1.f - s.lw;
          const float val = hh * hw * v1 + hh * s.lw * v2 + s.lh * hw * v3 + s.lh * s.lw * v4;
          gm += cg * val;
          const float wh = -hw * v1 - s.lw * v2 + hw * v3 + s.lw * v4;
          const float ww = -hh * v1 + hh * v2 - s.lh * v3 + s.lh * v4;
          const float top = cg * s.m;
          goh += wh * top;
          gow += ww * top;
          if (NHS) continue;
          const long cb = (long)c * HW;
          if (s.ok & 1) scatter(cb + s.i1, hh * hw * top);
          if (s.ok & 2) scatter(cb + s.i2, hh * s.lw * top);
          if (s.ok & 4) scatter(cb + s.i3, s.lh * hw * top);
          if (s.ok & 8) scatter(cb + s.i4, s.lh * s.lw * top);
        }
      }
      if (NHS) {
        // lanes 0-31: channel cl of pixel 16w + 2t, lanes 32-63: of pixel 16w + 2t + 1
        const int cl = lane & 31;
        if (cl < rows) {
          const long cbase = (long)n * HW * C + c0 + cl;
          auto nadd = [&](int i, float v) {
            if (DET)
              atomicAdd(reinterpret_cast<unsigned long long *>(gxi + cbase + (long)i * C),
                        (unsigned long long)__double2ll_rn((double)v * scale));
            else
              atomicAdd(gx + cbase + (long)i * C, v);
          };
#pragma unroll 2
          for (int t = 0; t < 8; ++t) {
#pragma clang fp contract(off)
            const int px = 16 * wave + 2 * t + (lane >> 5);
            const float *q = sS + px * 12;
            const f32x4 qi = *reinterpret_cast<const f32x4 *>(q);
            const f32x4 qw = *reinterpret_cast<const f32x4 *>(q + 4);
            const float top = sCg[cl * CP + px] * q[8];
            const float qi0 = qi[0], qi1 = qi[1], qi2 = qi[2], qi3 = qi[3];  // (bit_cast of an
            const int i1 = __builtin_bit_cast(int, qi0), i2 = __builtin_bit_cast(int, qi1);  // element
            const int i3 = __builtin_bit_cast(int, qi2), i4 = __builtin_bit_cast(int, qi3);  // lvalue)
            if (i1 >= 0) nadd(i1, qw[0] * top);
            if (i2 >= 0) nadd(i2, qw[1] * top);
            if (i3 >= 0) nadd(i3, qw[2] * top);
            if (i4 >= 0) nadd(i4, qw[3] * top);
          }
        }
      }
    }
    // reduce the 4 waves' channel partials for each pixel
    sRed[(0 * 4 + wave) * 64 + lane] = gm;
    sRed[(1 * 4 + wave) * 64 + lane] = goh;
    sRed[(2 * 4 + wave) * 64 + lane] = gow;
    __syncthreads();
    if (wave == 0 && pvalid) {
      float t0 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        t0 += sRed[(0 * 4 + q) * 64 + lane];
        t1 += sRed[(1 * 4 + q) * 64 + lane];
        t2 += sRed[(2 * 4 + q) * 64 + lane];
      }
      const long ob = (long)n * a.dg * 2 * K * P + (long)g * 2 * K * P;
      goff[ob + (long)(2 * k) * P + p] = t1;
      goff[ob + (long)(2 * k + 1) * P + p] = t2;
      gmask[(long)n * a.dg * K * P + ((long)g * K + k) * P + p] = t0;
    }
  }
}

// (1b) the same data/coordinate gradients from channels-last copies: x as [N][H*W][C] and the
// weight as wT[k][c][co] (both made by the launcher into the workspace), for C % 4 == 0 and
// C/dg % 4 == 0.  Workgroup = (image n, 64-pixel tile, deformable group g).  Per (tap, chunk):
//  - the W^T chunk is staged with coalesced rows of wT, colg = W^T gOut by MFMA into LDS;
//  - offset/mask partials: thread = (pixel, channel quad), each corner one 16-byte load of 4
//    channels (8 lanes = one 128-B line of a corner), reduced over the 8 quads by shuffles;
//  - grad_x: lanes on 32 consecutive channels of a corner, atomics into the NHWC accumulator.
template <int DET>
__global__ __launch_bounds__(NT) void mdcn_bwd_data_nhwc_kernel(MdcnArgs a, const float *__restrict__ xh,
                                                                const float *__restrict__ wT,
                                                                const float *__restrict__ gout,
                                                                float *__restrict__ gx,
                                                                float *__restrict__ goff,
                                                                float *__restrict__ gmask, int GP,
                                                                int WTP, long long *__restrict__ gxi,
                                                                const double *__restrict__ det_scale) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int Co = a.Co;
  float *sG = sm;                       // [Co][GP]      gOut tile
  float *sWt = sG + Co * GP;            // [KC][WTP]     W^T chunk
  float *sCg = sWt + KC * WTP;          // [KC][CP]      colg chunk
  float *sS = sCg + KC * CP;            // [PT][12]      per-pixel corners, weights, mask, fractions
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long P = (long)a.Ho * a.Wo;
  const int ntiles = (int)((P + PT - 1) / PT);
  const int n = blockIdx.x / ntiles, tile = blockIdx.x % ntiles, g = blockIdx.y;
  const int K = a.kh * a.kw, cpg = a.C / a.dg, C = a.C;
  const long HW = (long)a.H * a.W;
  const double scale = DET ? *det_scale : 1.0;
  const float *xn = xh + (long)n * HW * C;

  for (int e = tid; e < Co * PT; e += NT) {
    const int co = e / PT, pl = e % PT;
    const long pp = (long)tile * PT + pl;
    sG[co * GP + pl] = pp < P ? gout[((long)n * Co + co) * P + pp] : 0.f;
  }
  const int kr = lane >> 4, jj = lane & 15;
  const int q = tid & 7;  // channel quad of the gradient role; pixels (tid >> 3) + 32 it
  for (int k = 0; k < K; ++k) {
    if (k) __syncthreads();  // every wave is done scattering tap k-1 (it reads sS)
    if (wave == 0) {  // published for the chunk loop (its first barrier orders it)
#pragma clang fp contract(off)
      const long p = (long)tile * PT + lane;
      const bool pvalid = p < P;
      Samp s;
      pixel_samp(s, a, n, g, k, pvalid ? p : 0, pvalid ? (int)(p / a.Wo) : 0, pvalid ? (int)(p % a.Wo) : 0);
      const bool on = pvalid && s.valid;
      const float hh = 1.f - s.lh, hw = 1.f - s.lw;
      float *qq = sS + lane * 12;
      qq[0] = __builtin_bit_cast(float, on && (s.ok & 1) ? s.i1 : -1);
      qq[1] = __builtin_bit_cast(float, on && (s.ok & 2) ? s.i2 : -1);
      qq[2] = __builtin_bit_cast(float, on && (s.ok & 4) ? s.i3 : -1);
      qq[3] = __builtin_bit_cast(float, on && (s.ok & 8) ? s.i4 : -1);
      qq[4] = hh * hw, qq[5] = hh * s.lw, qq[6] = s.lh * hw, qq[7] = s.lh * s.lw;
      // an invalid sample's fractions are 0, not h - (float)(int)h (inf or NaN for an offset of
      // +-inf or +-3e38): its corners read as 0, and 0 * inf would put NaN where the reference
      // has grad_offset = grad_mask = 0 (kernel.cu:716-721)
      qq[8] = s.m, qq[9] = on ? s.lh : 0.f, qq[10] = on ? s.lw : 0.f, qq[11] = on ? 1.f : 0.f;
    }
    float gm[2] = {0.f, 0.f}, goh[2] = {0.f, 0.f}, gow[2] = {0.f, 0.f};
    for (int c0 = g * cpg; c0 < (g + 1) * cpg; c0 += KC) {
      const int rows = min(KC, (g + 1) * cpg - c0);
      __syncthreads();  // previous chunk's sCg / sWt readers are done
      for (int e = tid; e < KC * Co; e += NT) {
        const int co = e % Co, cl = e / Co;
        sWt[cl * WTP + co] = cl < rows ? wT[((long)k * C + c0 + cl) * Co + co] : 0.f;
      }
      __syncthreads();
      f32x4 cacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
      for (int ks = 0; ks < Co / 4; ++ks) {
        const float bv = sG[(4 * ks + kr) * GP + 16 * wave + jj];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          const float av = sWt[(16 * cb + jj) * WTP + 4 * ks + kr];
          cacc[cb] = mfma16x16x4(av, bv, cacc[cb]);
        }
      }
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) sCg[(16 * cb + 4 * kr + r) * CP + 16 * wave + jj] = cacc[cb][r];
      __syncthreads();
      // offset / mask partials: (pixel, channel quad)
      if (4 * q < rows) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
#pragma clang fp contract(off)
          const int px = (tid >> 3) + 32 * it;
          const float *qq = sS + px * 12;
          const f32x4 qi = *reinterpret_cast<const f32x4 *>(qq);
          const float qi0 = qi[0], qi1 = qi[1], qi2 = qi[2], qi3 = qi[3];
          const int i1 = __builtin_bit_cast(int, qi0), i2 = __builtin_bit_cast(int, qi1);
          const int i3 = __builtin_bit_cast(int, qi2), i4 = __builtin_bit_cast(int, qi3);
          const float m = qq[8], lh = qq[9], lw = qq[10];
          const float hh = 1.f - lh, hw = 1.f - lw;
          const int cq = c0 + 4 * q;
          const f32x4 z = {0.f, 0.f, 0.f, 0.f};
          const f32x4 v1 = i1 >= 0 ? *reinterpret_cast<const f32x4 *>(xn + (long)i1 * C + cq) : z;
          const f32x4 v2 = i2 >= 0 ? *reinterpret_cast<const f32x4 *>(xn + (long)i2 * C + cq) : z;
          const f32x4 v3 = i3 >= 0 ? *reinterpret_cast<const f32x4 *>(xn + (long)i3 * C + cq) : z;
          const f32x4 v4 = i4 >= 0 ? *reinterpret_cast<const f32x4 *>(xn + (long)i4 * C + cq) : z;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float cg = sCg[(4 * q + u) * CP + px];
            const float val = hh * hw * v1[u] + hh * lw * v2[u] + lh * hw * v3[u] + lh * lw * v4[u];
            gm[it] += cg * val;
            const float wh = -hw * v1[u] - lw * v2[u] + hw * v3[u] + lw * v4[u];
            const float ww = -hh * v1[u] + hh * v2[u] - lh * v3[u] + lh * v4[u];
            const float top = cg * m;
            goh[it] += wh * top;
            gow[it] += ww * top;
          }
        }
      }
      // grad_x: lanes 0-31 channel cl of pixel 16w + 2t, lanes 32-63 of pixel 16w + 2t + 1
      const int cl = lane & 31;
      if (cl < rows && !bwd_dbg(a)) {
        const long cbase = (long)n * HW * C + c0 + cl;
        auto nadd = [&](int i, float v) {
          if (DET)
            atomicAdd(reinterpret_cast<unsigned long long *>(gxi + cbase + (long)i * C),
                      (unsigned long long)__double2ll_rn((double)v * scale));
          else
            atomicAdd(gx + cbase + (long)i * C, v);
        };
#pragma unroll 2
        for (int t = 0; t < 8; ++t) {
#pragma clang fp contract(off)
          const int px = 16 * wave + 2 * t + (lane >> 5);
          const float *qq = sS + px * 12;
          const f32x4 qi = *reinterpret_cast<const f32x4 *>(qq);
          const f32x4 qw = *reinterpret_cast<const f32x4 *>(qq + 4);
          const float top = sCg[cl * CP + px] * qq[8];
          const float qi0 = qi[0], qi1 = qi[1], qi2 = qi[2], qi3 = qi[3];
          const int i1 = __builtin_bit_cast(int, qi0), i2 = __builtin_bit_cast(int, qi1);
          const int i3 = __builtin_bit_cast(int, qi2), i4 = __builtin_bit_cast(int, qi3);
          if (i1 >= 0) nadd(i1, qw[0] * top);
          if (i2 >= 0) nadd(i2, qw[1] * top);
          if (i3 >= 0) nadd(i3, qw[2] * top);
          if (i4 >= 0) nadd(i4, qw[3] * top);
        }
      }
    }
    // reduce the 8 channel quads of each pixel (lanes 8j .. 8j+7), fixed order
#pragma unroll
    for (int it = 0; it < 2; ++it) {
#pragma unroll
      for (int msk = 1; msk < 8; msk <<= 1) {
        gm[it] += __shfl_xor(gm[it], msk);
        goh[it] += __shfl_xor(goh[it], msk);
        gow[it] += __shfl_xor(gow[it], msk);
      }
      const long p = (long)tile * PT + (tid >> 3) + 32 * it;
      if (q == 0 && p < P) {
        const long ob = (long)n * a.dg * 2 * K * P + (long)g * 2 * K * P;
        goff[ob + (long)(2 * k) * P + p] = goh[it];
        goff[ob + (long)(2 * k + 1) * P + p] = gow[it];
        gmask[(long)n * a.dg * K * P + ((long)g * K + k) * P + p] = gm[it];
      }
    }
  }
}

// Window form of mdcn_bwd_data_nhwc_kernel (stride 1 or 2, <= 128 channels per deformable group,
// K <= 9 taps, <= 128 output channels; round 6 added the feature extractor's stride-2, 64-channel
// group, Co = 128 shapes).  The workgroup owns an 8 x 8 output tile and one deformable group, and walks the
// group's channels in 16-channel slices: per slice it sums the grad_x corner contributions in an
// LDS copy of the tile's input window (rows/cols [origin, origin + WR/WC): the corners of every
// offset in [-R, R)), then adds the window to the global accumulator once -- one global add per
// window element instead of one per (pixel, tap, corner, channel).  Corners outside the window
// take a global atomic directly.
// The window is INT64 FIXED POINT in both modes (scale 2^(38 - ceil(log2 bound)), computed on
// the device by det_scale_kernel): an LDS ds_add_u64 costs ~26 cycles per wave-instruction per CU
// against ~196 for ds_add_f32 (tools/lds_rmw_lab.hip, profiles/r04_lds_scatter_probe.txt), and
// the integer sums do not depend on the order.  The 16-channel slice keeps the window at 32 KB
// (two workgroups per CU).  DET: the window and the out-of-window corners go to the int64 global
// accumulator (bit-reproducible); otherwise the window is converted once to float and added with
// float atomics (its per-tile sums are exact to 2^-38 of the bound before that one rounding).
// grad_offset / grad_mask: the first slice's per-(tap, pixel) channel sums wait in LDS (sP) and
// the last slice adds its own and stores the result -- no atomics, fixed order.
// Taps are software-pipelined: the raw offsets / mask of the next tap (wave 0, lane = pixel) and
// this thread's elements of the next tap's W^T slice are loaded into registers one tap ahead.
// Round 4 also tried an atomic-free "owner computes" form (per-tap tables of the pixels whose
// corner block starts at each window position): bit-reproducible, but slower -- agg_s0 backward
// 7.84 ms float / 8.20 ms fixed point: the owner loop is a chain of dependent LDS reads per window
// position and tap.  It is in the git history (round 4).
// FUSEW (float mode): the weight gradient of the tile rides along -- the sampled column values
// (the forward's (w1 v1 + w2 v2 + w3 v3 + w4 v4) * mask, from the corner quads the offset / mask
// partials load anyway) go to LDS, one 16x16x4 f32 MFMA run per (tap, slice) forms the tile's
// [64 co][16 c] product with the staged gOut tile, and it is added with float atomics into a
// [K][Co][C] accumulator (64-byte segments; transposed into grad_weight afterwards).  DET: the
// same products go to an int64 fixed-point [K][Co][C] accumulator (scale det_scale[1]), so the sum
// does not depend on the order of the tiles and the workspace holds one copy of the weight
// gradient (round 4 stored a float partial per tile and reduced them in a fixed order: ~0.08 ms
// faster at agg_s0, but ~0.9 GB of workspace at B = 8).  This replaces mdcn_bwd_weight_kernel,
// whose 18 chunks each re-read gOut and re-gathered the corners.
// dynamic LDS: sG [Co][GP], sWt [16][WTP], sCg [16][WCP], sS [PT][16], sP [3][9][PT],
// [FUSEW: sCol [16][WCP]], window [WR*WC][16] int64
constexpr int WHC = 16;  // channels per window slice
// row pitch of the colg / column tiles of the window kernel: 66 (= 2 mod 32) makes the partials'
// (rows 4q+u, lanes q), the scatter's and the fused weight gradient's (rows = lane % 16) reads
// conflict-free; the engine's CP = 80 left them 4- to 8-way conflicted
constexpr int WCP = PT + 2;
constexpr int WKMAX = 9; // taps the sP partial buffer holds
constexpr int WCOMAX = 128;  // output channels (the W^T slice is prefetched in registers)
constexpr int GW_COPIES = 8; // copies of the fused weight-gradient accumulator, summed afterwards
template <int DET, int FUSEW = 0>
__global__ __launch_bounds__(NT, 2) void mdcn_bwd_data_win_kernel(MdcnArgs a, const float *__restrict__ xh,
                                                               const float *__restrict__ wT,
                                                               const float *__restrict__ gout,
                                                               float *__restrict__ gx,
                                                               float *__restrict__ goff,
                                                               float *__restrict__ gmask, int GP,
                                                               int WTP, long long *__restrict__ gxi,
                                                               const double *__restrict__ det_scale,
                                                               int WR, int WCc, int R,
                                                               float *__restrict__ gwT = nullptr,
                                                               long long *__restrict__ gwi = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int Co = a.Co;
  float *sG = sm;                       // [Co][GP]      gOut tile
  float *sWt = sG + Co * GP;            // [16][WTP]     W^T slice
  float *sCg = sWt + WHC * WTP;         // [16][WCP]      colg slice
  float *sS = sCg + WHC * WCP;           // [PT][16]      per-pixel corners, weights, mask, window pos
  float *sP = sS + PT * 16;             // [3][WKMAX][PT] first slice's grad_offset / mask sums
  float *sCol = sP + 3 * WKMAX * PT;    // [16][WCP]      sampled columns (FUSEW)
  long long *sAcc = reinterpret_cast<long long *>(sCol + (FUSEW ? WHC * WCP : 0));  // [WR*WC][16]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long P = (long)a.Ho * a.Wo;
  const int ttx = (a.Wo + 7) / 8, tpi = ttx * ((a.Ho + 7) / 8);
  const int K = a.kh * a.kw, cpg = a.C / a.dg, C = a.C;
  const int NH = (cpg + WHC - 1) / WHC;
  const int n = blockIdx.x / tpi, tile = blockIdx.x % tpi, g = blockIdx.y;
  const int ty0 = (tile / ttx) * 8, tx0 = (tile % ttx) * 8;
  const long HW = (long)a.H * a.W;
  const double scale = *det_scale;
  const double inv = 1.0 / scale;
  const double wscale = DET && FUSEW ? det_scale[1] : 1.0;  // the weight gradient's fixed point
  // the weight-gradient accumulator copy of this workgroup (consecutive workgroups run on
  // different XCDs: one copy per XCD keeps the atomics on one element from crossing them)
  const long gwc = (long)(blockIdx.x & (GW_COPIES - 1)) * K * Co * C;
  const float *xn = xh + (long)n * HW * C;
  // window origin: the tile's first input row / column (stride s: 8 output pixels span 7s + 1)
  const int wy0 = ty0 * a.stride - a.pad - R, wx0 = tx0 * a.stride - a.pad - R;
  const int nwin = WR * WCc * WHC;
  auto pix = [&](int pl) -> long {  // linear output pixel of tile pixel pl, or -1
    const int y = ty0 + (pl >> 3), x = tx0 + (pl & 7);
    return (y < a.Ho && x < a.Wo) ? (long)y * a.Wo + x : -1;
  };
  for (int e = tid; e < Co * PT; e += NT) {
    const int co = e / PT, pl = e % PT;
    const long pp = pix(pl);
    sG[co * GP + pl] = pp >= 0 ? gout[((long)n * Co + co) * P + pp] : 0.f;
  }
  const int kr = lane >> 4, jj = lane & 15;
  const int q = tid & 3, qpx = tid >> 2;  // gradient role: channel quad q of pixel qpx
  const long sp = pix(lane);
  const int sy = sp >= 0 ? (int)(sp / a.Wo) : 0, sx = sp >= 0 ? (int)(sp % a.Wo) : 0;
  const float *offg = a.offset + (long)n * a.off_bs + (long)g * 2 * K * P + (sp >= 0 ? sp : 0);
  constexpr int WPT = WHC * WCOMAX / NT;  // W^T slice elements per thread
  float roh = 0.f, row = 0.f, rm = 0.f, rw[WPT];
  auto prefetch = [&](int kk, int c0) {  // tap kk's offsets / mask and W^T rows c0 .. c0+15
    if (wave == 0) {
      roh = offg[(long)(2 * kk) * P];
      row = offg[(long)(2 * kk + 1) * P];
      rm = a.mask[(long)n * a.mask_bs + ((long)g * K + kk) * P + (sp >= 0 ? sp : 0)];
    }
    const int nr = min(WHC, (g + 1) * cpg - c0);
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      const int e = tid + NT * j, co = e % Co, cl = e / Co;
      rw[j] = (e < WHC * Co && cl < nr) ? wT[((long)kk * C + c0 + cl) * Co + co] : 0.f;
    }
  };
  prefetch(0, g * cpg);
  for (int sl = 0; sl < NH; ++sl) {
    const int cb0 = g * cpg + sl * WHC, rows = min(WHC, (g + 1) * cpg - cb0);
    const bool last = sl == NH - 1;
    for (int e = tid; e < nwin; e += NT) sAcc[e] = 0;  // ordered by the first tap's barrier
    for (int k = 0; k < K; ++k) {
      __syncthreads();  // every wave is done with tap k-1 (sS, sWt, sCg) and the last flush
      if (wave == 0) {
#pragma clang fp contract(off)
        const bool pvalid = sp >= 0;
        const int i = k / a.kw, j = k % a.kw;
        const float m = a.mask_logits ? a.mask_scale * (1.f / (1.f + expf(-rm))) : rm;  // deform.py:86-89
        Samp s;
        make_samp(s, (float)(sy * a.stride - a.pad + i * a.dil) + roh,
                  (float)(sx * a.stride - a.pad + j * a.dil) + row, a.H, a.W, m);
        const bool on = pvalid && s.valid;
        float *qq = sS + lane * 16;
        qq[0] = __builtin_bit_cast(float, on && (s.ok & 1) ? s.i1 : -1);
        qq[1] = __builtin_bit_cast(float, on && (s.ok & 2) ? s.i2 : -1);
        qq[2] = __builtin_bit_cast(float, on && (s.ok & 4) ? s.i3 : -1);
        qq[3] = __builtin_bit_cast(float, on && (s.ok & 8) ? s.i4 : -1);
        // make_samp's own weights (0 for a corner outside the image, the same products else) and
        // fractions 0 for an invalid sample: h - (float)(int)h is inf or NaN for an offset of +-inf
        // or +-3e38, and 0 * inf would put NaN into the sampled columns (grad_weight) and where
        // the reference has grad_offset = grad_mask = 0 (kernel.cu:716-721)
        qq[4] = s.w1, qq[5] = s.w2, qq[6] = s.w3, qq[7] = s.w4;
        qq[8] = s.m, qq[9] = on ? s.lh : 0.f, qq[10] = on ? s.lw : 0.f, qq[11] = on ? 1.f : 0.f;
        // window position of the 2x2 corner block (top-left), or -1: global atomics
        int wpos = -1;
        if (on) {
          const int rh = s.hl - wy0, rw_ = s.wl - wx0;
          if ((unsigned)rh <= (unsigned)(WR - 2) && (unsigned)rw_ <= (unsigned)(WCc - 2)) wpos = rh * WCc + rw_;
        }
        qq[12] = __builtin_bit_cast(float, wpos);
      }
#pragma unroll
      for (int j = 0; j < WPT; ++j) {
        const int e = tid + NT * j, co = e % Co, cl = e / Co;
        if (e < WHC * Co) sWt[cl * WTP + co] = rw[j];
      }
      if (k + 1 < K)
        prefetch(k + 1, cb0);
      else if (!last)
        prefetch(0, cb0 + WHC);
      __syncthreads();
      // corner quads of the offset / mask partials (pixel qpx, channel quad q), issued before the
      // colg MFMAs so their latency overlaps them
      const float *qq = sS + qpx * 16;
      const f32x4 qi = *reinterpret_cast<const f32x4 *>(qq);
      const float qi0 = qi[0], qi1 = qi[1], qi2 = qi[2], qi3 = qi[3];
      const int i1 = __builtin_bit_cast(int, qi0), i2 = __builtin_bit_cast(int, qi1);
      const int i3 = __builtin_bit_cast(int, qi2), i4 = __builtin_bit_cast(int, qi3);
      const bool qon = 4 * q < rows;
      const int cq = cb0 + 4 * q;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const f32x4 v1 = qon && i1 >= 0 ? *reinterpret_cast<const f32x4 *>(xn + (long)i1 * C + cq) : z;
      const f32x4 v2 = qon && i2 >= 0 ? *reinterpret_cast<const f32x4 *>(xn + (long)i2 * C + cq) : z;
      const f32x4 v3 = qon && i3 >= 0 ? *reinterpret_cast<const f32x4 *>(xn + (long)i3 * C + cq) : z;
      const f32x4 v4 = qon && i4 >= 0 ? *reinterpret_cast<const f32x4 *>(xn + (long)i4 * C + cq) : z;
      f32x4 cacc = {0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < Co / 4; ++ks) {
        const float bv = sG[(4 * ks + kr) * GP + 16 * wave + jj];
        const float av = sWt[jj * WTP + 4 * ks + kr];
        cacc = mfma16x16x4(av, bv, cacc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) sCg[(4 * kr + r) * WCP + 16 * wave + jj] = cacc[r];
      if constexpr (FUSEW) {
#pragma clang fp contract(off)
        // the forward's sampled value (samp_val order) times the mask; zeros past the slice
        const f32x4 wq = *reinterpret_cast<const f32x4 *>(qq + 4);
        const float mq = qq[8];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          sCol[(4 * q + u) * WCP + qpx] = (wq[0] * v1[u] + wq[1] * v2[u] + wq[2] * v3[u] + wq[3] * v4[u]) * mq;
      }
      __syncthreads();
      if constexpr (FUSEW) {
        // this tile's weight-gradient block: wave w = output channels cbk + 16w .. + 15 for each
        // 64-channel block cbk (Co <= 128, Co % 16 == 0: whole blocks), the slice's 16 channels,
        // K = the tile's 64 pixels; one float atomic per element into gwT[k][co][c]
        for (int cbk = 0; cbk < Co; cbk += 64) {
          const int cw = cbk + 16 * wave;  // wave-uniform
          if (cw >= Co) break;
          f32x4 wacc = {0.f, 0.f, 0.f, 0.f};
          for (int ks = 0; ks < PT / 4; ++ks) {
            const float av = sG[(cw + jj) * GP + 4 * ks + kr];
            const float bv = sCol[jj * WCP + 4 * ks + kr];
            wacc = mfma16x16x4(av, bv, wacc);
          }
          if (jj < rows) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int co = cw + 4 * kr + r;
              if (DET)  // int64 fixed point: the sum does not depend on the order of the tiles
                atomicAdd(reinterpret_cast<unsigned long long *>(gwi) + gwc + ((long)k * Co + co) * C + cb0 + jj,
                          (unsigned long long)__double2ll_rn((double)wacc[r] * wscale));
              else
                atomicAdd(gwT + gwc + ((long)k * Co + co) * C + cb0 + jj, wacc[r]);
            }
          }
        }
      }
      float gm = 0.f, goh = 0.f, gow = 0.f;
      if (qon) {
#pragma clang fp contract(off)
        const float m = qq[8], lh = qq[9], lw = qq[10];
        const float hh = 1.f - lh, hw = 1.f - lw;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float cg = sCg[(4 * q + u) * WCP + qpx];
          const float val = hh * hw * v1[u] + hh * lw * v2[u] + lh * hw * v3[u] + lh * lw * v4[u];
          gm += cg * val;
          const float wh = -hw * v1[u] - lw * v2[u] + hw * v3[u] + lw * v4[u];
          const float ww = -hh * v1[u] + hh * v2[u] - lh * v3[u] + lh * v4[u];
          const float top = cg * m;
          goh += wh * top;
          gow += ww * top;
        }
      }
      // grad_x: lane (pixel 16 w + 4 t + lane / 16, channel lane % 16)
      const int cl = lane & 15;
      if (cl < rows && bwd_dbg(a) != 1) {
        const long cbase = (long)n * HW * C + cb0 + cl;
#pragma unroll 2
        for (int t = 0; t < 4; ++t) {
#pragma clang fp contract(off)
          const int px = 16 * wave + 4 * t + (lane >> 4);
          const float *qp = sS + px * 16;
          const f32x4 pi = *reinterpret_cast<const f32x4 *>(qp);
          const f32x4 qw = *reinterpret_cast<const f32x4 *>(qp + 4);
          const float top = sCg[cl * WCP + px] * qp[8];
          const float pi0 = pi[0], pi1 = pi[1], pi2 = pi[2], pi3 = pi[3], q12 = qp[12];
          const int j1 = __builtin_bit_cast(int, pi0), j2 = __builtin_bit_cast(int, pi1);
          const int j3 = __builtin_bit_cast(int, pi2), j4 = __builtin_bit_cast(int, pi3);
          const int wp = __builtin_bit_cast(int, q12);
          if (wp >= 0) {  // corners outside the image have index -1 (skipped), as below
            unsigned long long *w0 = reinterpret_cast<unsigned long long *>(sAcc) + (long)wp * WHC + cl;
            if (j1 >= 0) atomicAdd(w0, (unsigned long long)__double2ll_rn((double)(qw[0] * top) * scale));
            if (j2 >= 0) atomicAdd(w0 + WHC, (unsigned long long)__double2ll_rn((double)(qw[1] * top) * scale));
            if (j3 >= 0) atomicAdd(w0 + WCc * WHC, (unsigned long long)__double2ll_rn((double)(qw[2] * top) * scale));
            if (j4 >= 0) atomicAdd(w0 + (WCc + 1) * WHC, (unsigned long long)__double2ll_rn((double)(qw[3] * top) * scale));
          } else {
            auto gadd = [&](int i, float v) {
              if (DET)
                atomicAdd(reinterpret_cast<unsigned long long *>(gxi + cbase + (long)i * C),
                          (unsigned long long)__double2ll_rn((double)v * scale));
              else
                atomicAdd(gx + cbase + (long)i * C, v);
            };
            if (j1 >= 0) gadd(j1, qw[0] * top);
            if (j2 >= 0) gadd(j2, qw[1] * top);
            if (j3 >= 0) gadd(j3, qw[2] * top);
            if (j4 >= 0) gadd(j4, qw[3] * top);
          }
        }
      }
      // reduce the 4 channel quads of each pixel (lanes 4j .. 4j+3), fixed order; the first
      // slice parks its sums in sP, the last adds them (slice order) and stores
#pragma unroll
      for (int msk = 1; msk < 4; msk <<= 1) {
        gm += __shfl_xor(gm, msk);
        goh += __shfl_xor(goh, msk);
        gow += __shfl_xor(gow, msk);
      }
      if (q == 0) {
        float *pp = sP + k * PT + qpx;
        if (sl > 0) {
          goh = pp[0] + goh;
          gow = pp[WKMAX * PT] + gow;
          gm = pp[2 * WKMAX * PT] + gm;
        }
        if (!last) {
          pp[0] = goh, pp[WKMAX * PT] = gow, pp[2 * WKMAX * PT] = gm;
        } else {
          const long p = pix(qpx);
          if (p >= 0) {
            const long ob = (long)n * a.dg * 2 * K * P + (long)g * 2 * K * P;
            goff[ob + (long)(2 * k) * P + p] = goh;
            goff[ob + (long)(2 * k + 1) * P + p] = gow;
            gmask[(long)n * a.dg * K * P + ((long)g * K + k) * P + p] = gm;
          }
        }
      }
    }
    __syncthreads();  // the slice's window is complete
    if (bwd_dbg(a)) continue;
    // add the window to the global accumulator: consecutive threads take consecutive channels of a
    // position (16 lanes = one 64-byte (float) / 128-byte (int64) segment); zero elements skipped
    for (int e = tid; e < nwin; e += NT) {
      const int pos = e / WHC, wc = e - pos * WHC;
      const int gy = wy0 + pos / WCc, gxp = wx0 + pos % WCc;
      if (wc >= rows || gy < 0 || gy >= a.H || gxp < 0 || gxp >= a.W) continue;
      const long o = ((long)n * HW + (long)gy * a.W + gxp) * C + cb0 + wc;
      const long long v = sAcc[e];
      // a non-finite bound (scale = NaN) converts every contribution to 0: add the NaN read-back
      // anyway (float mode), so grad_x is poisoned like the reference's float col2im
      if (!v && (DET || inv == inv)) continue;
      if (DET)
        atomicAdd(reinterpret_cast<unsigned long long *>(gxi + o), (unsigned long long)v);
      else
        atomicAdd(gx + o, (float)((double)v * inv));
    }
  }
}

// grad_weight [Co][C][K] += gwi [K][Co][C] / scale (the deterministic window form's int64
// fixed-point weight-gradient accumulator; NaN scale -> NaN, as det_scale_kernel says)
__global__ __launch_bounds__(256) void det_gw_final_kernel(const long long *__restrict__ gwi,
                                                           float *__restrict__ gw, int Co, int C, int K,
                                                           const double *__restrict__ wscale) {
  const long nw = (long)Co * C * K;
  const double inv = 1.0 / *wscale;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nw; e += (long)gridDim.x * 256) {
    const int k = (int)(e % K), c = (int)((e / K) % C), co = (int)(e / ((long)K * C));
    long long v = 0;
#pragma unroll
    for (int j = 0; j < GW_COPIES; ++j) v += gwi[j * nw + ((long)k * Co + co) * C + c];
    gw[e] += (float)((double)v * inv);
  }
}

// grad_weight [Co][C][K] += gwT [K][Co][C] (the fused window form's accumulator)
__global__ __launch_bounds__(256) void gw_kcoc_add_kernel(const float *__restrict__ gwT,
                                                          float *__restrict__ gw, int Co, int C, int K) {
  const long nw = (long)Co * C * K;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < nw; e += (long)gridDim.x * 256) {
    const int k = (int)(e % K), c = (int)((e / K) % C), co = (int)(e / ((long)K * C));
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < GW_COPIES; ++j) v += gwT[j * nw + ((long)k * Co + co) * C + c];
    gw[e] += v;
  }
}

// x [N][C][HW] -> [N][HW][C] and w [Co][C][K] -> wT [K][C][Co] (inputs of mdcn_bwd_data_nhwc_kernel)
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float *__restrict__ src,
                                                           float *__restrict__ dst, int C, long HW) {
  __shared__ float t[32][33];
  const int n = blockIdx.z;
  const long s0 = (long)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float *sn = src + (long)n * C * HW;
  float *dn = dst + (long)n * HW * C;
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r;
    t[r][tx] = (c < C && s0 + tx < HW) ? sn[(long)c * HW + s0 + tx] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const long sp = s0 + r;
    if (sp < HW && c0 + tx < C) dn[sp * C + c0 + tx] = t[tx][r];
  }
}

__global__ __launch_bounds__(256) void weight_kcco_kernel(const float *__restrict__ w,
                                                          float *__restrict__ wT, int Co, int C, int K) {
  const long n = (long)Co * C * K;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const int co = (int)(e % Co), c = (int)((e / Co) % C), k = (int)(e / ((long)Co * C));
    wT[e] = w[((long)co * C + c) * K + k];
  }
}

// (2) weight gradient: gW[co][c][k] += sum_{n,p} gOut[n][co][p] * col[c*K+k][n,p].
// Workgroup = one K chunk (tap k, <=32 channels of group g) x one range of pixels (all
// images flattened) x one 64-wide output-channel tile.  The col chunk is re-sampled into LDS
// per 64-pixel sub-tile, the [co][c] tile accumulates in MFMA registers across the whole
// pixel range, then one float atomic per element (grad accumulates, cpp:660-669).
// DET: each pixel-range split writes its partial sums to part[split][co][c][k] (no atomics);
// det_weight_reduce_kernel adds them to grad_weight in split order.
// NR: the col chunk is sampled from the channels-last copy xh [N][H*W][C] (C, C/dg % 4 == 0):
// thread = (pixel, channel quad), one 16-byte load per corner (8 lanes = one 128-B line); the
// sub-tile loop is software-pipelined (see the NR branch).
// PLAIN: the weight gradient of an ordinary (grouped) convolution (aanet_conv2d_wgrad_f32): the
// col chunk is the tap's shifted window of x (zero outside), a.dg carries the conv's groups,
// grad_weight is [Co][C/groups][K] and output-channel tiles stay inside the chunk's group.
template <int DET, int NR = 0, int PLAIN = 0>
__global__ __launch_bounds__(NT) void mdcn_bwd_weight_kernel(MdcnArgs a, const float *__restrict__ gout,
                                                             float *__restrict__ gw, int npieces,
                                                             long range, float *__restrict__ part,
                                                             const float *__restrict__ xh = nullptr) {
  constexpr int GP2 = PT + 2;  // A/B reads (16 rows x 4 cols per 16 lanes) conflict-free
  __shared__ __attribute__((aligned(16))) float sG[64 * GP2];
  __shared__ __attribute__((aligned(16))) float sC[KC * GP2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long P = (long)a.Ho * a.Wo, T = (long)a.N * P;
  const int K = a.kh * a.kw, cpg = a.C / a.dg, C = a.C, Co = a.Co;
  const int chunk = blockIdx.x;
  const int k = chunk / (a.dg * npieces), rem = chunk % (a.dg * npieces);
  const int g = rem / npieces, piece = rem % npieces;
  const int c0 = g * cpg + piece * KC, rows = min(KC, (g + 1) * cpg - c0);
  const int cog = PLAIN ? Co / a.dg : Co;  // output channels of the chunk's group
  const int co0 = (PLAIN ? g * cog : 0) + blockIdx.z * 64, coE = PLAIN ? (g + 1) * cog : Co;
  const int Cw = PLAIN ? cpg : C, cw0 = PLAIN ? c0 - g * cpg : c0;  // grad_weight's [co][c] view
  const long r0 = (long)blockIdx.y * range, r1 = min(r0 + range, T);
  const long HW = (long)a.H * a.W;
  const int kr = lane >> 4, jj = lane & 15;
  // wave w: output-channel block w (16 co), both 16-channel blocks of the chunk
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if constexpr (PLAIN) {
    // software-pipelined: the next sub-tile's column values and grad_out tile are loaded into
    // registers while the MFMAs of the current one run from LDS
    float rc[KC / 4], rg[64 * PT / NT];
    const int ki = (k / a.kw) * a.dil - a.pad, kj = (k % a.kw) * a.dil - a.pad;
    auto load = [&](long t0) {
      const long t = t0 + lane;
      const int n = t < r1 ? (int)(t / P) : 0;
      const long p = t < r1 ? t % P : 0;
      const int hi = (int)(p / a.Wo) * a.stride + ki, wi = (int)(p % a.Wo) * a.stride + kj;
      const bool ok = t < r1 && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
      const float *xn = a.x + (long)n * C * HW + (long)hi * a.W + wi;
#pragma unroll
      for (int ii = 0; ii < KC / 4; ++ii) {
        const int cl = wave + 4 * ii;
        rc[ii] = (cl < rows && ok) ? xn[(long)(c0 + cl) * HW] : 0.f;
      }
      const float *gp = gout + (long)n * Co * P + p;  // thread = pixel lane, rows wave + 4i
#pragma unroll
      for (int i = 0; i < 64 * PT / NT; ++i) {
        const int co = co0 + wave + 4 * i;
        rg[i] = (t < r1 && co < coE) ? gp[(long)co * P] : 0.f;
      }
    };
    auto store = [&]() {
#pragma unroll
      for (int ii = 0; ii < KC / 4; ++ii) sC[(wave + 4 * ii) * GP2 + lane] = rc[ii];
#pragma unroll
      for (int i = 0; i < 64 * PT / NT; ++i) sG[(wave + 4 * i) * GP2 + lane] = rg[i];
    };
    load(r0);
    store();
    __syncthreads();
    for (long t0 = r0; t0 < r1; t0 += PT) {
      const bool more = t0 + PT < r1;
      if (more) load(t0 + PT);
#pragma unroll 4
      for (int ks = 0; ks < PT / 4; ++ks) {
        const float av = sG[(16 * wave + jj) * GP2 + 4 * ks + kr];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          const float bv = sC[(16 * cb + jj) * GP2 + 4 * ks + kr];
          acc[cb] = mfma16x16x4(av, bv, acc[cb]);
        }
      }
      __syncthreads();
      if (more) {
        store();
        __syncthreads();
      }
    }
  }
  if constexpr (NR && !PLAIN) {
    // Three-stage pipeline over the 64-pixel sub-tiles: the offsets / mask of sub-tile t+2 and
    // the corner quads + grad_out tile of t+1 are loaded while the MFMAs of t run from LDS
    // (sampling positions depend on the offsets: two dependent load levels per sub-tile).
    const int q = tid & 7;
    const int K2 = 2 * K;
    float oh[2][2], ow[2][2], om[2][2];  // [stage slot][it]
    f32x4 rc[2][4];                       // corner quads of the next sub-tile, per it
    float rwt[2][5];                      // w1..w4, mask
    float rg[64 * PT / NT];
    auto off_load = [&](long t0, int sl) {
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const long t = t0 + (tid >> 3) + 32 * it;
        const bool tv = t < r1;
        const int n = tv ? (int)(t / P) : 0;
        const long p = tv ? t % P : 0;
        const float *off = a.offset + (long)n * a.off_bs + (long)g * K2 * P;
        oh[sl][it] = tv ? off[(long)(2 * k) * P + p] : 0.f;
        ow[sl][it] = tv ? off[(long)(2 * k + 1) * P + p] : 0.f;
        om[sl][it] = tv ? load_mask(a, n, g, k, K, P, p) : 0.f;
      }
    };
    auto corner_load = [&](long t0, int sl) {
#pragma clang fp contract(off)
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const long t = t0 + (tid >> 3) + 32 * it;
        const bool tv = t < r1;
        const int n = tv ? (int)(t / P) : 0;
        const long p = tv ? t % P : 0;
        const int ho = (int)(p / a.Wo), wo = (int)(p % a.Wo);
        const float h = (float)(ho * a.stride - a.pad + (k / a.kw) * a.dil) + oh[sl][it];
        const float w = (float)(wo * a.stride - a.pad + (k % a.kw) * a.dil) + ow[sl][it];
        Samp sp;
        make_samp(sp, h, w, a.H, a.W, om[sl][it]);
        const bool ok = tv && 4 * q < rows;
        const float *xq = xh + (long)n * HW * C + c0 + 4 * q;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        rc[it][0] = ok ? *reinterpret_cast<const f32x4 *>(xq + (long)sp.i1 * C) : z;
        rc[it][1] = ok ? *reinterpret_cast<const f32x4 *>(xq + (long)sp.i2 * C) : z;
        rc[it][2] = ok ? *reinterpret_cast<const f32x4 *>(xq + (long)sp.i3 * C) : z;
        rc[it][3] = ok ? *reinterpret_cast<const f32x4 *>(xq + (long)sp.i4 * C) : z;
        rwt[it][0] = sp.w1;
        rwt[it][1] = sp.w2;
        rwt[it][2] = sp.w3;
        rwt[it][3] = sp.w4;
        rwt[it][4] = ok ? sp.m : 0.f;  // 0 * (finite corners) = 0: masked-out rows stage zeros
      }
      const long t = t0 + lane;
      const int n = t < r1 ? (int)(t / P) : 0;
      const long p = t < r1 ? t % P : 0;
      const float *gp = gout + (long)n * Co * P + p;
#pragma unroll
      for (int i = 0; i < 64 * PT / NT; ++i) {
        const int co = co0 + wave + 4 * i;
        rg[i] = (t < r1 && co < coE) ? gp[(long)co * P] : 0.f;
      }
    };
    auto store = [&]() {
#pragma clang fp contract(off)
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int pl = (tid >> 3) + 32 * it;
#pragma unroll
        for (int u = 0; u < 4; ++u)  // samp_val per channel (same products and order)
          sC[(4 * q + u) * GP2 + pl] = (rwt[it][0] * rc[it][0][u] + rwt[it][1] * rc[it][1][u] +
                                        rwt[it][2] * rc[it][2][u] + rwt[it][3] * rc[it][3][u]) * rwt[it][4];
      }
#pragma unroll
      for (int i = 0; i < 64 * PT / NT; ++i) sG[(wave + 4 * i) * GP2 + lane] = rg[i];
    };
    off_load(r0, 0);
    corner_load(r0, 0);
    if (r0 + PT < r1) off_load(r0 + PT, 1);
    store();
    __syncthreads();
    int sl = 1;  // offset slot of sub-tile t0 + PT
    for (long t0 = r0; t0 < r1; t0 += PT) {
      const bool more = t0 + PT < r1;
      if (more) {
        corner_load(t0 + PT, sl);
        if (t0 + 2 * PT < r1) off_load(t0 + 2 * PT, sl ^ 1);
      }
#pragma unroll 4
      for (int ks = 0; ks < PT / 4; ++ks) {
        const float av = sG[(16 * wave + jj) * GP2 + 4 * ks + kr];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          const float bv = sC[(16 * cb + jj) * GP2 + 4 * ks + kr];
          acc[cb] = mfma16x16x4(av, bv, acc[cb]);
        }
      }
      __syncthreads();
      if (more) {
        store();
        __syncthreads();
      }
      sl ^= 1;
    }
  }
  // NCHW x (neither PLAIN nor NR): the sampled col chunk and the grad_out tile per sub-tile
  for (long t0 = r0; t0 < r1 && !PLAIN && !NR; t0 += PT) {
    const long t = t0 + lane;
    const bool tv = t < r1;
    const int n = tv ? (int)(t / P) : 0;
    const long p = tv ? t % P : 0;
    Samp s;
    pixel_samp(s, a, n, g, k, p, (int)(p / a.Wo), (int)(p % a.Wo));
    const float *xn = a.x + (long)n * C * HW;
#pragma unroll
    for (int ii = 0; ii < KC / 4; ++ii) {
      const int cl = wave + 4 * ii;
      float v = 0.f;
      if (cl < rows && tv) v = samp_val(xn + (long)(c0 + cl) * HW, s);
      sC[cl * GP2 + lane] = v;
    }
    for (int e = tid; e < 64 * PT; e += NT) {
      const int col = e / PT, pl = e % PT;
      const long tt = t0 + pl;
      const int co = co0 + col;
      float v = 0.f;
      if (tt < r1 && co < coE) v = gout[((long)(tt / P) * Co + co) * P + tt % P];
      sG[col * GP2 + pl] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int ks = 0; ks < PT / 4; ++ks) {
      const float av = sG[(16 * wave + jj) * GP2 + 4 * ks + kr];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const float bv = sC[(16 * cb + jj) * GP2 + 4 * ks + kr];
        acc[cb] = mfma16x16x4(av, bv, acc[cb]);
      }
    }
    __syncthreads();
  }
  // D[i = co (4kr + r)][jj = channel]
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + 16 * wave + 4 * kr + r, cl = 16 * cb + jj;
      if (co < coE && cl < rows) {
        const long e = ((long)co * Cw + cw0 + cl) * K + k;
        if (DET)
          part[(long)blockIdx.y * Co * Cw * K + e] = acc[cb][r];
        else
          atomicAdd(gw + e, acc[cb][r]);
      }
    }
}

// gb[co] += sum over n, p of gout[n][co][p]: one 1024-thread workgroup per channel, 16-byte
// loads when P % 4 == 0, fixed-order tree reduction (bit-reproducible).
__global__ __launch_bounds__(1024) void bias_grad_kernel(const float *__restrict__ gout,
                                                         float *__restrict__ gb, int N, int Co,
                                                         long P, int overwrite = 0) {
  const int co = blockIdx.x;
  float s = 0.f;
  if ((P & 3) == 0 && (reinterpret_cast<uintptr_t>(gout) & 15) == 0) {
    for (int n = 0; n < N; ++n) {
      const f32x4 *g4 = reinterpret_cast<const f32x4 *>(gout + ((long)n * Co + co) * P);
      for (long q = threadIdx.x; q < (P >> 2); q += 1024) {
        const f32x4 v = g4[q];
        s += (v[0] + v[1]) + (v[2] + v[3]);
      }
    }
  } else {
    for (int n = 0; n < N; ++n)
      for (long p = threadIdx.x; p < P; p += 1024) s += gout[((long)n * Co + co) * P + p];
  }
  __shared__ float red[1024];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) gb[co] = overwrite ? red[0] : gb[co] + red[0];
}

// grad_x NHWC workspace [N][HW][C] -> NCHW: 32 x 32 tiles through LDS (both sides coalesced).
// T = long long: the deterministic fixed-point accumulator (value * scale), converted to fp32 here.
template <typename T>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const T *__restrict__ src,
                                                           float *__restrict__ dst, int C, long HW,
                                                           const double *__restrict__ det_scale) {
  __shared__ float t[32][33];
  const double inv = det_scale ? 1.0 / *det_scale : 1.0;
  const int n = blockIdx.z;
  const long s0 = (long)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const T *sn = src + (long)n * HW * C;
  float *dn = dst + (long)n * C * HW;
  for (int r = ty; r < 32; r += 8) {
    const long sp = s0 + r;
    float v = 0.f;
    if (sp < HW && c0 + tx < C) {
      if constexpr (sizeof(T) == 8)
        v = (float)((double)sn[sp * C + c0 + tx] * inv);
      else
        v = sn[sp * C + c0 + tx];
    }
    t[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r;
    if (c < C && s0 + tx < HW) dn[(long)c * HW + s0 + tx] = t[tx][r];
  }
}

// ---- deterministic-backward helpers ---------------------------------------------------------
// bounds[0] = max_{c,k} sum_co |W[co][c][k]|, bounds[1] = max|gOut|, bounds[2] = max|mask|, as
// float bits (non-negative floats order like their bit patterns).  Every grad_x contribution is
// colg * w_corner * m with |colg| <= bounds[0]*bounds[1] and |w_corner| <= 1.
__global__ __launch_bounds__(256) void det_wbound_kernel(const float *__restrict__ w, int Co, int CK,
                                                         unsigned *__restrict__ bounds) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < CK; e += gridDim.x * 256) {
    float s = 0.f;
    for (int co = 0; co < Co; ++co) s += fabsf(w[(long)co * CK + e]);
    atomicMax(bounds, __float_as_uint(s) & 0x7fffffffu);  // NaN bits order above +inf
  }
}

// max |v| into *slot (as the uint bits of a non-negative float): 16-byte loads when v is
// 16-byte aligned, one atomic per workgroup (a few hundred workgroups: per-wave atomics on one
// address serialise at the L2 and dominated this kernel).  The max is taken over the bit
// patterns of |v|, which order like the values and put NaN (0x7fc...) above +inf: a NaN or an
// inf anywhere reaches the bound (fmaxf would drop a NaN), and det_scale_kernel then poisons.
__device__ __forceinline__ unsigned abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__global__ __launch_bounds__(256) void det_absmax_kernel(const float *__restrict__ v, long n,
                                                         unsigned *__restrict__ slot) {
  __shared__ unsigned red[4];
  unsigned m = 0u;
  const long stride = (long)gridDim.x * 256, t0 = (long)blockIdx.x * 256 + threadIdx.x;
  long tail = 0;
  if ((reinterpret_cast<uintptr_t>(v) & 15) == 0) {
    const long n4 = n >> 2;
    for (long q = t0; q < n4; q += stride) {
      const f32x4 x = reinterpret_cast<const f32x4 *>(v)[q];
      m = max(m, max(max(abs_bits(x[0]), abs_bits(x[1])), max(abs_bits(x[2]), abs_bits(x[3]))));
    }
    tail = n4 << 2;
  }
  for (long e = tail + t0; e < n; e += stride) m = max(m, abs_bits(v[e]));
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(slot, max(max(red[0], red[1]), max(red[2], red[3])));
}

// scale[0] = 2^(38 - ceil(log2 bound)): a single contribution stays below 2^38, so up to 2^25 of
// them can meet in one element before the int64 sum could overflow; the fixed-point step
// (2^-38 of the largest possible contribution) is far below fp32 rounding of typical sums.
// A non-finite bound (an inf or NaN in the weights, grad_out or mask) gives scale = NaN: the
// fixed-point sums are then read back through 1/scale = NaN, so grad_x comes out NaN instead
// of finite garbage from __double2ll_rn(inf/NaN) (the reference's float col2im would propagate
// the non-finite value).
// scale[1]: the deterministic window form's weight-gradient accumulator.  Every element is a sum
// over the npix output pixels of gOut * column, |column| <= max|x| * max|mask| (bilinear weights
// sum to <= 1), so the whole sum is bounded by bw = npix * bounds[1] * bounds[3] * bounds[2] and
// 2^(62 - ceil(log2 bw)) keeps it (plus half a step per tile of rounding) inside int64.
__global__ void det_scale_kernel(const unsigned *__restrict__ bounds, double *__restrict__ scale, long npix) {
  const double b = (double)__uint_as_float(bounds[0]) * (double)__uint_as_float(bounds[1]) *
                   (double)__uint_as_float(bounds[2]);
  scale[0] = !isfinite(b) ? __builtin_nan("") : (b > 0.0 ? ldexp(1.0, 38 - (int)ceil(log2(b))) : 1.0);
  const double bw = (double)npix * (double)__uint_as_float(bounds[1]) * (double)__uint_as_float(bounds[2]) *
                    (double)__uint_as_float(bounds[3]);
  scale[1] = !isfinite(bw) ? __builtin_nan("") : (bw > 0.0 ? ldexp(1.0, 62 - (int)ceil(log2(bw))) : 1.0);
}

// gw[e] += sum over the splits of part[split][e], in a fixed order: workgroup = 64 consecutive
// elements x 4 split lanes (lane l sums splits l, l+4, ... in order, 4 loads in flight), then the
// 4 lane sums are added in lane order -- bit-reproducible for a given nsplit.
__global__ __launch_bounds__(256) void det_weight_reduce_kernel(const float *__restrict__ part,
                                                                float *__restrict__ gw, long n,
                                                                int nsplit, int overwrite = 0) {
  __shared__ float red[4][64];
  const int ex = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const long e = (long)blockIdx.x * 64 + ex;
  float s = 0.f;
  if (e < n) {
    int y = sl;
    for (; y + 12 < nsplit; y += 16) {
      const float v0 = part[(long)y * n + e], v1 = part[(long)(y + 4) * n + e];
      const float v2 = part[(long)(y + 8) * n + e], v3 = part[(long)(y + 12) * n + e];
      s += v0;
      s += v1;
      s += v2;
      s += v3;
    }
    for (; y < nsplit; y += 4) s += part[(long)y * n + e];
  }
  red[sl][ex] = s;
  __syncthreads();
  if (sl == 0 && e < n) {
    const float v = ((red[0][ex] + red[1][ex]) + red[2][ex]) + red[3][ex];
    gw[e] = overwrite ? v : gw[e] + v;
  }
}

struct BwdPlan {
  int npieces, nchunks, nsplit;
  long range;
};

BwdPlan bwd_plan(const MdcnArgs &a, long target = 2048) {
  BwdPlan pl;
  const long P = (long)a.Ho * a.Wo, T = (long)a.N * P;
  const int K = a.kh * a.kw, cpg = a.C / a.dg;
  pl.npieces = host_div_up(cpg, KC);
  pl.nchunks = K * a.dg * pl.npieces;
  // ~target workgroups in total; each covers `range` flattened pixels
  long nsplit = target / pl.nchunks;
  if (nsplit < 1) nsplit = 1;
  long range = (T + nsplit - 1) / nsplit;
  range = ((range + PT - 1) / PT) * PT;
  pl.nsplit = (int)((T + range - 1) / range);
  pl.range = range;
  return pl;
}

// Deterministic-backward workspace, per chunk of images (det_chunk): [grad_x as int64]
// [weight-gradient partials (global form) | int64 [K][Co][C] accumulator (window form)]
// [bounds, scales][x channels-last][W^T]
struct DetLayout {
  size_t gxi, part, bounds, scale, xh, wt, gw, total;
};

bool bwd_nhwc_reads(const MdcnArgs &a);
// the window form's LDS (mdcn_bwd_core), fused weight gradient, and whether a shape takes it
// the window of an 8 x 8 output tile: 7 * stride + 1 input rows / columns under the taps' reach,
// plus the R = 2 margin on both sides (offsets in [-2, 2) stay inside)
int win_rows(int kh, int dil, int stride) { return 7 * stride + 1 + (kh - 1) * dil + 4; }
size_t win_smem(const MdcnArgs &a) {
  const int GPW = round_pitch(PT, 2), WTP = round_pitch(a.Co, 2);
  const int WR = win_rows(a.kh, a.dil, a.stride), WCw = win_rows(a.kw, a.dil, a.stride);
  return sizeof(float) * ((size_t)a.Co * GPW + (size_t)WHC * WTP + (size_t)WHC * WCP + (size_t)PT * 16 +
                          (size_t)3 * WKMAX * PT + (size_t)WHC * WCP) +
         (size_t)WR * WCw * WHC * 8;
}
// round 6: stride 2, up to 128 channels per deformable group (the 16-channel slices' offset /
// mask partials accumulate in sP in slice order) and up to 128 output channels (the fused weight
// gradient loops over 64-channel blocks): the feature extractor's DCNs (nets/resnet.py:133-134)
bool win_shape_ok(const MdcnArgs &a) {
  return bwd_nhwc_reads(a) && (a.stride == 1 || a.stride == 2) && a.C / a.dg <= 8 * WHC &&
         a.kh * a.kw <= WKMAX && a.Co <= WCOMAX && a.Co % 16 == 0 && win_smem(a) <= 160 * 1024;
}

// The deterministic backward runs over the batch in chunks of images whose int64 grad_x
// accumulator + channels-last x (12 bytes per input element) fit DET_CHUNK_BYTES: the workspace
// no longer grows with the batch (agg_s0 at B = 8: 377 MB unchunked).  Chunks are a fixed
// function of the shape, so the result stays bit-reproducible.
constexpr size_t DET_CHUNK_BYTES = (size_t)96 << 20;
int det_chunk(const MdcnArgs &a) {
  const size_t per = (size_t)12 * a.C * a.H * a.W;
  size_t nc = per ? DET_CHUNK_BYTES / per : (size_t)a.N;
  if (nc < 1) nc = 1;
  return nc < (size_t)a.N ? (int)nc : a.N;
}

DetLayout det_layout(const MdcnArgs &a0, const BwdPlan &) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  MdcnArgs a = a0;
  a.N = det_chunk(a0);
  const BwdPlan pl = bwd_plan(a);
  DetLayout L{};
  const size_t nx = (size_t)a.N * a.C * a.H * a.W;
  const size_t nw = (size_t)a.Co * a.C * a.kh * a.kw;
  const size_t part = (size_t)pl.nsplit * nw * 4;
  L.gxi = 0;
  L.part = up(L.gxi + nx * 8);
  L.gw = L.part;  // the window form's accumulator shares the region with the global form's partials
  L.bounds = up(L.part + (part > GW_COPIES * nw * 8 ? part : GW_COPIES * nw * 8));
  L.scale = L.bounds + 16;
  L.xh = up(L.scale + 16);  // channels-last x and wT[k][c][co] (mdcn_bwd_data_nhwc_kernel)
  L.wt = up(L.xh + nx * 4);
  L.total = up(L.wt + nw * 4);
  return L;
}

// Float-atomic workspace (aanet_mdcn_bwd_ws_f32): [grad_x NHWC accumulator][x NHWC][wT]
// [bounds, scale] (the window form's fixed-point scale)
DetLayout ws_layout(const MdcnArgs &a) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  DetLayout L{};
  const size_t nx = (size_t)a.N * a.C * a.H * a.W;
  const size_t nw = (size_t)a.Co * a.C * a.kh * a.kw;
  L.gxi = 0;
  L.xh = up(nx * 4);
  L.wt = up(L.xh + nx * 4);
  L.bounds = up(L.wt + nw * 4);
  L.scale = L.bounds + 16;
  L.gw = up(L.scale + 16);  // [GW_COPIES][K][Co][C] weight-gradient accumulator of the fused window form
  L.total = up(L.gw + GW_COPIES * nw * 4);
  return L;
}

bool bwd_nhwc_reads(const MdcnArgs &a) { return a.C % 4 == 0 && (a.C / a.dg) % 4 == 0; }

int mdcn_bwd_core(const float *x, const float *offset, const float *mask, const float *weight,
                  const float *grad_out, float *grad_x, float *grad_offset, float *grad_mask,
                  float *grad_weight, float *grad_bias, int n, int c, int h, int w, int co,
                  int kh, int kw, int stride, int pad, int dil, int groups, int dg, int det,
                  int algo, void *ws, size_t ws_bytes, hipStream_t st) {
  if (algo < AANET_DCN_BWD_AUTO || algo > AANET_DCN_BWD_WINDOW) return AANET_EINVAL;
  MdcnArgs a = make_args(x, offset, -1, mask, -1, 0, 1.f, weight, nullptr, nullptr, nullptr, 0,
                         nullptr, n, c, h, w, co, kh, kw, stride, pad, dil, groups, dg);
  int rc = check_shapes(a);
  if (rc) return rc;
  if (!x || !offset || !mask || !weight || !grad_out || !grad_x || !grad_offset || !grad_mask ||
      !grad_weight)
    return AANET_EINVAL;
  if (groups != 1) return AANET_EUNSUPPORTED;  // AANet uses groups=1 (nets/deform.py:25)
  if (co % 4 || co > 256) return AANET_EUNSUPPORTED;
  const long P = (long)a.Ho * a.Wo;
  const int K = kh * kw;
  const BwdPlan pl = bwd_plan(a);
  DetLayout L{};
  char *wb = static_cast<char *>(ws);
  // det: 0 float atomics into grad_x (NCHW); 1 deterministic (fixed point, workspace);
  // 2 float atomics into an NHWC workspace of n*h*w*c floats, then transposed into grad_x
  // (the deterministic form always scatters into its fixed-point accumulator in NHWC order)
  const int nhs = det != 0;
  det = det == 1;
  if (det || nhs) {
    L = det ? det_layout(a, pl) : ws_layout(a);
    if (!ws || ws_bytes < L.total) return AANET_EINVAL;
  }
  const bool nr = nhs && bwd_nhwc_reads(a);  // channels-last reads too
  const int GP = round_pitch(PT, 16), WTP = round_pitch(co, 2);
  // window form of grad_x (stride 1 / 2, <= 128 channels per deformable group, channels-last reads,
  // <= 9 taps, <= 128 output channels): 8x8 tile per workgroup in 16-channel slices, int64
  // fixed-point LDS window.
  // AUTO takes it in both modes; GLOBAL / WINDOW force one form (tests, A/B).
  const int R = 2;
  const int WR = win_rows(kh, dil, stride), WCw = win_rows(kw, dil, stride);
  // the weight gradient rides in the window kernel (both modes).
  // gOut tile pitch of the window kernel: 80 (= 16 mod 32) keeps the colg reads (rows kr,
  // columns jj) conflict-free; the fused weight gradient also reads it transposed (rows jj), which
  // that pitch makes 8-way conflicted, so the fused form uses 66 (2-way for both)
  const int GPW = round_pitch(PT, 2);
  const bool win_ok = nr && win_shape_ok(a);
  if (algo == AANET_DCN_BWD_WINDOW && !win_ok) return AANET_EUNSUPPORTED;
  // AUTO takes the window form where it measured faster: the aggregation's shapes (stride 1,
  // <= 32 channels per group, Co <= 64).  At the feature extractor's shapes (64-channel groups,
  // Co = 128, one workgroup per CU for its LDS) it measured slower in float mode (C4 feat_s1 /
  // feat_s2 990 / 1089 us vs 853 / 856 us global) and mixed in fixed point (983 vs 1046 us at
  // stride 1, 1177 vs 1073 at stride 2; CHANGELOG.md round 6): WINDOW selects it there.
  const bool win_auto = a.stride == 1 && a.C / a.dg <= 2 * WHC && a.Co <= 64;
  const bool use_win = win_ok && (algo == AANET_DCN_BWD_WINDOW || (algo == AANET_DCN_BWD_AUTO && win_auto));
  float *xh = nhs ? reinterpret_cast<float *>(wb + L.xh) : nullptr;
  float *wt = nhs ? reinterpret_cast<float *>(wb + L.wt) : nullptr;
  long long *gxi = det ? reinterpret_cast<long long *>(wb + L.gxi) : nullptr;
  float *part = det ? reinterpret_cast<float *>(wb + L.part) : nullptr;
  const bool fixed = det || use_win;  // a fixed-point scale is needed
  unsigned *bounds = fixed ? reinterpret_cast<unsigned *>(wb + L.bounds) : nullptr;
  double *scale = fixed ? reinterpret_cast<double *>(wb + L.scale) : nullptr;
  const size_t nx = (size_t)n * c * h * w;
  hipError_t e;
  if (det)
    e = hipMemsetAsync(gxi, 0, nx * 8, st);
  else
    e = hipMemsetAsync(nhs ? ws : grad_x, 0, sizeof(float) * nx, st);  // float atomics
  if (e != hipSuccess) return (int)e;
  if (fixed) {
    e = hipMemsetAsync(bounds, 0, 16, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(det_wbound_kernel, dim3(host_div_up((long)c * K, 256)), dim3(256), 0, st,
                       weight, co, c * K, bounds);
    const long ng = (long)n * co * P, nm = (long)n * dg * K * P;
    hipLaunchKernelGGL(det_absmax_kernel, dim3(host_div_up(ng, 1024) > 512 ? 512 : host_div_up(ng, 1024)),
                       dim3(256), 0, st, grad_out, ng, bounds + 1);
    hipLaunchKernelGGL(det_absmax_kernel, dim3(host_div_up(nm, 1024) > 512 ? 512 : host_div_up(nm, 1024)),
                       dim3(256), 0, st, mask, nm, bounds + 2);
    if (det && use_win) {  // max|x|: the window form's weight-gradient bound (det_scale_kernel)
      const long nxl = (long)nx;
      hipLaunchKernelGGL(det_absmax_kernel, dim3(host_div_up(nxl, 1024) > 512 ? 512 : host_div_up(nxl, 1024)),
                         dim3(256), 0, st, x, nxl, bounds + 3);
    }
    hipLaunchKernelGGL(det_scale_kernel, dim3(1), dim3(1), 0, st, bounds, scale, (long)n * P);
  }
  const size_t smem = sizeof(float) * ((size_t)co * GP + (size_t)KC * WTP + (size_t)KC * CP + 3 * 4 * 64 +
                                      (size_t)PT * 12);
  // sG grows with Co (Co = 128 in the feature extractor's DCNs: ~69 KB); a gfx950 workgroup may
  // use the CU's whole 160 KiB of LDS
  if (smem > 160 * 1024) return AANET_EUNSUPPORTED;
  static const bool lds_attr = [] {
    const void *const big_lds[] = {
        reinterpret_cast<const void *>(&mdcn_bwd_data_kernel<0>),
        reinterpret_cast<const void *>(&mdcn_bwd_data_kernel<1, 1>),
        reinterpret_cast<const void *>(&mdcn_bwd_data_kernel<0, 1>),
        reinterpret_cast<const void *>(&mdcn_bwd_data_nhwc_kernel<0>),
        reinterpret_cast<const void *>(&mdcn_bwd_data_nhwc_kernel<1>),
        reinterpret_cast<const void *>(&mdcn_bwd_data_win_kernel<1, 1>),
        reinterpret_cast<const void *>(&mdcn_bwd_data_win_kernel<0, 1>)};
    for (const void *k : big_lds)
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return true;
  }();
  (void)lds_attr;
  const dim3 gdata((unsigned)(n * host_div_up(P, PT)), (unsigned)dg);
  if (nr) {
    const long HW = (long)h * w;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3((unsigned)host_div_up(HW, 32), (unsigned)host_div_up(c, 32), (unsigned)n),
                       dim3(256), 0, st, x, xh, c, HW);
    const long nw = (long)co * c * K;
    hipLaunchKernelGGL(weight_kcco_kernel, dim3(host_div_up(nw, 256) > 1024 ? 1024 : host_div_up(nw, 256)),
                       dim3(256), 0, st, weight, wt, co, c, K);
    const size_t smem2 = sizeof(float) * ((size_t)co * GP + (size_t)KC * WTP + (size_t)KC * CP + (size_t)PT * 12);
#ifdef AANET_DEBUG_SWITCHES  // timing build only (skips the grad_x scatter: WRONG gradients)
    const char *dbg_env = getenv("AANET_DCN_BWD_DBG");
    a.dbg_noatom = dbg_env ? atoi(dbg_env) : 0;
    if (a.dbg_noatom) fprintf(stderr, "aanet: AANET_DCN_BWD_DBG -- timing build, gradients INVALID\n");
#else
    a.dbg_noatom = 0;
#endif
    if (use_win) {
      const dim3 gwin((unsigned)(n * host_div_up(a.Wo, 8) * host_div_up(a.Ho, 8)), (unsigned)dg);
      if (det) {
        long long *gwi = reinterpret_cast<long long *>(wb + L.gw);
        const long nw = (long)co * c * K;
        e = hipMemsetAsync(gwi, 0, sizeof(long long) * GW_COPIES * (size_t)nw, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((mdcn_bwd_data_win_kernel<1, 1>), gwin, dim3(NT), win_smem(a), st, a, xh, wt, grad_out,
                           grad_x, grad_offset, grad_mask, GPW, WTP, gxi, scale, WR, WCw, R, nullptr, gwi);
        hipLaunchKernelGGL(det_gw_final_kernel, dim3(host_div_up(nw, 256) > 1024 ? 1024 : host_div_up(nw, 256)),
                           dim3(256), 0, st, gwi, grad_weight, co, c, K, scale + 1);
      } else {
        float *gwT = reinterpret_cast<float *>(wb + L.gw);
        const long nw = (long)co * c * K;
        e = hipMemsetAsync(gwT, 0, sizeof(float) * GW_COPIES * (size_t)nw, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((mdcn_bwd_data_win_kernel<0, 1>), gwin, dim3(NT), win_smem(a), st, a, xh, wt, grad_out,
                           reinterpret_cast<float *>(wb + L.gxi), grad_offset, grad_mask, GPW, WTP,
                           nullptr, scale, WR, WCw, R, gwT);
        hipLaunchKernelGGL(gw_kcoc_add_kernel, dim3(host_div_up(nw, 256) > 1024 ? 1024 : host_div_up(nw, 256)),
                           dim3(256), 0, st, gwT, grad_weight, co, c, K);
      }
    } else if (det)
      hipLaunchKernelGGL(mdcn_bwd_data_nhwc_kernel<1>, gdata, dim3(NT), smem2, st, a, xh, wt, grad_out,
                         grad_x, grad_offset, grad_mask, GP, WTP, gxi, scale);
    else
      hipLaunchKernelGGL(mdcn_bwd_data_nhwc_kernel<0>, gdata, dim3(NT), smem2, st, a, xh, wt, grad_out,
                         reinterpret_cast<float *>(wb + L.gxi), grad_offset, grad_mask, GP, WTP,
                         nullptr, nullptr);
  } else if (det)
    hipLaunchKernelGGL((mdcn_bwd_data_kernel<1, 1>), gdata, dim3(NT), smem, st, a, grad_out, grad_x,
                       grad_offset, grad_mask, GP, WTP, gxi, scale);
  else if (nhs)
    hipLaunchKernelGGL((mdcn_bwd_data_kernel<0, 1>), gdata, dim3(NT), smem, st, a, grad_out,
                       reinterpret_cast<float *>(wb + L.gxi), grad_offset, grad_mask, GP, WTP, nullptr, nullptr);
  else
    hipLaunchKernelGGL(mdcn_bwd_data_kernel<0>, gdata, dim3(NT), smem, st, a, grad_out, grad_x,
                       grad_offset, grad_mask, GP, WTP, nullptr, nullptr);
  rc = aanet_launch_status();
  if (rc) return rc;
  {
    const long HW = (long)h * w;
    const dim3 gt((unsigned)host_div_up(HW, 32), (unsigned)host_div_up(c, 32), (unsigned)n);
    if (det)
      hipLaunchKernelGGL(nhwc_to_nchw_kernel<long long>, gt, dim3(256), 0, st, gxi, grad_x, c, HW, scale);
    else if (nhs)
      hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, gt, dim3(256), 0, st,
                         reinterpret_cast<const float *>(wb + L.gxi), grad_x, c, HW, nullptr);
    rc = aanet_launch_status();
    if (rc) return rc;
  }
  const dim3 gw3(pl.nchunks, (unsigned)pl.nsplit, host_div_up(co, 64));
  if (use_win)
    ;  // the window kernel added the weight gradient
  else if (nr && det)
    hipLaunchKernelGGL((mdcn_bwd_weight_kernel<1, 1>), gw3, dim3(NT), 0, st, a, grad_out, grad_weight,
                       pl.npieces, pl.range, part, xh);
  else if (nr)
    hipLaunchKernelGGL((mdcn_bwd_weight_kernel<0, 1>), gw3, dim3(NT), 0, st, a, grad_out, grad_weight,
                       pl.npieces, pl.range, nullptr, xh);
  else if (det)
    hipLaunchKernelGGL(mdcn_bwd_weight_kernel<1>, gw3, dim3(NT), 0, st, a, grad_out, grad_weight,
                       pl.npieces, pl.range, part);
  else
    hipLaunchKernelGGL(mdcn_bwd_weight_kernel<0>, gw3, dim3(NT), 0, st, a, grad_out, grad_weight,
                       pl.npieces, pl.range, nullptr);
  rc = aanet_launch_status();
  if (rc) return rc;
  if (det && !use_win) {
    const long nw = (long)co * c * K;
    hipLaunchKernelGGL(det_weight_reduce_kernel, dim3(host_div_up(nw, 64)), dim3(256), 0, st,
                       part, grad_weight, nw, pl.nsplit);
    rc = aanet_launch_status();
    if (rc) return rc;
  }
  if (grad_bias) {
    hipLaunchKernelGGL(bias_grad_kernel, dim3(co), dim3(1024), 0, st, grad_out, grad_bias, n, co, P);
    rc = aanet_launch_status();
  }
  return rc;
}

// The backward entry: the deterministic mode (det == 1) runs mdcn_bwd_core over chunks of images
// (det_chunk) that share one workspace -- grad_x / grad_offset / grad_mask are per image, the
// weight gradient is added per chunk in chunk order -- and the bias gradient once over the batch.
int mdcn_bwd_impl(const float *x, const float *offset, const float *mask, const float *weight,
                  const float *grad_out, float *grad_x, float *grad_offset, float *grad_mask,
                  float *grad_weight, float *grad_bias, int n, int c, int h, int w, int co,
                  int kh, int kw, int stride, int pad, int dil, int groups, int dg, int det,
                  int algo, void *ws, size_t ws_bytes, hipStream_t st) {
  MdcnArgs a = make_args(x, offset, -1, mask, -1, 0, 1.f, weight, nullptr, nullptr, nullptr, 0,
                         nullptr, n, c, h, w, co, kh, kw, stride, pad, dil, groups, dg);
  if (det != 1 || check_shapes(a) || !x || !offset || !mask || !grad_out || !grad_x || !grad_offset ||
      !grad_mask)
    return mdcn_bwd_core(x, offset, mask, weight, grad_out, grad_x, grad_offset, grad_mask, grad_weight,
                         grad_bias, n, c, h, w, co, kh, kw, stride, pad, dil, groups, dg, det, algo, ws,
                         ws_bytes, st);
  const int nc = det_chunk(a);
  if (ws_bytes < det_layout(a, BwdPlan{}).total) return AANET_EINVAL;
  const long P = (long)a.Ho * a.Wo, K = (long)kh * kw;
  const long sx = (long)c * h * w, soff = 2L * dg * K * P, sm = (long)dg * K * P, sg = (long)co * P;
  for (int i0 = 0; i0 < n; i0 += nc) {
    const int m = n - i0 < nc ? n - i0 : nc;
    const int rc = mdcn_bwd_core(x + i0 * sx, offset + i0 * soff, mask + i0 * sm, weight, grad_out + i0 * sg,
                                 grad_x + i0 * sx, grad_offset + i0 * soff, grad_mask + i0 * sm, grad_weight,
                                 nullptr, m, c, h, w, co, kh, kw, stride, pad, dil, groups, dg, det, algo, ws,
                                 ws_bytes, st);
    if (rc) return rc;
  }
  if (grad_bias) {
    hipLaunchKernelGGL(bias_grad_kernel, dim3(co), dim3(1024), 0, st, grad_out, grad_bias, n, co, P);
    return aanet_launch_status();
  }
  return 0;
}

// Workgroups per conv weight-gradient launch (pixel splits x chunks x co tiles, before rounding):
// fewer splits mean longer MFMA accumulation per workgroup and less partial-sum traffic for the
// reduction.  Training step (bench.py --train, same-call A/B): 14.44 ms at 1024, 14.59 at 2048,
// 14.42 at 768, 14.53 at 512, 14.87 at 4096.
#ifndef AANET_WGRAD_WGS
#define AANET_WGRAD_WGS 1024
#endif
// aanet_conv2d_wgrad_f32: the weight kernel in PLAIN form (a.dg = groups), then for det the
// fixed-order reduction of the per-split partials; the bias gradient is a per-channel sum in a
// fixed order either way.  det == 2: the same, but the reduction and the bias sum STORE their
// results (grad_weight / grad_bias need no zero fill beforehand).
int conv_wgrad_impl(const float *x, const float *grad_out, float *grad_weight, float *grad_bias,
                    int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad,
                    int dil, int groups, int det, void *ws, size_t ws_bytes, hipStream_t st) {
  MdcnArgs a = make_args(x, nullptr, -1, nullptr, -1, 0, 1.f, nullptr, nullptr, nullptr, nullptr,
                         0, nullptr, n, c, h, w, co, kh, kw, stride, pad, dil, groups, groups);
  int rc = check_shapes(a);
  if (rc) return rc;
  if (!x || !grad_out || !grad_weight || det < 0 || det > 2) return AANET_EINVAL;
  const BwdPlan pl = bwd_plan(a, AANET_WGRAD_WGS);
  const long nw = (long)co * (c / groups) * kh * kw;
  float *part = nullptr;
  if (det) {
    if (!ws || ws_bytes < (size_t)pl.nsplit * nw * 4) return AANET_EINVAL;
    part = static_cast<float *>(ws);
  }
  const dim3 gw3(pl.nchunks, (unsigned)pl.nsplit, host_div_up(co / groups, 64));
  if (det)
    hipLaunchKernelGGL((mdcn_bwd_weight_kernel<1, 0, 1>), gw3, dim3(NT), 0, st, a, grad_out,
                       grad_weight, pl.npieces, pl.range, part, nullptr);
  else
    hipLaunchKernelGGL((mdcn_bwd_weight_kernel<0, 0, 1>), gw3, dim3(NT), 0, st, a, grad_out,
                       grad_weight, pl.npieces, pl.range, nullptr, nullptr);
  rc = aanet_launch_status();
  if (rc) return rc;
  if (det) {
    hipLaunchKernelGGL(det_weight_reduce_kernel, dim3(host_div_up(nw, 64)), dim3(256), 0, st,
                       part, grad_weight, nw, pl.nsplit, (int)(det == 2));
    rc = aanet_launch_status();
    if (rc) return rc;
  }
  if (grad_bias) {
    hipLaunchKernelGGL(bias_grad_kernel, dim3(co), dim3(1024), 0, st, grad_out, grad_bias, n, co,
                       (long)a.Ho * a.Wo, (int)(det == 2));
    rc = aanet_launch_status();
  }
  return rc;
}

}  // namespace

extern "C" size_t aanet_conv2d_wgrad_workspace_size(int n, int c, int h, int w, int co, int kh,
                                                    int kw, int stride, int pad, int dil,
                                                    int groups) {
  MdcnArgs a = make_args(nullptr, nullptr, -1, nullptr, -1, 0, 1.f, nullptr, nullptr, nullptr,
                         nullptr, 0, nullptr, n, c, h, w, co, kh, kw, stride, pad, dil, groups,
                         groups);
  if (check_shapes(a)) return 0;
  return (size_t)bwd_plan(a, AANET_WGRAD_WGS).nsplit * co * (c / groups) * kh * kw * 4;
}

extern "C" int aanet_conv2d_wgrad_f32(const float *x, const float *grad_out, float *grad_weight,
                                      float *grad_bias, int n, int c, int h, int w, int co, int kh,
                                      int kw, int stride, int pad, int dil, int groups,
                                      int deterministic, void *workspace, size_t workspace_bytes,
                                      aanet_stream_t stream) {
  return conv_wgrad_impl(x, grad_out, grad_weight, grad_bias, n, c, h, w, co, kh, kw, stride, pad,
                         dil, groups, deterministic, workspace, workspace_bytes, as_hip(stream));
}

extern "C" int aanet_mdcn_bwd_f32(const float *x, const float *offset, const float *mask,
                                  const float *weight, const float *grad_out, float *grad_x,
                                  float *grad_offset, float *grad_mask, float *grad_weight,
                                  float *grad_bias, int n, int c, int h, int w, int co, int kh,
                                  int kw, int stride, int pad, int dil, int groups, int dg,
                                  aanet_stream_t stream) {
  return mdcn_bwd_impl(x, offset, mask, weight, grad_out, grad_x, grad_offset, grad_mask,
                       grad_weight, grad_bias, n, c, h, w, co, kh, kw, stride, pad, dil, groups,
                       dg, 0, AANET_DCN_BWD_GLOBAL, nullptr, 0, as_hip(stream));
}

extern "C" size_t aanet_mdcn_bwd_ws_workspace_size(int n, int c, int h, int w, int co, int kh,
                                                   int kw, int stride, int pad, int dil,
                                                   int groups, int dg) {
  MdcnArgs a = make_args(nullptr, nullptr, -1, nullptr, -1, 0, 1.f, nullptr, nullptr, nullptr,
                         nullptr, 0, nullptr, n, c, h, w, co, kh, kw, stride, pad, dil, groups, dg);
  if (check_shapes(a)) return 0;
  return ws_layout(a).total;
}

extern "C" int aanet_mdcn_bwd_ws_f32(const float *x, const float *offset, const float *mask,
                                     const float *weight, const float *grad_out, float *grad_x,
                                     float *grad_offset, float *grad_mask, float *grad_weight,
                                     float *grad_bias, int n, int c, int h, int w, int co, int kh,
                                     int kw, int stride, int pad, int dil, int groups, int dg,
                                     void *workspace, size_t workspace_bytes,
                                     aanet_stream_t stream) {
  return mdcn_bwd_impl(x, offset, mask, weight, grad_out, grad_x, grad_offset, grad_mask,
                       grad_weight, grad_bias, n, c, h, w, co, kh, kw, stride, pad, dil, groups,
                       dg, 2, AANET_DCN_BWD_AUTO, workspace, workspace_bytes, as_hip(stream));
}

extern "C" size_t aanet_mdcn_bwd_det_workspace_size(int n, int c, int h, int w, int co, int kh,
                                                    int kw, int stride, int pad, int dil,
                                                    int groups, int dg) {
  MdcnArgs a = make_args(nullptr, nullptr, -1, nullptr, -1, 0, 1.f, nullptr, nullptr, nullptr,
                         nullptr, 0, nullptr, n, c, h, w, co, kh, kw, stride, pad, dil, groups, dg);
  if (check_shapes(a)) return 0;
  return det_layout(a, bwd_plan(a)).total;
}

extern "C" int aanet_mdcn_bwd_det_f32(const float *x, const float *offset, const float *mask,
                                      const float *weight, const float *grad_out, float *grad_x,
                                      float *grad_offset, float *grad_mask, float *grad_weight,
                                      float *grad_bias, int n, int c, int h, int w, int co,
                                      int kh, int kw, int stride, int pad, int dil, int groups,
                                      int dg, void *workspace, size_t workspace_bytes,
                                      aanet_stream_t stream) {
  return mdcn_bwd_impl(x, offset, mask, weight, grad_out, grad_x, grad_offset, grad_mask,
                       grad_weight, grad_bias, n, c, h, w, co, kh, kw, stride, pad, dil, groups,
                       dg, 1, AANET_DCN_BWD_AUTO, workspace, workspace_bytes, as_hip(stream));
}

extern "C" int aanet_mdcn_bwd_algo_f32(const float *x, const float *offset, const float *mask,
                                       const float *weight, const float *grad_out, float *grad_x,
                                       float *grad_offset, float *grad_mask, float *grad_weight,
                                       float *grad_bias, int n, int c, int h, int w, int co,
                                       int kh, int kw, int stride, int pad, int dil, int groups,
                                       int dg, int deterministic, int algo, void *workspace,
                                       size_t workspace_bytes, aanet_stream_t stream) {
  if (deterministic != 0 && deterministic != 1) return AANET_EINVAL;
  return mdcn_bwd_impl(x, offset, mask, weight, grad_out, grad_x, grad_offset, grad_mask,
                       grad_weight, grad_bias, n, c, h, w, co, kh, kw, stride, pad, dil, groups,
                       dg, deterministic ? 1 : 2, algo, workspace, workspace_bytes, as_hip(stream));
}
