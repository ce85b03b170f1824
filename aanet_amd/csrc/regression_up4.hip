// regression_up4.hip -- x4 trilinear upsampling fused into the soft-argmin (the tail of the PSMNet
// aggregators, nets/aggregation.py:136 / 252 + nets/estimation.py:13-30):
//   disp = disp_regress(F.interpolate(cost[:, None], scale_factor=4, mode='trilinear',
//                                     align_corners=False)[:, 0], negate)
// cost [n, d, h, w] -> disp [n, 4h, 4w], candidates 0 .. 4d-1.  The [4d, 4h, 4w] volume is never
// stored: HBM traffic is the coarse cost once (16 output rows share a coarse row; the re-reads
// come from L2) and the disparity map once.
//
// align_corners=False at an exact factor of 4 is separable with constant weights: output index
// 4k + p reads k-1, k, k+1 (clamped to the ends) with weights (.375, .625, 0), (.125, .875, 0),
// (0, .875, .125), (0, .625, .375) for p = 0..3, the same on all three axes (exact in fp32).
//
// One thread owns one coarse column kx of one output row Y, i.e. the four output pixels
// X = 4kx .. 4kx+3.  Per coarse plane k it loads 2 rows x 3 columns (lanes are consecutive in kx:
// three coalesced, shifted loads per row), blends the two rows (the row weights of Y), then forms
// the in-plane values v_k of its four pixels.  A sliding window (v_{k-1}, v_k, v_{k+1}) per pixel
// yields the four fine logits of plane k; normaliser and weighted sum accumulate online as in
// disp_regress_kernel.  The running maximum is that of the fine logits themselves: max_k v_k
// bounds them from above but a fine logit next to a lone peak is only .875 of it, so with logits
// of a few thousand every exponential would underflow against it.  Plane k+2 is loaded before
// plane k's exponentials, so a plane of loads is in flight behind them.  No LDS: the four waves
// of a workgroup share nothing but cache lines, the loads are coalesced as they are, and the
// kernel is bound by its 4d exponentials per pixel, not by the loads (6 per 16 fine logits).
#include "common.h"

namespace {

constexpr int UB = 256;

template <bool VEC>
__global__ __launch_bounds__(UB) void disp_regress_up4_kernel(const float *__restrict__ cost,
                                                              float *__restrict__ disp, int D,
                                                              int H, int W, long total,
                                                              float sign) {
  const long e = (long)blockIdx.x * UB + threadIdx.x;  // (b, Y, kx), kx fastest
  if (e >= total) return;
  const int kx = (int)(e % W);
  const long t = e / W;
  const int Y = (int)(t % (4 * H));
  const long b = t / (4 * H);
  const int ky = Y >> 2, py = Y & 3;
  // rows r0 <= r1 with weights wa, wb; columns kx-1, kx, kx+1 clamped
  const int r0 = py < 2 ? max(ky - 1, 0) : ky, r1 = py < 2 ? ky : min(ky + 1, H - 1);
  const float wa = py == 0 ? 0.375f : py == 1 ? 0.125f : py == 2 ? 0.875f : 0.625f;
  const float wb = 1.f - wa;  // exact
  const int xm = max(kx - 1, 0), xp = min(kx + 1, W - 1);
  const long HW = (long)H * W;
  const float *c0 = cost + b * D * HW + (long)r0 * W, *c1 = cost + b * D * HW + (long)r1 * W;

  // the in-plane (bilinear) values of the four pixels at coarse plane k, sign applied
  auto plane = [&](int k) {
    const float *p0 = c0 + (long)k * HW, *p1 = c1 + (long)k * HW;
    const float a0 = sign * fmaf(wa, p0[xm], wb * p1[xm]);
    const float a1 = sign * fmaf(wa, p0[kx], wb * p1[kx]);
    const float a2 = sign * fmaf(wa, p0[xp], wb * p1[xp]);
    return f32x4{fmaf(0.375f, a0, 0.625f * a1), fmaf(0.125f, a0, 0.875f * a1),
                 fmaf(0.125f, a2, 0.875f * a1), fmaf(0.375f, a2, 0.625f * a1)};
  };

  f32x4 prev = plane(0), cur = prev, nxt = plane(min(1, D - 1));
  float m[4], z[4], acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = -INFINITY, z[i] = 0.f, acc[i] = 0.f;
  for (int k = 0; k < D; ++k) {
    const f32x4 nn = plane(min(k + 2, D - 1));
    const float f0 = (float)(4 * k);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float u0 = fmaf(0.375f, prev[i], 0.625f * cur[i]);
      const float u1 = fmaf(0.125f, prev[i], 0.875f * cur[i]);
      const float u2 = fmaf(0.125f, nxt[i], 0.875f * cur[i]);
      const float u3 = fmaf(0.375f, nxt[i], 0.625f * cur[i]);
      const float cm = fmaxf(fmaxf(u0, u1), fmaxf(u2, u3));
      if (cm > m[i]) {
        const float sc = __expf(m[i] - cm);  // 0 on the first plane (m = -inf)
        z[i] *= sc;
        acc[i] *= sc;
        m[i] = cm;
      }
      const float e0 = __expf(u0 - m[i]), e1 = __expf(u1 - m[i]);
      const float e2 = __expf(u2 - m[i]), e3 = __expf(u3 - m[i]);
      z[i] += (e0 + e1) + (e2 + e3);
      acc[i] += fmaf(e0, f0, e1 * (f0 + 1.f)) + fmaf(e2, f0 + 2.f, e3 * (f0 + 3.f));
    }
    prev = cur;
    cur = nxt;
    nxt = nn;
  }
  float *o = disp + (b * 4 * H + Y) * (4L * W) + 4 * kx;
  const f32x4 r = {acc[0] / z[0], acc[1] / z[1], acc[2] / z[2], acc[3] / z[3]};
  if (VEC) {
    *reinterpret_cast<f32x4 *>(o) = r;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = r[i];
  }
}

}  // namespace

extern "C" int aanet_disp_regress_up4_f32(const float *cost, float *disp, int n, int d, int h,
                                          int w, int negate, aanet_stream_t stream) {
  AANET_HOST_CHECK(cost && disp && n > 0 && d > 0 && h > 0 && w > 0);
  const long total = (long)n * 4 * h * w;
  const long nblk = (total + UB - 1) / UB;
  if (nblk > 0x7fffffffL) return AANET_EUNSUPPORTED;
  const float sign = negate ? -1.f : 1.f;
  hipStream_t st = as_hip(stream);
  if ((reinterpret_cast<uintptr_t>(disp) & 15) == 0)
    hipLaunchKernelGGL(disp_regress_up4_kernel<true>, dim3((unsigned)nblk), dim3(UB), 0, st, cost,
                       disp, d, h, w, total, sign);
  else
    hipLaunchKernelGGL(disp_regress_up4_kernel<false>, dim3((unsigned)nblk), dim3(UB), 0, st, cost,
                       disp, d, h, w, total, sign);
  return aanet_launch_status();
}
