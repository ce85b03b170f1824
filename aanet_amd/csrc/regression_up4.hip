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
//
// Backward (disp_regress_up4_bwd_kernel): grad_disp [n, 4h, 4w] -> grad_cost [n, d, h, w], a gather
// with one owner per coarse element, no atomics, no scratch; bits depend on the shapes only.
//   dL/du_K = g p_K ((K - Kmax) - sum_K' p_K' (K' - Kmax)),  dL/dc = s sum_{K,Y,X} wd wy wx dL/du_K
// (the offset-from-the-arg-max form of regression.hip's disp_regress_bwd_kernel, for its reason).
// The transposed weights: along each axis coarse j collects from fine 4j-2 .. 4j+5 with
// (.125, .375, .625, .875, .875, .625, .375, .125); at a clamped end the weight of the missing
// neighbour folds into the end element.
// A workgroup of BQ x BR threads owns TX x TY = (BQ-2) x (BR/4-1) coarse (kx, ky) and the fine
// pixels of their window: thread (q, r) has the forward's four pixels of coarse column
// kx0 - 1 + q on fine row 4 ky0 - 2 + r (pixels outside the image carry gradient 0).  Each thread
// marches the planes twice with the forward's sliding window.  March 1 is the forward's online
// softmax, which also tracks the arg max Kmax and accumulates sum e (K - Kmax), re-referenced
// when the maximum moves: it leaves m, 1/z and the offset.  March 2 forms dL/du of the four fine
// candidates of plane k per pixel and splits them over planes k-1, k, k+1 (a pending and a carry
// register per pixel, so plane k-1 is complete at step k); the four pixels are reduced over x in
// registers into the contributions to columns kx-1, kx, kx+1, the side ones travel by a lane
// shuffle, and one value per thread goes to LDS (double-buffered: one barrier per plane), from
// where the TY x TX owners add their 8 fine rows in a fixed order and store a coalesced row.
// Statistics recomputed, not saved by the forward -- chosen by reasoning, not measured: the
// Function then keeps nothing but the coarse cost, the entry needs no workspace, and the price is
// one more pass of exponentials: per fine pixel the backward spends 2 (marches) x
// BQ/TX x BR/(4 TY) = 2 x 1.07 x 1.33 = 2.8 forwards' worth of them (measured afterwards,
// profiles/regress_up4_bwd_bench.txt: 3.1 and 3.6 times the forward kernel's time).
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

constexpr int BQ = 32, BR = 16, BT = BQ * BR;  // coarse columns x fine rows of a workgroup
constexpr int TX = BQ - 2, TY = BR / 4 - 1;    // coarse elements it owns per plane

__global__ __launch_bounds__(BT) void disp_regress_up4_bwd_kernel(
    const float *__restrict__ cost, const float *__restrict__ gdisp, float *__restrict__ gcost,
    int D, int H, int W, int tiles_x, int tiles_y, float sign) {
  __shared__ float red[2][BR][BQ];
  const int q = threadIdx.x % BQ, r = threadIdx.x / BQ;
  long blk = blockIdx.x;
  const int kx0 = (int)(blk % tiles_x) * TX;
  blk /= tiles_x;
  const int ky0 = (int)(blk % tiles_y) * TY;
  const long b = blk / tiles_y;
  const int kxu = kx0 - 1 + q, Yu = 4 * ky0 - 2 + r;  // may lie outside the image
  const bool inside = kxu >= 0 && kxu < W && Yu >= 0 && Yu < 4 * H;
  const int kx = min(max(kxu, 0), W - 1), Y = min(max(Yu, 0), 4 * H - 1);
  const int ky = Y >> 2, py = Y & 3;
  const int r0 = py < 2 ? max(ky - 1, 0) : ky, r1 = py < 2 ? ky : min(ky + 1, H - 1);
  const float wa = py == 0 ? 0.375f : py == 1 ? 0.125f : py == 2 ? 0.875f : 0.625f;
  const float wb = 1.f - wa;
  const int xm = max(kx - 1, 0), xp = min(kx + 1, W - 1);
  const long HW = (long)H * W;
  const float *c0 = cost + b * D * HW + (long)r0 * W, *c1 = cost + b * D * HW + (long)r1 * W;

  auto plane = [&](int k) {  // as the forward's
    const float *p0 = c0 + (long)k * HW, *p1 = c1 + (long)k * HW;
    const float a0 = sign * fmaf(wa, p0[xm], wb * p1[xm]);
    const float a1 = sign * fmaf(wa, p0[kx], wb * p1[kx]);
    const float a2 = sign * fmaf(wa, p0[xp], wb * p1[xp]);
    return f32x4{fmaf(0.375f, a0, 0.625f * a1), fmaf(0.125f, a0, 0.875f * a1),
                 fmaf(0.125f, a2, 0.875f * a1), fmaf(0.375f, a2, 0.625f * a1)};
  };

  // march 1: m = max, kr = arg max, z = sum e, acc = sum e (K - kr)
  float m[4], z[4], acc[4], kr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = -INFINITY, z[i] = 0.f, acc[i] = 0.f, kr[i] = 0.f;
  f32x4 prev = plane(0), cur = prev, nxt = plane(min(1, D - 1));
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
        const float kn = f0 + (u0 == cm ? 0.f : u1 == cm ? 1.f : u2 == cm ? 2.f : 3.f);
        const float sc = __expf(m[i] - cm);  // 0 on the first plane (m = -inf)
        acc[i] = fmaf(z[i], kr[i] - kn, acc[i]) * sc;  // re-referenced to the new arg max
        z[i] *= sc;
        m[i] = cm;
        kr[i] = kn;
      }
      const float e0 = __expf(u0 - m[i]), e1 = __expf(u1 - m[i]);
      const float e2 = __expf(u2 - m[i]), e3 = __expf(u3 - m[i]);
      const float o = f0 - kr[i];  // exact
      z[i] += (e0 + e1) + (e2 + e3);
      acc[i] += fmaf(e0, o, e1 * (o + 1.f)) + fmaf(e2, o + 2.f, e3 * (o + 3.f));
    }
    prev = cur;
    cur = nxt;
    nxt = nn;
  }
  // cf = s g / z (0 outside the image), off = sum p (K - kr)
  float cf[4], off[4];
  {
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    const f4u g = *reinterpret_cast<const f4u *>(gdisp + (b * 4 * H + Y) * (4L * W) + 4 * kx);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float inv = 1.f / z[i];
      off[i] = acc[i] * inv;
      cf[i] = inside ? sign * g[i] * inv : 0.f;
    }
  }

  // plane kp of this thread's four pixels -> LDS -> the owners' stores
  auto emit = [&](int kp, const float (&G)[4]) {
    const float L = fmaf(0.375f, G[0], 0.125f * G[1]), R = fmaf(0.125f, G[2], 0.375f * G[3]);
    float C = fmaf(0.625f, G[0], 0.875f * G[1]) + fmaf(0.875f, G[2], 0.625f * G[3]);
    if (kxu == 0) C += L;  // the clamped ends keep their outer shares
    if (kxu == W - 1) C += R;
    // column kx's sum: its own, the right share of kx-1, the left share of kx+1 (the window's
    // two edge columns are not owned, what they receive here is not read)
    const float s = C + __shfl_up(R, 1, BQ) + __shfl_down(L, 1, BQ);
    red[kp & 1][r][q] = s;
    __syncthreads();
    const int oy = ky0 + r;  // owners: r < TY, q = 1 .. TX
    if (r < TY && q >= 1 && q <= TX && kxu < W && oy < H) {
      const float (*col)[BQ] = &red[kp & 1][4 * r];
      const float w2 = oy == 0 ? 1.f : 0.625f, w3 = oy == 0 ? 1.f : 0.875f;
      const float w4 = oy == H - 1 ? 1.f : 0.875f, w5 = oy == H - 1 ? 1.f : 0.625f;
      float t = fmaf(0.125f, col[0][q], 0.375f * col[1][q]);
      t += fmaf(w2, col[2][q], w3 * col[3][q]);
      t += fmaf(w4, col[4][q], w5 * col[5][q]);
      t += fmaf(0.375f, col[6][q], 0.125f * col[7][q]);
      gcost[((b * D + kp) * H + oy) * (long)W + kxu] = t;
    }
  };

  // march 2
  float pend[4] = {}, carry[4] = {}, G[4] = {};
  prev = plane(0), cur = prev, nxt = plane(min(1, D - 1));
  for (int k = 0; k < D; ++k) {
    const f32x4 nn = plane(min(k + 2, D - 1));
    const float f0 = (float)(4 * k);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float u0 = fmaf(0.375f, prev[i], 0.625f * cur[i]);
      const float u1 = fmaf(0.125f, prev[i], 0.875f * cur[i]);
      const float u2 = fmaf(0.125f, nxt[i], 0.875f * cur[i]);
      const float u3 = fmaf(0.375f, nxt[i], 0.625f * cur[i]);
      const float o = f0 - kr[i];
      const float d0 = cf[i] * __expf(u0 - m[i]) * (o - off[i]);
      const float d1 = cf[i] * __expf(u1 - m[i]) * ((o + 1.f) - off[i]);
      const float d2 = cf[i] * __expf(u2 - m[i]) * ((o + 2.f) - off[i]);
      const float d3 = cf[i] * __expf(u3 - m[i]) * ((o + 3.f) - off[i]);
      const float lo = fmaf(0.375f, d0, 0.125f * d1);  // to plane k-1
      const float mid = fmaf(0.625f, d0, 0.875f * d1) + fmaf(0.875f, d2, 0.625f * d3);
      if (k == 0) {
        pend[i] = mid + lo;  // the clamped end keeps it
      } else {
        G[i] = pend[i] + lo;
        pend[i] = carry[i] + mid;
      }
      carry[i] = fmaf(0.125f, d2, 0.375f * d3);  // to plane k+1
    }
    if (k > 0) emit(k - 1, G);
    prev = cur;
    cur = nxt;
    nxt = nn;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) G[i] = pend[i] + carry[i];
  emit(D - 1, G);
}

}  // namespace

extern "C" int aanet_disp_regress_up4_bwd_f32(const float *cost, const float *grad_disp,
                                              float *grad_cost, int n, int d, int h, int w,
                                              int negate, aanet_stream_t stream) {
  AANET_HOST_CHECK(cost && grad_disp && grad_cost && n > 0 && d > 0 && h > 0 && w > 0);
  // candidates exact in fp32, fine coordinates in int
  if (d > (1 << 22) || h > (1 << 28) || w > (1 << 28)) return AANET_EUNSUPPORTED;
  const int tiles_x = (w + TX - 1) / TX, tiles_y = (h + TY - 1) / TY;
  const long nblk = (long)n * tiles_x * tiles_y;
  if (nblk > 0x7fffffffL) return AANET_EUNSUPPORTED;
  hipLaunchKernelGGL(disp_regress_up4_bwd_kernel, dim3((unsigned)nblk), dim3(BT), 0,
                     as_hip(stream), cost, grad_disp, grad_cost, d, h, w, tiles_x, tiles_y,
                     negate ? -1.f : 1.f);
  return aanet_launch_status();
}

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
