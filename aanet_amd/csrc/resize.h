// resize.h -- device helpers of the bilinear resize (PyTorch upsample_bilinear2d,
// align_corners=False), shared by csa.hip (CSA sum, resize forward / backward) and disp_loss.hip
// (the loss's and the metrics' on-the-fly upsampling).
#pragma once

#include "common.h"

// PyTorch upsample_bilinear2d, align_corners=False: src = scale*(dst+0.5)-0.5, clamped at 0;
// i1 = (int)src; i1p = i1 < in-1; lambda = src - i1.
__device__ __forceinline__ float bilinear_resize(const float *__restrict__ im, int ih, int iw,
                                                 float sh, float sw, int y, int x) {
  float hr = sh * ((float)y + 0.5f) - 0.5f;
  hr = hr < 0.f ? 0.f : hr;
  float wr = sw * ((float)x + 0.5f) - 0.5f;
  wr = wr < 0.f ? 0.f : wr;
  const int h1 = (int)hr, w1 = (int)wr;
  const int h1p = h1 < ih - 1 ? 1 : 0, w1p = w1 < iw - 1 ? 1 : 0;
  const float h1l = hr - (float)h1, h0l = 1.f - h1l;
  const float w1l = wr - (float)w1, w0l = 1.f - w1l;
  const float *r0 = im + (long)h1 * iw, *r1 = im + (long)(h1 + h1p) * iw;
  return h0l * (w0l * r0[w1] + w1l * r0[w1 + w1p]) + h1l * (w0l * r1[w1] + w1l * r1[w1 + w1p]);
}

// Weight of input index i in output index o along one axis (the align_corners=False rule of
// bilinear_resize): lambda0 if i is o's lower tap, lambda1 if its upper one (both at the edge).
__device__ __forceinline__ float bilinear_axis_weight(int o, int i, float s, int in) {
  float r = s * ((float)o + 0.5f) - 0.5f;
  r = r < 0.f ? 0.f : r;
  const int i1 = (int)r, i1p = i1 < in - 1 ? 1 : 0;
  const float l1 = r - (float)i1, l0 = 1.f - l1;
  return (i1 == i ? l0 : 0.f) + (i1 + i1p == i ? l1 : 0.f);
}

// Output (oy, ox) of the resize of one plane im [ih][iw], bit-identical to torch's kernel: the 2x2
// stencil of bilinear_axis_weight's rule, combined in the reference kernel's order (rows of the
// stencil first) with explicit FMAs: the contraction torch's kernel gets (tools/resize_lab.hip:
// bit-identical for this form only; plain or differently fused expressions differ in 2-40% of
// the outputs).
__device__ __forceinline__ float bilinear_resize_fma(const float *__restrict__ im, int ih, int iw,
                                                     float sh, float sw, int oy, int ox) {
  float ry = __builtin_fmaf(sh, (float)oy + 0.5f, -0.5f), rx = __builtin_fmaf(sw, (float)ox + 0.5f, -0.5f);
  ry = ry < 0.f ? 0.f : ry;
  rx = rx < 0.f ? 0.f : rx;
  const int y1 = (int)ry, x1 = (int)rx;
  const int y1p = y1 < ih - 1 ? iw : 0, x1p = x1 < iw - 1 ? 1 : 0;
  const float ly1 = ry - (float)y1, ly0 = 1.f - ly1, lx1 = rx - (float)x1, lx0 = 1.f - lx1;
  const float *p = im + (long)y1 * iw + x1;
  return __builtin_fmaf(ly0, __builtin_fmaf(lx0, p[0], lx1 * p[x1p]),
                        ly1 * __builtin_fmaf(lx0, p[y1p], lx1 * p[y1p + x1p]));
}
