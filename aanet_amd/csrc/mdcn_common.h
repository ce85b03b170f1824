// mdcn_common.h -- what the conv engine (mdcn.hip) and the DCN / conv training backward
// (mdcn_bwd.hip) share: the kernel argument struct, the reference's bilinear sampler, the tile
// constants and the host helpers both call (defined once, in mdcn.hip).
//
// Bit-exactness: the coordinate h = float(int) + offset is one fp32 add (kernel.cu:615-616);
// floor / bilinear follow kernel.cu:467-497 with fp contraction disabled, so im2col values
// and sampling indices equal the CPU oracle's bit for bit (tests/test_gpu_mdcn.py).
#pragma once

#include "split.h"

namespace mdcn {  // tile constants: `using namespace mdcn;` in the units that take them
constexpr int NT = 256;    // threads per workgroup (backward kernels)
constexpr int PT = 64;     // pixels per workgroup tile
constexpr int KC = 32;     // max channels per K chunk
constexpr int CP = PT + 16;  // sCol pitch (floats): rows r, r+1 land 16 banks apart
}  // namespace mdcn

typedef bf16x8 bf16x8_t;  // the engine's name for split.h's fragment type

struct MdcnArgs {
  const float *x;
  const float *offset;
  long off_bs;
  const float *mask;
  long mask_bs;
  int mask_logits;
  float mask_scale;
  const float *weight;
  const float *bias;
  const float *post_scale;
  const float *post_shift;
  const float *residual;  // added before the (last) activation, same shape as out, or NULL
  int act;
  // pointwise tail (bottleneck conv3 fused into this conv's epilogue); tail_w == NULL: none.
  // out = tail_act(tail_w . act(post_scale*(conv + bias) + post_shift) + tail_b + residual)
  const float *tail_w;  // packed [Co2][Co]
  const float *tail_b;
  int tail_act, Co2;
  float *out;
  int N, C, H, W, Co, kh, kw, stride, pad, dil, groups, dg, Ho, Wo;
  int layout;  // AANET_LAYOUT_* bits (conv engine only)
  int split;   // conv engine: split-bf16 contraction (AANET_CONV_EXACT_F32 clear, weights carry pieces)
  int halo;    // conv engine: 3x3 stride-1 halo-tile form (conv_fwd_kernel HALO)
  const bf16x8_t *wsplit, *tail_wsplit;  // bf16 piece fragments of weight / tail_w (split_frag_offset)
  int dbg_noatom;  // AANET_DCN_BWD_DBG=1: the backward data kernels skip the grad_x scatter (timing)
  // CSA epilogue (tail kernels): csa_out = csa_act(out + sum_j up_r[j](up[j])), r = 2 or 4
  float *csa_out;
  const float *up[3];
  int up_h[3], up_w[3], up_r[3], num_up, csa_act;
  const aanet_post_stage_t *post;  // HOST pointer (launch checks only): the post stage on csa_out
  // its fields for the device (HALO 1 tail, POST instantiation)
  const char *post_w;     // split fragments of the [64][64] 1x1 weight
  const float *post_b;
  int post_act;
  float *post_out;        // NHWC [N][Ho][Wo][64]
};

// Bilinear sampling state of one (pixel, tap, deformable group).  Invalid corners get
// weight 0 and a clamped (valid) address, which reproduces the reference's `v = 0` branch
// exactly: w*0 adds a zero term, as 0-valued v does in kernel.cu:478-493.
struct Samp {
  int i1, i2, i3, i4;
  float w1, w2, w3, w4;
  float m;
  float lh, lw;   // fractional parts (backward)
  int hl, wl;     // floor of the sampling position (backward window form)
  int valid;
  int ok;         // corner validity bits (backward)
};

__device__ __forceinline__ void make_samp(Samp &s, float h, float w, int H, int W, float m) {
#pragma clang fp contract(off)
  const bool valid = h > -1.f && w > -1.f && h < (float)H && w < (float)W;
  const int hl = (int)floorf(h), wl = (int)floorf(w);
  const float lh = h - (float)hl, lw = w - (float)wl;
  const float hh = 1.f - lh, hw = 1.f - lw;
  const bool ok1 = valid && hl >= 0 && wl >= 0;
  const bool ok2 = valid && hl >= 0 && wl + 1 <= W - 1;
  const bool ok3 = valid && hl + 1 <= H - 1 && wl >= 0;
  const bool ok4 = valid && hl + 1 <= H - 1 && wl + 1 <= W - 1;
  s.w1 = ok1 ? hh * hw : 0.f;
  s.w2 = ok2 ? hh * lw : 0.f;
  s.w3 = ok3 ? lh * hw : 0.f;
  s.w4 = ok4 ? lh * lw : 0.f;
  s.i1 = ok1 ? hl * W + wl : 0;
  s.i2 = ok2 ? hl * W + wl + 1 : 0;
  s.i3 = ok3 ? (hl + 1) * W + wl : 0;
  s.i4 = ok4 ? (hl + 1) * W + wl + 1 : 0;
  s.m = m;
  s.lh = lh;
  s.lw = lw;
  s.hl = hl;
  s.wl = wl;
  s.valid = valid;
  s.ok = (ok1 ? 1 : 0) | (ok2 ? 2 : 0) | (ok3 ? 4 : 0) | (ok4 ? 8 : 0);
}

// kernel.cu:494-496 then `val * mask` (kernel.cu:627): ((w1 v1 + w2 v2) + w3 v3) + w4 v4.
__device__ __forceinline__ float samp_val(const float *__restrict__ im, const Samp &s) {
#pragma clang fp contract(off)
  const float v = s.w1 * im[s.i1] + s.w2 * im[s.i2] + s.w3 * im[s.i3] + s.w4 * im[s.i4];
  return v * s.m;
}

// Forward form of the sampler: the two horizontal corners of a row are read with ONE 8-byte
// load (dword aligned) at a column base clamped into [0, W-2]; invalid corners carry weight 0
// so the clamped read never changes the value.  Same products and sum order as samp_val.
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
struct Samp2 {
  int itop, ibot;   // element offsets of the 2-wide column pair in rows hl and hl+1
  int swap;         // 1 when the pair base is wl+1 (wl == -1) -> corners swapped
  float w1, w2, w3, w4, m;
};

__device__ __forceinline__ void make_samp2(Samp2 &s, float h, float w, int H, int W, float m) {
#pragma clang fp contract(off)
  const bool valid = h > -1.f && w > -1.f && h < (float)H && w < (float)W;
  const int hl = (int)floorf(h), wl = (int)floorf(w);
  const float lh = h - (float)hl, lw = w - (float)wl;
  const float hh = 1.f - lh, hw = 1.f - lw;
  const bool ok1 = valid && hl >= 0 && wl >= 0;
  const bool ok2 = valid && hl >= 0 && wl + 1 <= W - 1;
  const bool ok3 = valid && hl + 1 <= H - 1 && wl >= 0;
  const bool ok4 = valid && hl + 1 <= H - 1 && wl + 1 <= W - 1;
  s.w1 = ok1 ? hh * hw : 0.f;
  s.w2 = ok2 ? hh * lw : 0.f;
  s.w3 = ok3 ? lh * hw : 0.f;
  s.w4 = ok4 ? lh * lw : 0.f;
  const int pb = valid ? min(max(wl, 0), W - 2) : 0;
  const int rt = valid ? min(max(hl, 0), H - 1) : 0;
  const int rb = valid ? min(max(hl + 1, 0), H - 1) : 0;
  s.itop = rt * W + pb;
  s.ibot = rb * W + pb;
  s.swap = (valid && pb != wl) ? 1 : 0;
  s.m = m;
}

__device__ __forceinline__ float samp_val2(const float *__restrict__ im, const Samp2 &s) {
#pragma clang fp contract(off)
  const f2u t = *reinterpret_cast<const f2u *>(im + s.itop);
  const f2u b = *reinterpret_cast<const f2u *>(im + s.ibot);
  const float v1 = s.swap ? t.y : t.x, v2 = s.swap ? t.x : t.y;
  const float v3 = s.swap ? b.y : b.x, v4 = s.swap ? b.x : b.y;
  const float v = s.w1 * v1 + s.w2 * v2 + s.w3 * v3 + s.w4 * v4;
  return v * s.m;
}

__device__ __forceinline__ float load_mask(const MdcnArgs &a, int n, int g, int k, int K, long P,
                                           long p) {
  const float v = a.mask[(long)n * a.mask_bs + ((long)g * K + k) * P + p];
  if (!a.mask_logits) return v;
  return a.mask_scale * (1.f / (1.f + expf(-v)));  // deform.py:86-89
}

// Sampling state for output pixel p of image n, tap k (= i*kw + j), deformable group g.
__device__ __forceinline__ void pixel_samp(Samp &s, const MdcnArgs &a, int n, int g, int k, long p,
                                           int ho, int wo) {
#pragma clang fp contract(off)
  const int K = a.kh * a.kw;
  const long P = (long)a.Ho * a.Wo;
  const int i = k / a.kw, j = k % a.kw;
  const float *off = a.offset + (long)n * a.off_bs + (long)g * 2 * K * P;
  const float oh = off[(long)(2 * k) * P + p], ow = off[(long)(2 * k + 1) * P + p];
  const float m = load_mask(a, n, g, k, K, P, p);
  const float h = (float)(ho * a.stride - a.pad + i * a.dil) + oh;
  const float w = (float)(wo * a.stride - a.pad + j * a.dil) + ow;
  make_samp(s, h, w, a.H, a.W, m);
}

__device__ __forceinline__ void pixel_samp2(Samp2 &s, const MdcnArgs &a, int n, int g, int k,
                                            long p, int ho, int wo) {
#pragma clang fp contract(off)
  const int K = a.kh * a.kw;
  const long P = (long)a.Ho * a.Wo;
  const int i = k / a.kw, j = k % a.kw;
  const float *off = a.offset + (long)n * a.off_bs + (long)g * 2 * K * P;
  const float oh = off[(long)(2 * k) * P + p], ow = off[(long)(2 * k + 1) * P + p];
  const float m = load_mask(a, n, g, k, K, P, p);
  const float h = (float)(ho * a.stride - a.pad + i * a.dil) + oh;
  const float w = (float)(wo * a.stride - a.pad + j * a.dil) + ow;
  make_samp2(s, h, w, a.H, a.W, m);
}

// ---- host helpers (mdcn.hip) ------------------------------------------------------------------
int check_shapes(const MdcnArgs &a);
MdcnArgs make_args(const float *x, const float *offset, long off_bs, const float *mask,
                   long mask_bs, int mask_logits, float mask_scale, const float *weight,
                   const float *bias, const float *ps, const float *psh, int act, float *out,
                   int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad,
                   int dil, int groups, int dg);
int round_pitch(int v, int mod32);  // smallest p >= v with p % 32 == mod32
