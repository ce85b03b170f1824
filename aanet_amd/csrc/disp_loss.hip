// disp_loss.hip -- what sits on the network's output in every training and validation step, for
// gfx950: the multi-scale disparity loss (model.py:109-134) with its backward, and the validation
// metrics (metric.py; model.py:142-148, 320-341).
//
// Loss forward: ONE pass over gt / mask (and the optional pseudo ground truth).  Every pyramid
// level is upsampled on the fly with the resize kernel's stencil (resize.h, bit-identical to
// ops.resize_bilinear) and scaled by W / w_k in a separate fp32 multiply, then
// smooth-L1(beta = 1) against gt, SELECTED by the mask (masked-out gt may be inf / NaN).
// Reduction, in a fixed order: per thread fp32 sums over its grid-stride pixels, a fixed-shape
// tree over the block (shuffles inside a wave, then the waves in order), one partial per block in
// the caller's workspace; a second one-block launch adds the partials in block order in double.
// Pixel counts are integers.  No atomics: the result is bit-reproducible.
//
// Loss backward: a gather per prediction element, the form of resize_bilinear_bwd_kernel: the
// element sums axis weights x scale x clamp(d, -1, 1) x w_k / count over the outputs whose 2x2
// stencil covers it, d recomputed from pred_k and gt (no full-resolution temporary).  A group of
// 16 or 64 lanes shares one element (at x12 it covers 26 x 26 outputs): lane l takes window
// positions l, l + lanes, ... in order, then a fixed-shape shuffle tree (fp32 terms, summed in
// double) -- the sum depends on the shapes only, never on the launch geometry.  The upstream
// gradient and the counts are read from the device: nothing here synchronises the host.
//
// Metrics: the loss forward's pass and partial scheme with one prediction: valid count, sum |e|,
// the D1 count and #(e > t) per threshold; the counts are integers, hence exact.
#include "common.h"
#include "resize.h"

namespace {

constexpr int MAXL = AANET_LOSS_MAX_LEVELS;
constexpr int MAXT = AANET_METRICS_MAX_THRESHOLDS;
constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int PIXELS_PER_THREAD = 4;  // what the grid is sized for, up to MAX_BLOCKS
constexpr int MAX_BLOCKS = 512;       // partials the one-block finishing launch adds in order

typedef unsigned long long u64;

struct Target {  // what every level is compared with
  const float *gt, *pgt;            // pgt, pmask: NULL without pseudo ground truth
  const unsigned char *mask, *pmask;
  int B, H, W;
};

struct LossArgs {
  const float *pred[MAXL];
  int h[MAXL], w[MAXL];
  float sh[MAXL], sw[MAXL];  // input/output size ratios (area_pixel_compute_scale)
  float scale[MAXL];         // (float)W / (float)w_k
  float weight[MAXL];
  int levels;
  Target t;
};

// up * scale - gt with the product rounded on its own (ops.resize_bilinear(pred) * scale, then
// the subtraction of smooth_l1): never contracted into one FMA
__device__ __forceinline__ float scaled_diff(float up, float scale, float gt) {
#pragma clang fp contract(off)
  const float p = up * scale;
  return p - gt;
}

// the same product where the subtraction comes later (|gt - up * scale| of the metrics)
__device__ __forceinline__ float scaled(float up, float scale) {
#pragma clang fp contract(off)
  return up * scale;
}

__device__ __forceinline__ float smooth_l1(float d) {
  const float z = fabsf(d);
  return z < 1.f ? 0.5f * z * z : z - 0.5f;
}

__device__ __forceinline__ float clamp1(float d) { return fminf(fmaxf(d, -1.f), 1.f); }

// sum over the wave in a fixed tree; lane 0 holds it
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// sum of part[0], part[stride], ... (n values) in that order, in double; the LDS reads go out 16
// at a time, ahead of the dependent adds
__device__ __forceinline__ double ordered_sum(const float *part, int n, int stride) {
  double s = 0.0;
  int g = 0;
  for (; g + 16 <= n; g += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = part[(g + u) * stride];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += (double)v[u];
  }
  for (; g < n; ++g) s += (double)part[g * stride];
  return s;
}

static int grid_for(long pixels) {
  long g = (pixels + (long)BLOCK * PIXELS_PER_THREAD - 1) / ((long)BLOCK * PIXELS_PER_THREAD);
  return (int)(g < 1 ? 1 : (g > MAX_BLOCKS ? MAX_BLOCKS : g));
}

// ------------------------------------------------------------------------ loss forward ---
// workspace: float sums[blocks][2 * MAXL] (level k at k, its pseudo term at MAXL + k), then
// u64 counts[blocks][2]
__global__ __launch_bounds__(BLOCK) void disp_loss_fwd_kernel(LossArgs a, float *__restrict__ psum,
                                                              u64 *__restrict__ pcnt) {
  const Target &t = a.t;
  const long HW = (long)t.H * t.W, total = t.B * HW;
  const bool pseudo = t.pgt != nullptr;
  float acc[MAXL], pacc[MAXL];
#pragma unroll
  for (int k = 0; k < MAXL; ++k) acc[k] = pacc[k] = 0.f;
  u64 cnt = 0, pc = 0;
  for (long e = (long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * BLOCK) {
    const long b = e / HW;
    const int q = (int)(e - b * HW), y = q / t.W, x = q - y * t.W;
    const bool m = t.mask[e] != 0;
    const float g = t.gt[e];
    bool pm = false;
    float pg = 0.f;
    if (pseudo) {
      pm = t.pmask[e] != 0;
      pg = t.pgt[e];
    }
    cnt += m ? 1 : 0;
    pc += pm ? 1 : 0;
#pragma unroll
    for (int k = 0; k < MAXL; ++k) {
      if (k >= a.levels) break;
      float d, pd;
      if (a.w[k] == t.W) {  // full resolution: read directly, no scale (model.py:114)
        const float v = a.pred[k][e];
        d = v - g;
        pd = v - pg;
      } else {
        const float up = bilinear_resize_fma(a.pred[k] + b * a.h[k] * a.w[k], a.h[k], a.w[k],
                                             a.sh[k], a.sw[k], y, x);
        d = scaled_diff(up, a.scale[k], g);
        pd = scaled_diff(up, a.scale[k], pg);
      }
      acc[k] += m ? smooth_l1(d) : 0.f;
      if (pseudo) pacc[k] += pm ? smooth_l1(pd) : 0.f;
    }
  }
  __shared__ float ssum[WAVES][2 * MAXL];
  __shared__ u64 scnt[WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < MAXL; ++k) {
    if (k >= a.levels) break;
    const float s = wave_sum(acc[k]);
    const float p = pseudo ? wave_sum(pacc[k]) : 0.f;
    if (lane == 0) {
      ssum[wave][k] = s;
      ssum[wave][MAXL + k] = p;
    }
  }
  cnt = wave_sum(cnt);
  pc = wave_sum(pc);
  if (lane == 0) {
    scnt[wave][0] = cnt;
    scnt[wave][1] = pc;
  }
  __syncthreads();
  if (threadIdx.x < 2 * MAXL) {
    const int j = threadIdx.x, k = j < MAXL ? j : j - MAXL;
    float s = 0.f;
    if (k < a.levels)
      for (int w = 0; w < WAVES; ++w) s += ssum[w][j];
    psum[(long)blockIdx.x * 2 * MAXL + j] = s;
  } else if (threadIdx.x < 2 * MAXL + 2) {
    const int j = threadIdx.x - 2 * MAXL;
    u64 s = 0;
    for (int w = 0; w < WAVES; ++w) s += scnt[w][j];
    pcnt[(long)blockIdx.x * 2 + j] = s;
  }
}

struct LossOut {
  float *per_level, *pseudo_per_level, *total;
  long *count, *pseudo_count;
};

// One block.  The float partials are staged in LDS by all threads (a thread adding them straight
// from memory waits for one load after the other); thread j then adds partial j of every block,
// in block order, in double.  Integer counts are associative: the first wave adds them as a tree.
__global__ __launch_bounds__(BLOCK) void disp_loss_finish_kernel(const float *__restrict__ psum,
                                                                 const u64 *__restrict__ pcnt,
                                                                 int blocks, LossArgs a, LossOut o) {
  __shared__ float part[MAX_BLOCKS * 2 * MAXL];
  __shared__ double sum[2 * MAXL];
  __shared__ u64 cnt[2];
  const int j = threadIdx.x;
  for (int i = j; i < blocks * 2 * MAXL; i += BLOCK) part[i] = psum[i];
  if (j < 64) {
    u64 c0 = 0, c1 = 0;
    for (int g = j; g < blocks; g += 64) {
      c0 += pcnt[2 * g];
      c1 += pcnt[2 * g + 1];
    }
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
    if (j == 0) {
      cnt[0] = c0;
      cnt[1] = c1;
    }
  }
  __syncthreads();
  if (j < 2 * MAXL) sum[j] = ordered_sum(part + j, blocks, 2 * MAXL);
  __syncthreads();
  if (j != 0) return;
  const bool pseudo = a.t.pgt != nullptr;
  double total = 0.0;
  for (int k = 0; k < a.levels; ++k) {
    const double lvl = sum[k] / (double)cnt[0];  // 0 / 0 = NaN on an empty mask, as the mean is
    const double pl = pseudo ? sum[MAXL + k] / (double)cnt[1] : 0.0;
    o.per_level[k] = (float)lvl;
    o.pseudo_per_level[k] = (float)pl;
    total += (double)a.weight[k] * (lvl + pl);
  }
  *o.total = (float)total;
  *o.count = (long)cnt[0];
  *o.pseudo_count = (long)cnt[1];
}

// ----------------------------------------------------------------------- loss backward ---
// d total / d (upsampled, scaled prediction) at output pixel o, before the `* scale` of the
// upsampling: grad_total * w_k / count * clamp(d, -1, 1) where the mask is set, plus the pseudo term
__device__ __forceinline__ float pixel_grad(const Target &t, long o, float v, float scale,
                                            bool scaled, float coef, float pcoef) {
  const float g = t.gt[o];
  const float d = scaled ? scaled_diff(v, scale, g) : v - g;
  float go = t.mask[o] != 0 ? coef * clamp1(d) : 0.f;
  if (t.pgt) {
    const float pg = t.pgt[o];
    const float pd = scaled ? scaled_diff(v, scale, pg) : v - pg;
    go += t.pmask[o] != 0 ? pcoef * clamp1(pd) : 0.f;
  }
  return go;
}

// a level at full resolution: one thread per element
__global__ __launch_bounds__(BLOCK) void disp_loss_bwd_direct_kernel(
    const float *__restrict__ pred, float *__restrict__ grad, float weight, Target t,
    const float *__restrict__ grad_total, const long *__restrict__ count,
    const long *__restrict__ pseudo_count) {
  const long total = (long)t.B * t.H * t.W;
  const float gw = *grad_total * weight;
  const float coef = gw / (float)*count, pcoef = t.pgt ? gw / (float)*pseudo_count : 0.f;
  for (long e = (long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * BLOCK)
    grad[e] = pixel_grad(t, e, pred[e], 1.f, false, coef, pcoef);
}

// an upsampled level: LANES lanes per element
template <int LANES>
__global__ __launch_bounds__(BLOCK) void disp_loss_bwd_up_kernel(
    const float *__restrict__ pred, float *__restrict__ grad, int ih, int iw, float sh, float sw,
    float scale, float weight, Target t, const float *__restrict__ grad_total,
    const long *__restrict__ count, const long *__restrict__ pseudo_count) {
  constexpr int PER_BLOCK = BLOCK / LANES;
  const long total = (long)t.B * ih * iw;
  const int lane = threadIdx.x % LANES;
  const float gw = *grad_total * weight;
  const float coef = gw / (float)*count, pcoef = t.pgt ? gw / (float)*pseudo_count : 0.f;
  // e is the same in all lanes of a group, so a group stays together through the shuffles
  for (long e = (long)blockIdx.x * PER_BLOCK + threadIdx.x / LANES; e < total;
       e += (long)gridDim.x * PER_BLOCK) {
    const int x = (int)(e % iw);
    const long r = e / iw;
    const int y = (int)(r % ih);
    const long b = r / ih;
    // the outputs whose source coordinate lies in (i - 1, i + 1), with a margin for rounding
    // (resize_bilinear_bwd_kernel's bounds); outputs outside get weight 0.  Trimming the window
    // to the outputs of non-zero weight measured slower: the trimming is serial, the positions
    // it saves are spread over the lanes.
    const int ylo = max(0, (int)floorf(((float)y - 0.5f) / sh - 0.5f) - 1);
    const int yhi = min(t.H - 1, (int)ceilf(((float)y + 1.5f) / sh - 0.5f) + 1);
    const int xlo = max(0, (int)floorf(((float)x - 0.5f) / sw - 0.5f) - 1);
    const int xhi = min(t.W - 1, (int)ceilf(((float)x + 1.5f) / sw - 0.5f) + 1);
    const int nw = xhi - xlo + 1, np = (yhi - ylo + 1) * nw;
    const float *im = pred + b * ih * iw;
    // every term is rounded to fp32 as the unfused chain rounds it; the SUM is kept in double, so
    // that one dominant term (a lone valid pixel among pseudo ones) loses nothing to the order
    double acc = 0.0;
    for (int p = lane; p < np; p += LANES) {
      const int py = p / nw, oy = ylo + py, ox = xlo + (p - py * nw);
      const float wy = bilinear_axis_weight(oy, y, sh, ih), wx = bilinear_axis_weight(ox, x, sw, iw);
      if (wy == 0.f || wx == 0.f) continue;
      const float up = bilinear_resize_fma(im, ih, iw, sh, sw, oy, ox);
      const float go = pixel_grad(t, ((long)b * t.H + oy) * t.W + ox, up, scale, true, coef, pcoef);
      // the roundings of the unfused chain per term: (go * scale), x wx, x wy
      acc += (double)(wy * (wx * (go * scale)));
    }
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) acc += __shfl_down(acc, o, LANES);
    if (lane == 0) grad[e] = (float)acc;
  }
}

// ----------------------------------------------------------------------------- metrics ---
struct MetricArgs {
  const float *pred;
  int h, w;
  float sh, sw, scale;
  int nt;
  float thres[MAXT];
  Target t;
};

constexpr int MCOUNTS = 2 + MAXT;  // valid, D1, thresholds

// workspace: float abs_sum[blocks], padded to 8 bytes, then u64 counts[blocks][MCOUNTS]
__global__ __launch_bounds__(BLOCK) void disp_metrics_kernel(MetricArgs a, float *__restrict__ psum,
                                                             u64 *__restrict__ pcnt) {
  const Target &t = a.t;
  const long HW = (long)t.H * t.W, total = t.B * HW;
  float acc = 0.f;
  unsigned cnt[MCOUNTS];  // per thread: at most total / (blocks * BLOCK) pixels, checked on the host
#pragma unroll
  for (int j = 0; j < MCOUNTS; ++j) cnt[j] = 0;
  for (long e = (long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * BLOCK) {
    const long b = e / HW;
    const int q = (int)(e - b * HW), y = q / t.W, x = q - y * t.W;
    const bool m = t.mask[e] != 0;
    const float g = t.gt[e];
    float v;
    if (a.w == t.W) {
      v = a.pred[e];
    } else {
      v = scaled(bilinear_resize_fma(a.pred + b * a.h * a.w, a.h, a.w, a.sh, a.sw, y, x), a.scale);
    }
    const float err = fabsf(g - v);
    acc += m ? err : 0.f;
    cnt[0] += m ? 1 : 0;
    cnt[1] += m && err > 3.f && __fdiv_rn(err, g) > 0.05f ? 1 : 0;
#pragma unroll
    for (int j = 0; j < MAXT; ++j)
      if (j < a.nt) cnt[2 + j] += m && err > a.thres[j] ? 1 : 0;
  }
  __shared__ float ssum[WAVES];
  __shared__ u64 scnt[WAVES][MCOUNTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  acc = wave_sum(acc);
  if (lane == 0) ssum[wave] = acc;
#pragma unroll
  for (int j = 0; j < MCOUNTS; ++j) {
    const u64 s = wave_sum((u64)cnt[j]);
    if (lane == 0) scnt[wave][j] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < WAVES; ++w) s += ssum[w];
    psum[blockIdx.x] = s;
  } else if (threadIdx.x <= MCOUNTS) {
    const int j = threadIdx.x - 1;
    u64 s = 0;
    for (int w = 0; w < WAVES; ++w) s += scnt[w][j];
    pcnt[(long)blockIdx.x * MCOUNTS + j] = s;
  }
}

// out: [epe, d1, thres_0 ...] as means over the valid pixels (NaN when there is none, as the
// mean over an empty selection is); count: the valid pixels.  One block: wave q adds the integer
// counts q, q + WAVES, ... as trees; thread 0 adds the staged |e| partials in block order in double.
__global__ __launch_bounds__(BLOCK) void disp_metrics_finish_kernel(const float *__restrict__ psum,
                                                                    const u64 *__restrict__ pcnt,
                                                                    int blocks, int nt,
                                                                    float *__restrict__ out,
                                                                    long *__restrict__ count) {
  __shared__ float part[MAX_BLOCKS];
  __shared__ u64 cnt[MCOUNTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < blocks; i += BLOCK) part[i] = psum[i];
  for (int q = wave; q < MCOUNTS; q += WAVES) {
    u64 c = 0;
    for (int g = lane; g < blocks; g += 64) c += pcnt[(long)g * MCOUNTS + q];
    c = wave_sum(c);
    if (lane == 0) cnt[q] = c;
  }
  __syncthreads();
  const int j = threadIdx.x;
  const double n = (double)cnt[0];
  if (j == 0) {
    out[0] = (float)(ordered_sum(part, blocks, 1) / n);
    *count = (long)cnt[0];
  } else if (j < 2 + nt) {
    out[j] = (float)((double)cnt[j] / n);  // cnt[1] = D1, cnt[2 + t] = threshold t
  }
}

size_t metrics_sum_bytes(int blocks) { return ((size_t)blocks * sizeof(float) + 7) & ~(size_t)7; }

// the checks that the three entries share; AANET_OK, or the status to return
int check_target(const float *gt, const unsigned char *mask, const float *pgt,
                 const unsigned char *pmask, int b, int h, int w) {
  if (!gt || !mask || b <= 0 || h <= 0 || w <= 0) return AANET_EINVAL;
  if ((pgt == nullptr) != (pmask == nullptr)) return AANET_EINVAL;
  if ((long)h * w > 0x7fffffffL) return AANET_EUNSUPPORTED;  // the in-image index is an int
  return AANET_OK;
}

int check_level(const float *pred, int ph, int pw, int h, int w) {
  if (!pred || ph <= 0 || pw <= 0) return AANET_EINVAL;
  if (pw == w && ph != h) return AANET_EINVAL;
  if (ph > h || pw > w) return AANET_EUNSUPPORTED;
  return AANET_OK;
}

int fill_args(LossArgs &a, int levels, const float *const *preds, const int *pred_h,
              const int *pred_w, const float *weights, const float *gt, const unsigned char *mask,
              const float *pgt, const unsigned char *pmask, int b, int h, int w) {
  if (levels < 1 || levels > MAXL || !preds || !pred_h || !pred_w || !weights) return AANET_EINVAL;
  if (int rc = check_target(gt, mask, pgt, pmask, b, h, w)) return rc;
  for (int k = 0; k < MAXL; ++k) {
    const bool on = k < levels;
    if (on)
      if (int rc = check_level(preds[k], pred_h[k], pred_w[k], h, w)) return rc;
    a.pred[k] = on ? preds[k] : nullptr;
    a.h[k] = on ? pred_h[k] : 1;
    a.w[k] = on ? pred_w[k] : 1;
    a.sh[k] = (float)a.h[k] / (float)h;
    a.sw[k] = (float)a.w[k] / (float)w;
    a.scale[k] = (float)w / (float)a.w[k];
    a.weight[k] = on ? weights[k] : 0.f;
  }
  a.levels = levels;
  a.t = Target{gt, pgt, mask, pmask, b, h, w};
  return AANET_OK;
}

}  // namespace

extern "C" size_t aanet_disp_loss_workspace_size(int levels, int b, int h, int w) {
  if (levels < 1 || levels > MAXL || b <= 0 || h <= 0 || w <= 0) return 0;
  return (size_t)grid_for((long)b * h * w) * (2 * MAXL * sizeof(float) + 2 * sizeof(u64));
}

extern "C" int aanet_disp_loss_f32(int levels, const float *const *preds, const int *pred_h,
                                   const int *pred_w, const float *weights, const float *gt,
                                   const unsigned char *mask, const float *pseudo_gt,
                                   const unsigned char *pseudo_mask, int b, int h, int w,
                                   float *per_level, float *pseudo_per_level, float *total,
                                   long *count, long *pseudo_count, void *workspace,
                                   size_t workspace_bytes, aanet_stream_t stream) {
  LossArgs a;
  if (int rc = fill_args(a, levels, preds, pred_h, pred_w, weights, gt, mask, pseudo_gt,
                         pseudo_mask, b, h, w))
    return rc;
  AANET_HOST_CHECK(per_level && pseudo_per_level && total && count && pseudo_count && workspace);
  AANET_HOST_CHECK(workspace_bytes >= aanet_disp_loss_workspace_size(levels, b, h, w));
  const int blocks = grid_for((long)b * h * w);
  float *psum = static_cast<float *>(workspace);
  u64 *pcnt = reinterpret_cast<u64 *>(psum + (size_t)blocks * 2 * MAXL);
  hipLaunchKernelGGL(disp_loss_fwd_kernel, dim3(blocks), dim3(BLOCK), 0, as_hip(stream), a, psum,
                     pcnt);
  hipLaunchKernelGGL(disp_loss_finish_kernel, dim3(1), dim3(BLOCK), 0, as_hip(stream), psum, pcnt,
                     blocks, a, LossOut{per_level, pseudo_per_level, total, count, pseudo_count});
  return aanet_launch_status();
}

extern "C" int aanet_disp_loss_bwd_f32(int levels, const float *const *preds,
                                       float *const *grad_preds, const int *pred_h,
                                       const int *pred_w, const float *weights, const float *gt,
                                       const unsigned char *mask, const float *pseudo_gt,
                                       const unsigned char *pseudo_mask, int b, int h, int w,
                                       const float *grad_total, const long *count,
                                       const long *pseudo_count, aanet_stream_t stream) {
  LossArgs a;
  if (int rc = fill_args(a, levels, preds, pred_h, pred_w, weights, gt, mask, pseudo_gt,
                         pseudo_mask, b, h, w))
    return rc;
  AANET_HOST_CHECK(grad_preds && grad_total && count && (pseudo_count || !pseudo_gt));
  for (int k = 0; k < levels; ++k) AANET_HOST_CHECK(grad_preds[k]);
  for (int k = 0; k < levels; ++k) {
    const long elems = (long)b * a.h[k] * a.w[k];
    if (a.w[k] == w) {
      long g = (elems + BLOCK - 1) / BLOCK;
      if (g > 65536) g = 65536;
      hipLaunchKernelGGL(disp_loss_bwd_direct_kernel, dim3((unsigned)g), dim3(BLOCK), 0,
                         as_hip(stream), a.pred[k], grad_preds[k], a.weight[k], a.t, grad_total,
                         count, pseudo_count);
      continue;
    }
    // the window of one element: about 2 / ratio + 4 outputs per axis; 16 lanes up to 64 outputs
    const float win = (2.f / a.sh[k] + 4.f) * (2.f / a.sw[k] + 4.f);
    const int lanes = win <= 64.f ? 16 : 64;
    long g = (elems + BLOCK / lanes - 1) / (BLOCK / lanes);
    if (g > 65536) g = 65536;
    if (lanes == 16)
      hipLaunchKernelGGL(disp_loss_bwd_up_kernel<16>, dim3((unsigned)g), dim3(BLOCK), 0,
                         as_hip(stream), a.pred[k], grad_preds[k], a.h[k], a.w[k], a.sh[k], a.sw[k],
                         a.scale[k], a.weight[k], a.t, grad_total, count, pseudo_count);
    else
      hipLaunchKernelGGL(disp_loss_bwd_up_kernel<64>, dim3((unsigned)g), dim3(BLOCK), 0,
                         as_hip(stream), a.pred[k], grad_preds[k], a.h[k], a.w[k], a.sh[k], a.sw[k],
                         a.scale[k], a.weight[k], a.t, grad_total, count, pseudo_count);
  }
  return aanet_launch_status();
}

extern "C" size_t aanet_disp_metrics_workspace_size(int b, int h, int w) {
  if (b <= 0 || h <= 0 || w <= 0) return 0;
  const int blocks = grid_for((long)b * h * w);
  return metrics_sum_bytes(blocks) + (size_t)blocks * MCOUNTS * sizeof(u64);
}

extern "C" int aanet_disp_metrics_f32(const float *pred, int pred_h, int pred_w, const float *gt,
                                      const unsigned char *mask, int b, int h, int w,
                                      int num_thresholds, const float *thresholds, float *out,
                                      long *count, void *workspace, size_t workspace_bytes,
                                      aanet_stream_t stream) {
  if (int rc = check_target(gt, mask, nullptr, nullptr, b, h, w)) return rc;
  if (int rc = check_level(pred, pred_h, pred_w, h, w)) return rc;
  AANET_HOST_CHECK(num_thresholds >= 0 && num_thresholds <= MAXT && (thresholds || !num_thresholds));
  AANET_HOST_CHECK(out && count && workspace);
  AANET_HOST_CHECK(workspace_bytes >= aanet_disp_metrics_workspace_size(b, h, w));
  const long pixels = (long)b * h * w;
  const int blocks = grid_for(pixels);
  // the per-thread counters are 32-bit
  if (pixels / ((long)blocks * BLOCK) >= 0x7fffffffL) return AANET_EUNSUPPORTED;
  MetricArgs a;
  a.pred = pred;
  a.h = pred_h;
  a.w = pred_w;
  a.sh = (float)pred_h / (float)h;
  a.sw = (float)pred_w / (float)w;
  a.scale = (float)w / (float)pred_w;
  a.nt = num_thresholds;
  for (int j = 0; j < MAXT; ++j) a.thres[j] = j < num_thresholds ? thresholds[j] : 0.f;
  a.t = Target{gt, nullptr, mask, nullptr, b, h, w};
  float *psum = static_cast<float *>(workspace);
  u64 *pcnt = reinterpret_cast<u64 *>(static_cast<char *>(workspace) + metrics_sum_bytes(blocks));
  hipLaunchKernelGGL(disp_metrics_kernel, dim3(blocks), dim3(BLOCK), 0, as_hip(stream), a, psum,
                     pcnt);
  hipLaunchKernelGGL(disp_metrics_finish_kernel, dim3(1), dim3(BLOCK), 0, as_hip(stream), psum, pcnt,
                     blocks, num_thresholds, out, count);
  return aanet_launch_status();
}
