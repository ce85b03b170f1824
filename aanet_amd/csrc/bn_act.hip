// bn_act.hip -- training-mode BatchNorm fused with its activation and residual add:
//   y = act(gamma * (x - mean_batch) * invstd + beta [+ residual])        (aanet_bn_act_*)
// x is [N, C, S] (S = H*W or D*H*W), fp32, contiguous.  One kernel family in two forms, chosen
// from the shape alone (aanet_bn_act_plan):
//   one-launch: a workgroup owns a channel; pass 1 reduces its N segments, pass 2 re-reads them
//               (from L2 / the Infinity Cache at the 2-D training shapes) and writes y; the same
//               launch writes save_mean / save_invstd, the running statistics and the counter.
//   split:      grid C x splits; every workgroup writes its (sum, sum of squares) in double into
//               a caller-owned workspace, a finishing launch adds them in split order, the apply
//               launch follows.  Backward: partials, then an apply launch in which every
//               workgroup re-adds its channel's partials in the same order.
// Reductions: per-thread double accumulators, a xor butterfly inside the wave, the waves' sums
// added in wave order, the splits' partials in split order: a function of the shapes and the form
// only.  No atomics, no hand-off between workgroups inside a launch.
#include "common.h"

namespace {

constexpr int kOneThreads = 1024;  // one-launch form: 16 waves stream one channel
constexpr int kSplitThreads = 256;
constexpr int kMaxWaves = kOneThreads / 64;
constexpr int kMaxSplits = 4096;   // the apply workgroups re-add this many partials each
constexpr long kSegMin = 2048;     // segments at least this long are walked one by one

// How a workgroup walks its share of a channel.  The channel's N*S values have the logical index
// e = n*S + s; segment n starts at float offset (n*C + c)*S, 16-byte aligned only when that is a
// multiple of 4.
enum {
  PATH_SCALAR = 0,  // one value per lane at logical index e: any S, no idle lanes at S = 1, 2, 3
  PATH_VEC = 1,     // S % 4 == 0: one float4 per lane at logical quad e/4 (no quad straddles)
  PATH_SEG = 2      // long segments: scalar head up to the 16-byte boundary, float4 body, tail
};

typedef float f4a __attribute__((ext_vector_type(4), aligned(16)));

// Calls op.v4(off) for aligned quads and op.s1(off) for single values (off: float offset into the
// tensors) over the channel's logical range [e0, e1).  PATH_VEC needs e0 % 4 == 0.
template <class Op>
__device__ __forceinline__ void walk(Op &op, int path, int C, int c, int S, unsigned e0,
                                     unsigned e1, unsigned tid, unsigned nthr) {
  if (path == PATH_VEC) {
    const unsigned S4 = (unsigned)S >> 2;
    for (unsigned q = (e0 >> 2) + tid; q < (e1 >> 2); q += nthr) {
      const unsigned n = q / S4, sq = q - n * S4;
      op.v4((((long)n * C + c) * S4 + sq) << 2);
    }
  } else if (path == PATH_SEG) {
    unsigned e = e0;
    while (e < e1) {
      const unsigned n = e / (unsigned)S, s0 = e - n * (unsigned)S;
      const unsigned len = min((unsigned)S - s0, e1 - e);
      const long base = ((long)n * C + c) * S + s0;
      const unsigned head = min((unsigned)(-base) & 3u, len);
      if (tid < head) op.s1(base + tid);
      const unsigned nb = (len - head) >> 2;
      for (unsigned q = tid; q < nb; q += nthr) op.v4(base + head + 4l * q);
      const unsigned t0 = head + 4u * nb;
      if (tid < len - t0) op.s1(base + t0 + tid);
      e += len;
    }
  } else {
    for (unsigned e = e0 + tid; e < e1; e += nthr) {
      const unsigned n = e / (unsigned)S;
      op.s1(((long)n * C + c) * S + (e - n * (unsigned)S));
    }
  }
}

// Both sums over the workgroup, the same bits in every thread.  sm: 2 * kMaxWaves doubles.
__device__ __forceinline__ void block_sum2(double &a, double &b, double *sm, unsigned tid,
                                           unsigned nthr) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    a += __shfl_xor(a, o);
    b += __shfl_xor(b, o);
  }
  __syncthreads();  // sm may still be read from an earlier call
  if ((tid & 63u) == 0) {
    sm[2 * (tid >> 6)] = a;
    sm[2 * (tid >> 6) + 1] = b;
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
  for (unsigned w = 0; w < nthr >> 6; ++w) {
    a += sm[2 * w];
    b += sm[2 * w + 1];
  }
}

// d act / d v from the saved output: y > 0 -> 1, else 0 (relu) or 0.2 (leaky); identity: 1
__device__ __forceinline__ float act_grad(float dy, float y, int act) {
  const float neg = act == 2 ? 0.2f * dy : 0.f;
  return (act == 0 || y > 0.f) ? dy : neg;
}

struct StatOp {
  const float *__restrict__ x;
  double s, ss;
  __device__ __forceinline__ void add(float v) {
    const double d = (double)v;
    s += d;
    ss += d * d;
  }
  __device__ __forceinline__ void v4(long o) {
    const f4a v = *reinterpret_cast<const f4a *>(x + o);
    add(v.x), add(v.y), add(v.z), add(v.w);
  }
  __device__ __forceinline__ void s1(long o) { add(x[o]); }
};

struct ApplyOp {
  const float *__restrict__ x;
  const float *__restrict__ res;  // may be null
  float *__restrict__ y;
  float mean, invstd, g, b;
  int act;
  __device__ __forceinline__ float f(float v, float r) const {
    return act_f(fmaf((v - mean) * invstd, g, b) + r, act);
  }
  __device__ __forceinline__ void v4(long o) {
    const f4a v = *reinterpret_cast<const f4a *>(x + o);
    f4a r = {0.f, 0.f, 0.f, 0.f};
    if (res) r = *reinterpret_cast<const f4a *>(res + o);
    f4a out;
    out.x = f(v.x, r.x), out.y = f(v.y, r.y), out.z = f(v.z, r.z), out.w = f(v.w, r.w);
    *reinterpret_cast<f4a *>(y + o) = out;
  }
  __device__ __forceinline__ void s1(long o) { y[o] = f(x[o], res ? res[o] : 0.f); }
};

struct GradStatOp {
  const float *__restrict__ dy;
  const float *__restrict__ x;
  const float *__restrict__ y;  // null without an activation
  float mean, invstd;
  int act;
  double sg, sgx;
  __device__ __forceinline__ void add(float d, float v, float yv) {
    const float g = act_grad(d, yv, act);
    const float xh = (v - mean) * invstd;
    sg += (double)g;
    sgx += (double)g * (double)xh;
  }
  __device__ __forceinline__ void v4(long o) {
    const f4a d = *reinterpret_cast<const f4a *>(dy + o);
    const f4a v = *reinterpret_cast<const f4a *>(x + o);
    f4a yv = {1.f, 1.f, 1.f, 1.f};
    if (act) yv = *reinterpret_cast<const f4a *>(y + o);
    add(d.x, v.x, yv.x), add(d.y, v.y, yv.y), add(d.z, v.z, yv.z), add(d.w, v.w, yv.w);
  }
  __device__ __forceinline__ void s1(long o) { add(dy[o], x[o], act ? y[o] : 1.f); }
};

struct GradApplyOp {
  const float *__restrict__ dy;
  const float *__restrict__ x;
  const float *__restrict__ y;  // null without an activation
  float *__restrict__ dx;
  float *__restrict__ dres;  // may be null
  float mean, invstd, a, mg, mgx;  // a = gamma * invstd; mg = mean(g); mgx = mean(g * xhat)
  int act;
  __device__ __forceinline__ float f(float g, float v) const {
    const float xh = (v - mean) * invstd;
    return a * (g - mg - xh * mgx);
  }
  __device__ __forceinline__ void v4(long o) {
    const f4a d = *reinterpret_cast<const f4a *>(dy + o);
    const f4a v = *reinterpret_cast<const f4a *>(x + o);
    f4a yv = {1.f, 1.f, 1.f, 1.f};
    if (act) yv = *reinterpret_cast<const f4a *>(y + o);
    f4a g, out;
    g.x = act_grad(d.x, yv.x, act), g.y = act_grad(d.y, yv.y, act);
    g.z = act_grad(d.z, yv.z, act), g.w = act_grad(d.w, yv.w, act);
    out.x = f(g.x, v.x), out.y = f(g.y, v.y), out.z = f(g.z, v.z), out.w = f(g.w, v.w);
    *reinterpret_cast<f4a *>(dx + o) = out;
    if (dres) *reinterpret_cast<f4a *>(dres + o) = g;
  }
  __device__ __forceinline__ void s1(long o) {
    const float g = act_grad(dy[o], act ? y[o] : 1.f, act);
    dx[o] = f(g, x[o]);
    if (dres) dres[o] = g;
  }
};

struct Stats {
  float *save_mean, *save_invstd, *running_mean, *running_var;
  long *num_batches_tracked;
  float momentum, eps;
};

// Channel c's statistics from its sums over `count` values; the running update
// running = (1 - m) * running + m * stat (variance unbiased by count / (count - 1)); the counter
// advances once per call (channel 0).  One thread per channel calls this.
__device__ __forceinline__ void finish_channel(const Stats &st, int c, double s, double ss,
                                               double count, float &mean_f, float &invstd_f) {
  const double mean = s / count;
  double var = ss / count - mean * mean;
  var = var > 0.0 ? var : 0.0;
  mean_f = (float)mean;
  invstd_f = (float)(1.0 / sqrt(var + (double)st.eps));
  st.save_mean[c] = mean_f;
  st.save_invstd[c] = invstd_f;
  const double m = (double)st.momentum;
  st.running_mean[c] = (float)((1.0 - m) * (double)st.running_mean[c] + m * mean);
  st.running_var[c] =
      (float)((1.0 - m) * (double)st.running_var[c] + m * var * (count / (count - 1.0)));
  if (c == 0) *st.num_batches_tracked += 1;
}

// ------------------------------------------------------------------ one-launch form ---
__global__ __launch_bounds__(kOneThreads) void bn_fwd_one(
    const float *__restrict__ x, const float *__restrict__ res, float *__restrict__ y,
    const float *__restrict__ gamma, const float *__restrict__ beta, Stats st, int N, int C, int S,
    int path, int act) {
  __shared__ double sm[2 * kMaxWaves];
  __shared__ float bc[2];
  const int c = blockIdx.x;
  const unsigned tid = threadIdx.x, total = (unsigned)N * (unsigned)S;
  StatOp so{x, 0.0, 0.0};
  walk(so, path, C, c, S, 0u, total, tid, kOneThreads);
  block_sum2(so.s, so.ss, sm, tid, kOneThreads);
  if (tid == 0) finish_channel(st, c, so.s, so.ss, (double)total, bc[0], bc[1]);
  __syncthreads();
  ApplyOp ao{x, res, y, bc[0], bc[1], gamma[c], beta[c], act};
  walk(ao, path, C, c, S, 0u, total, tid, kOneThreads);
}

__global__ __launch_bounds__(kOneThreads) void bn_bwd_one(
    const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ y,
    const float *__restrict__ gamma, const float *__restrict__ save_mean,
    const float *__restrict__ save_invstd, float *__restrict__ dx, float *__restrict__ dres,
    float *__restrict__ dgamma, float *__restrict__ dbeta, int N, int C, int S, int path, int act) {
  __shared__ double sm[2 * kMaxWaves];
  const int c = blockIdx.x;
  const unsigned tid = threadIdx.x, total = (unsigned)N * (unsigned)S;
  const float mean = save_mean[c], invstd = save_invstd[c];
  GradStatOp go{dy, x, y, mean, invstd, act, 0.0, 0.0};
  walk(go, path, C, c, S, 0u, total, tid, kOneThreads);
  block_sum2(go.sg, go.sgx, sm, tid, kOneThreads);
  if (tid == 0) {
    dgamma[c] = (float)go.sgx;
    dbeta[c] = (float)go.sg;
  }
  GradApplyOp ga{dy, x, y, dx, dres, mean, invstd, gamma[c] * invstd,
                 (float)(go.sg / (double)total), (float)(go.sgx / (double)total), act};
  walk(ga, path, C, c, S, 0u, total, tid, kOneThreads);
}

// ------------------------------------------------------------------------ split form ---
// workgroup b: channel b / splits, logical range [k * split_elems, ...) with k = b % splits
struct SplitRange {
  int c;
  unsigned k, e0, e1;
};
__device__ __forceinline__ SplitRange split_range(int splits, unsigned split_elems,
                                                  unsigned total) {
  SplitRange r;
  r.c = blockIdx.x / splits;
  r.k = blockIdx.x - r.c * splits;
  r.e0 = r.k * split_elems;
  r.e1 = min(total, r.e0 + split_elems);
  return r;
}

// ws[(c * splits + k) * 2 + {0, 1}] = (sum, sum of squares) of split k of channel c
__global__ __launch_bounds__(kSplitThreads) void bn_fwd_partial(const float *__restrict__ x,
                                                               double *__restrict__ ws, int N,
                                                               int C, int S, int path, int splits,
                                                               unsigned split_elems) {
  __shared__ double sm[2 * kMaxWaves];
  const unsigned tid = threadIdx.x;
  const SplitRange r = split_range(splits, split_elems, (unsigned)N * (unsigned)S);
  StatOp so{x, 0.0, 0.0};
  walk(so, path, C, r.c, S, r.e0, r.e1, tid, kSplitThreads);
  block_sum2(so.s, so.ss, sm, tid, kSplitThreads);
  if (tid == 0) {
    ws[2l * blockIdx.x] = so.s;
    ws[2l * blockIdx.x + 1] = so.ss;
  }
}

// one thread per channel: the partials in split order -> statistics and the running update
__global__ __launch_bounds__(kSplitThreads) void bn_fwd_finish(const double *__restrict__ ws,
                                                              Stats st, int C, int splits,
                                                              double count) {
  const int c = blockIdx.x * kSplitThreads + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, ss = 0.0;
  for (int k = 0; k < splits; ++k) {
    s += ws[2l * ((long)c * splits + k)];
    ss += ws[2l * ((long)c * splits + k) + 1];
  }
  float m, i;
  finish_channel(st, c, s, ss, count, m, i);
}

__global__ __launch_bounds__(kSplitThreads) void bn_fwd_apply(
    const float *__restrict__ x, const float *__restrict__ res, float *__restrict__ y,
    const float *__restrict__ gamma, const float *__restrict__ beta,
    const float *__restrict__ mean, const float *__restrict__ invstd, int N, int C, int S,
    int path, int splits, unsigned split_elems, int act) {
  const SplitRange r = split_range(splits, split_elems, (unsigned)N * (unsigned)S);
  ApplyOp ao{x, res, y, mean[r.c], invstd[r.c], gamma[r.c], beta[r.c], act};
  walk(ao, path, C, r.c, S, r.e0, r.e1, threadIdx.x, kSplitThreads);
}

__global__ __launch_bounds__(kSplitThreads) void bn_bwd_partial(
    const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ y,
    const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
    double *__restrict__ ws, int N, int C, int S, int path, int splits, unsigned split_elems,
    int act) {
  __shared__ double sm[2 * kMaxWaves];
  const unsigned tid = threadIdx.x;
  const SplitRange r = split_range(splits, split_elems, (unsigned)N * (unsigned)S);
  GradStatOp go{dy, x, y, save_mean[r.c], save_invstd[r.c], act, 0.0, 0.0};
  walk(go, path, C, r.c, S, r.e0, r.e1, tid, kSplitThreads);
  block_sum2(go.sg, go.sgx, sm, tid, kSplitThreads);
  if (tid == 0) {
    ws[2l * blockIdx.x] = go.sg;
    ws[2l * blockIdx.x + 1] = go.sgx;
  }
}

// every workgroup re-adds its channel's partials in split order (the same bits in each); split 0
// writes dgamma / dbeta.  With ext_sums (the stage form) the sums and the count come from the
// caller and dgamma / dbeta are not written.
__global__ __launch_bounds__(kSplitThreads) void bn_bwd_apply(
    const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ y,
    const float *__restrict__ gamma, const float *__restrict__ save_mean,
    const float *__restrict__ save_invstd, const double *__restrict__ ws,
    const double *__restrict__ ext_sums, const double *__restrict__ ext_count,
    float *__restrict__ dx, float *__restrict__ dres, float *__restrict__ dgamma,
    float *__restrict__ dbeta, int N, int C, int S, int path, int splits, unsigned split_elems,
    int act) {
  const unsigned total = (unsigned)N * (unsigned)S;
  const SplitRange r = split_range(splits, split_elems, total);
  double sg = 0.0, sgx = 0.0, count = (double)total;
  if (ext_sums) {  // sums over every rank's batch [2C] and their total count
    sg = ext_sums[r.c];
    sgx = ext_sums[C + r.c];
    count = *ext_count;
  } else {
    for (int k = 0; k < splits; ++k) {
      sg += ws[2l * ((long)r.c * splits + k)];
      sgx += ws[2l * ((long)r.c * splits + k) + 1];
    }
    if (r.k == 0 && threadIdx.x == 0) {
      dgamma[r.c] = (float)sgx;
      dbeta[r.c] = (float)sg;
    }
  }
  const float mean = save_mean[r.c], invstd = save_invstd[r.c];
  GradApplyOp ga{dy, x, y, dx, dres, mean, invstd, gamma[r.c] * invstd,
                 (float)(sg / count), (float)(sgx / count), act};
  walk(ga, path, C, r.c, S, r.e0, r.e1, threadIdx.x, kSplitThreads);
}

// ---- the split form's stages on their own (SyncBatchNorm) ----
// one thread per channel: this rank's partials in split order -> row = mean [C], M2 [C], count
__global__ __launch_bounds__(kSplitThreads) void bn_moments(const double *__restrict__ ws,
                                                           double *__restrict__ row, int C,
                                                           int splits, double count) {
  const int c = blockIdx.x * kSplitThreads + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, ss = 0.0;
  for (int k = 0; k < splits; ++k) {
    s += ws[2l * ((long)c * splits + k)];
    ss += ws[2l * ((long)c * splits + k) + 1];
  }
  const double m2 = ss - s * (s / count);
  row[c] = s / count;
  row[C + c] = m2 > 0.0 ? m2 : 0.0;
  if (c == 0) row[2 * C] = count;
}

// one thread per channel: R rows of (mean, M2, count) merged in row order (Chan et al.), rows
// with count 0 skipped -> statistics of the whole batch and the running update
__global__ __launch_bounds__(kSplitThreads) void bn_finish_rows(const double *__restrict__ rows,
                                                               int R, Stats st, int C) {
  const int c = blockIdx.x * kSplitThreads + threadIdx.x;
  if (c >= C) return;
  const long stride = 2l * C + 1;
  double n = 0.0, mean = 0.0, m2 = 0.0;
  for (int r = 0; r < R; ++r) {
    const double nb = rows[r * stride + 2 * C];
    if (!(nb > 0.0)) continue;
    const double delta = rows[r * stride + c] - mean, tot = n + nb;
    mean += delta * (nb / tot);
    m2 += rows[r * stride + C + c] + delta * delta * (n * (nb / tot));
    n = tot;
  }
  const double var = n > 0.0 ? m2 / n : 0.0, m = (double)st.momentum;
  st.save_mean[c] = (float)mean;
  st.save_invstd[c] = (float)(1.0 / sqrt(var + (double)st.eps));
  // fewer than 2 values per channel over all rows have no unbiased variance (torch raises there,
  // which would take a host synchronisation here): the running statistics and the counter stay
  if (n < 2.0) return;
  st.running_mean[c] = (float)((1.0 - m) * (double)st.running_mean[c] + m * mean);
  st.running_var[c] = (float)((1.0 - m) * (double)st.running_var[c] + m * (m2 / (n - 1.0)));
  if (c == 0) *st.num_batches_tracked += 1;
}

// one thread per channel: this rank's backward partials in split order -> sums [2C] (sum g, then
// sum g * xhat) and the local dgamma / dbeta
__global__ __launch_bounds__(kSplitThreads) void bn_bwd_sums(const double *__restrict__ ws,
                                                            double *__restrict__ sums,
                                                            float *__restrict__ dgamma,
                                                            float *__restrict__ dbeta, int C,
                                                            int splits) {
  const int c = blockIdx.x * kSplitThreads + threadIdx.x;
  if (c >= C) return;
  double sg = 0.0, sgx = 0.0;
  for (int k = 0; k < splits; ++k) {
    sg += ws[2l * ((long)c * splits + k)];
    sgx += ws[2l * ((long)c * splits + k) + 1];
  }
  sums[c] = sg;
  sums[C + c] = sgx;
  dgamma[c] = (float)sgx;
  dbeta[c] = (float)sg;
}

// ------------------------------------------------------------------------------ host ---
struct Plan {
  int form, splits, split_elems;
};

// AANET_OK and the plan, or the status the launch returns for these sizes
int make_plan(int n, int c, int s, int algo, int split_elems, Plan *p, long min_total = 2) {
  if (n <= 0 || c <= 0 || s <= 0 || split_elems < 0) return AANET_EINVAL;
  if (algo != AANET_BN_AUTO && algo != AANET_BN_ONE_LAUNCH && algo != AANET_BN_SPLIT)
    return AANET_EINVAL;
  const long total = (long)n * s;
  if (total < min_total) return AANET_EINVAL;  // one value per channel: no variance to train on
  // the logical index of a channel is 32-bit (with room for one stride past its end)
  if (total > 0x7fffffffl - 4l * kOneThreads) return AANET_EUNSUPPORTED;
  int form = algo;
  if (algo == AANET_BN_AUTO)
    form = total <= AANET_BN_ONE_LAUNCH_MAX ? AANET_BN_ONE_LAUNCH : AANET_BN_SPLIT;
  p->form = form;
  if (form == AANET_BN_ONE_LAUNCH) {
    p->splits = 1;
    p->split_elems = (int)total;
    return AANET_OK;
  }
  long se = split_elems;
  if (se == 0) {
    // about 2048 workgroups in all, none below 8192 values
    const long want = (2048 + c - 1) / c;
    se = (total + want - 1) / want;
    if (se < 8192) se = 8192;
  }
  se = (se + 3) / 4 * 4;  // quads never straddle two splits
  const long splits = (total + se - 1) / se;
  if (splits > kMaxSplits) return AANET_EINVAL;
  if (splits * c > 0x7fffffffl) return AANET_EUNSUPPORTED;
  p->splits = (int)splits;
  p->split_elems = (int)se;
  return AANET_OK;
}

bool aligned16(const void *p) { return p == nullptr || ((uintptr_t)p & 15u) == 0; }

int choose_path(int s, bool aligned) {
  if (!aligned) return PATH_SCALAR;
  if (s >= kSegMin) return PATH_SEG;
  return s % 4 == 0 ? PATH_VEC : PATH_SCALAR;
}

}  // namespace

extern "C" {

int aanet_bn_act_plan(int n, int c, int s, int algo, int split_elems, int *form, int *splits,
                      int *elems_per_split) {
  AANET_HOST_CHECK(form && splits && elems_per_split);
  Plan p;
  const int rc = make_plan(n, c, s, algo, split_elems, &p);
  if (rc != AANET_OK) return rc;
  *form = p.form;
  *splits = p.splits;
  *elems_per_split = p.split_elems;
  return AANET_OK;
}

size_t aanet_bn_act_workspace_size(int n, int c, int s, int algo, int split_elems) {
  Plan p;
  // (a single value per channel is a stage call's business: aanet_bn_act_stats_f32)
  if (make_plan(n, c, s, algo, split_elems, &p, 1) != AANET_OK || p.form != AANET_BN_SPLIT)
    return 0;
  return (size_t)c * p.splits * 2 * sizeof(double);
}

int aanet_bn_act_train_f32(const float *x, const float *residual, const float *weight,
                           const float *bias, float *running_mean, float *running_var,
                           long *num_batches_tracked, float momentum, float eps, int act,
                           float *y, float *save_mean, float *save_invstd, int n, int c, int s,
                           int algo, int split_elems, void *workspace, size_t workspace_bytes,
                           aanet_stream_t stream) {
  AANET_HOST_CHECK(x && weight && bias && running_mean && running_var && num_batches_tracked &&
                   y && save_mean && save_invstd);
  AANET_HOST_CHECK(act >= 0 && act <= 2 && eps >= 0.f);
  Plan p;
  const int rc = make_plan(n, c, s, algo, split_elems, &p);
  if (rc != AANET_OK) return rc;
  const int path = choose_path(s, aligned16(x) && aligned16(residual) && aligned16(y));
  const Stats st{save_mean, save_invstd, running_mean, running_var, num_batches_tracked,
                 momentum, eps};
  if (p.form == AANET_BN_ONE_LAUNCH) {
    bn_fwd_one<<<c, kOneThreads, 0, as_hip(stream)>>>(x, residual, y, weight, bias, st, n, c, s,
                                                      path, act);
    return aanet_launch_status();
  }
  AANET_HOST_CHECK(workspace && workspace_bytes >= (size_t)c * p.splits * 2 * sizeof(double));
  double *ws = static_cast<double *>(workspace);
  const int grid = c * p.splits;
  bn_fwd_partial<<<grid, kSplitThreads, 0, as_hip(stream)>>>(x, ws, n, c, s, path, p.splits,
                                                            (unsigned)p.split_elems);
  bn_fwd_finish<<<host_div_up(c, kSplitThreads), kSplitThreads, 0, as_hip(stream)>>>(
      ws, st, c, p.splits, (double)n * (double)s);
  bn_fwd_apply<<<grid, kSplitThreads, 0, as_hip(stream)>>>(x, residual, y, weight, bias,
                                                          save_mean, save_invstd, n, c, s, path,
                                                          p.splits, (unsigned)p.split_elems, act);
  return aanet_launch_status();
}

int aanet_bn_act_train_bwd_f32(const float *grad_out, const float *x, const float *y,
                               const float *weight, const float *save_mean,
                               const float *save_invstd, int act, float *grad_x,
                               float *grad_residual, float *grad_weight, float *grad_bias, int n,
                               int c, int s, int algo, int split_elems, void *workspace,
                               size_t workspace_bytes, aanet_stream_t stream) {
  AANET_HOST_CHECK(grad_out && x && weight && save_mean && save_invstd && grad_x && grad_weight &&
                   grad_bias);
  AANET_HOST_CHECK(act >= 0 && act <= 2 && (act == 0 || y));
  Plan p;
  const int rc = make_plan(n, c, s, algo, split_elems, &p);
  if (rc != AANET_OK) return rc;
  if (act == 0) y = nullptr;
  const int path = choose_path(s, aligned16(grad_out) && aligned16(x) && aligned16(y) &&
                                      aligned16(grad_x) && aligned16(grad_residual));
  if (p.form == AANET_BN_ONE_LAUNCH) {
    bn_bwd_one<<<c, kOneThreads, 0, as_hip(stream)>>>(grad_out, x, y, weight, save_mean,
                                                      save_invstd, grad_x, grad_residual,
                                                      grad_weight, grad_bias, n, c, s, path, act);
    return aanet_launch_status();
  }
  AANET_HOST_CHECK(workspace && workspace_bytes >= (size_t)c * p.splits * 2 * sizeof(double));
  double *ws = static_cast<double *>(workspace);
  const int grid = c * p.splits;
  bn_bwd_partial<<<grid, kSplitThreads, 0, as_hip(stream)>>>(grad_out, x, y, save_mean,
                                                            save_invstd, ws, n, c, s, path,
                                                            p.splits, (unsigned)p.split_elems, act);
  bn_bwd_apply<<<grid, kSplitThreads, 0, as_hip(stream)>>>(
      grad_out, x, y, weight, save_mean, save_invstd, ws, nullptr, nullptr, grad_x, grad_residual,
      grad_weight, grad_bias, n, c, s, path, p.splits, (unsigned)p.split_elems, act);
  return aanet_launch_status();
}

// ---- stages (always the split form; one rank may hold a single value per channel) ----
int aanet_bn_act_stats_f32(const float *x, int n, int c, int s, int split_elems, double *row,
                           void *workspace, size_t workspace_bytes, aanet_stream_t stream) {
  AANET_HOST_CHECK(x && row);
  Plan p;
  const int rc = make_plan(n, c, s, AANET_BN_SPLIT, split_elems, &p, 1);
  if (rc != AANET_OK) return rc;
  AANET_HOST_CHECK(workspace && workspace_bytes >= (size_t)c * p.splits * 2 * sizeof(double));
  double *ws = static_cast<double *>(workspace);
  bn_fwd_partial<<<c * p.splits, kSplitThreads, 0, as_hip(stream)>>>(
      x, ws, n, c, s, choose_path(s, aligned16(x)), p.splits, (unsigned)p.split_elems);
  bn_moments<<<host_div_up(c, kSplitThreads), kSplitThreads, 0, as_hip(stream)>>>(
      ws, row, c, p.splits, (double)n * (double)s);
  return aanet_launch_status();
}

int aanet_bn_act_finish_f32(const double *rows, int num_rows, int c, float momentum, float eps,
                            float *running_mean, float *running_var, long *num_batches_tracked,
                            float *save_mean, float *save_invstd, aanet_stream_t stream) {
  AANET_HOST_CHECK(rows && running_mean && running_var && num_batches_tracked && save_mean &&
                   save_invstd);
  AANET_HOST_CHECK(num_rows > 0 && c > 0 && eps >= 0.f);
  const Stats st{save_mean, save_invstd, running_mean, running_var, num_batches_tracked,
                 momentum, eps};
  bn_finish_rows<<<host_div_up(c, kSplitThreads), kSplitThreads, 0, as_hip(stream)>>>(
      rows, num_rows, st, c);
  return aanet_launch_status();
}

int aanet_bn_act_apply_f32(const float *x, const float *residual, const float *weight,
                           const float *bias, const float *mean, const float *invstd, int act,
                           float *y, int n, int c, int s, int split_elems,
                           aanet_stream_t stream) {
  AANET_HOST_CHECK(x && weight && bias && mean && invstd && y && act >= 0 && act <= 2);
  Plan p;
  const int rc = make_plan(n, c, s, AANET_BN_SPLIT, split_elems, &p, 1);
  if (rc != AANET_OK) return rc;
  bn_fwd_apply<<<c * p.splits, kSplitThreads, 0, as_hip(stream)>>>(
      x, residual, y, weight, bias, mean, invstd, n, c, s,
      choose_path(s, aligned16(x) && aligned16(residual) && aligned16(y)), p.splits,
      (unsigned)p.split_elems, act);
  return aanet_launch_status();
}

int aanet_bn_act_bwd_reduce_f32(const float *grad_out, const float *x, const float *y,
                                const float *mean, const float *invstd, int act, double *sums,
                                float *grad_weight, float *grad_bias, int n, int c, int s,
                                int split_elems, void *workspace, size_t workspace_bytes,
                                aanet_stream_t stream) {
  AANET_HOST_CHECK(grad_out && x && mean && invstd && sums && grad_weight && grad_bias);
  AANET_HOST_CHECK(act >= 0 && act <= 2 && (act == 0 || y));
  Plan p;
  const int rc = make_plan(n, c, s, AANET_BN_SPLIT, split_elems, &p, 1);
  if (rc != AANET_OK) return rc;
  AANET_HOST_CHECK(workspace && workspace_bytes >= (size_t)c * p.splits * 2 * sizeof(double));
  if (act == 0) y = nullptr;
  double *ws = static_cast<double *>(workspace);
  bn_bwd_partial<<<c * p.splits, kSplitThreads, 0, as_hip(stream)>>>(
      grad_out, x, y, mean, invstd, ws, n, c, s,
      choose_path(s, aligned16(grad_out) && aligned16(x) && aligned16(y)), p.splits,
      (unsigned)p.split_elems, act);
  bn_bwd_sums<<<host_div_up(c, kSplitThreads), kSplitThreads, 0, as_hip(stream)>>>(
      ws, sums, grad_weight, grad_bias, c, p.splits);
  return aanet_launch_status();
}

int aanet_bn_act_bwd_apply_f32(const float *grad_out, const float *x, const float *y,
                               const float *weight, const float *mean, const float *invstd,
                               const double *sums, const double *total_count, int act,
                               float *grad_x, float *grad_residual, int n, int c, int s,
                               int split_elems, aanet_stream_t stream) {
  AANET_HOST_CHECK(grad_out && x && weight && mean && invstd && sums && total_count && grad_x);
  AANET_HOST_CHECK(act >= 0 && act <= 2 && (act == 0 || y));
  Plan p;
  const int rc = make_plan(n, c, s, AANET_BN_SPLIT, split_elems, &p, 1);
  if (rc != AANET_OK) return rc;
  if (act == 0) y = nullptr;
  bn_bwd_apply<<<c * p.splits, kSplitThreads, 0, as_hip(stream)>>>(
      grad_out, x, y, weight, mean, invstd, nullptr, sums, total_count, grad_x, grad_residual,
      nullptr, nullptr, n, c, s,
      choose_path(s, aligned16(grad_out) && aligned16(x) && aligned16(y) && aligned16(grad_x) &&
                         aligned16(grad_residual)),
      p.splits, (unsigned)p.split_elems, act);
  return aanet_launch_status();
}

}  // extern "C"
