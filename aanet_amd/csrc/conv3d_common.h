// conv3d_common.h -- what the 3x3x3 depth-marching kernels share (conv3d.hip: stride 1;
// conv3d_s2.hip: stride 2; deconv3d.hip: transposed, stride 2): the swizzled LDS halo slot, the
// args struct, the host side of their entry points and the pre-split weight pack with its
// kernel; conv3d_head.hip uses the host checks.
//
// Addressing.  One buffer resource per image for x, out and the residual (64-bit base per n,
// 32-bit byte offsets inside the image's volume), so C3_OOB is an offset the range check
// refuses: a load there returns zeros, a store is dropped.  c3_volumes_ok is the matching host
// check: the entry points refuse volumes of 2^31 bytes per image.
//
// Host.  c3_conv_args_ok screens a support query's arguments, c3_supported is the query of the
// three kernels, c3_volumes_ok / c3_tiles are the addressing and grid limits, and c3_launch is
// the whole entry point of a kernel.
//
// The kernels' staging, march and epilogue stay written out in each file.  Sharing them (a halo
// helper, a tile / epilogue struct, the march as a template over callables) gave bit-identical
// results but different register allocation and scheduling, and the full-resolution 32-channel
// shapes timed 0.7-1.8 % slower than before (CHANGELOG.md); equal device code was the bar.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"
#include "split.h"

namespace {

constexpr unsigned C3_OOB = 0x80000000u;  // a buffer offset the range check refuses (volumes < 2^31 B)
constexpr int C3_NT = 256;                // threads of a workgroup: 4 waves

// bf16 offset of 16-byte slot q8 (channels 8 q8 .. 8 q8 + 7) of halo position pos (conv_g3.hip)
__device__ __forceinline__ int c3_swz(int pos, int q8) {
  return pos * 32 + ((q8 ^ (((pos >> 2) & 1) << 1)) << 3);
}

struct C3Args {
  const float *x;        // [N][D][H][W][C]
  const bf16x8 *wsplit;  // [Co/32][C/32][9 (kh,kw)][3 kd][2 co blocks][3 pieces][64 lanes] x 16 B
  const float *bias;     // [Co] or NULL
  const float *res;      // [N][Do][Ho][Wo][Co] or NULL
  float *out;            // [N][Do][Ho][Wo][Co]
  int N, C, D, H, W, Co, act;
};

// ---- host side
inline bool c3_channels(int c) { return c == 32 || c == 64 || c == 96 || c == 128; }

// the arguments of a support query: sizes positive, paddings not negative
inline bool c3_conv_args_ok(int c, int co, int kd, int kh, int kw, int stride, int pad, int out_pad,
                            int dil, int groups) {
  return c > 0 && co > 0 && kd > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0 && out_pad >= 0 &&
         dil > 0 && groups > 0;
}

// the support query of the three kernels: 3x3x3, padding 1, dilation 1, one group, the channel
// table, and this kernel's stride and output padding (0 for a Conv3d)
inline int c3_supported(int want_stride, int want_out_pad, int c, int co, int kd, int kh, int kw,
                        int stride, int pad, int out_pad, int dil, int groups) {
  if (!c3_conv_args_ok(c, co, kd, kh, kw, stride, pad, out_pad, dil, groups)) return AANET_EINVAL;
  const bool ok = kd == 3 && kh == 3 && kw == 3 && stride == want_stride && pad == 1 &&
                  out_pad == want_out_pad && dil == 1 && groups == 1 && c3_channels(c) &&
                  c3_channels(co);
  return ok ? AANET_OK : AANET_EUNSUPPORTED;
}

// per-image buffer resources with 32-bit offsets: both volumes (elements of one image) < 2^31 bytes
inline bool c3_volumes_ok(long in_img, long out_img) {
  return in_img * 4 < (1L << 31) && out_img * 4 < (1L << 31);
}

// workgroups of grid.x for n images of th x tw cut into tr x tc tiles, or 0 past the grid limit
inline unsigned c3_tiles(long th, long tw, int tr, int tc, int n) {
  const long tiles = (long)host_div_up(tw, tc) * host_div_up(th, tr) * n;
  return tiles > 0x7fffffffL ? 0u : (unsigned)tiles;
}

struct C3Tiling {
  int tr, tc;   // tile (rows x columns)
  long th, tw;  // the extent cut into tiles: the output's, for the transposed conv the input's
};
struct C3Extent {
  long d, h, w;  // one image's output
};

// The entry point of a depth-marching kernel: validate, check both volumes and the tile count,
// fill the args, launch.
template <class Kernel>
inline int c3_launch(Kernel kernel, C3Tiling t, C3Extent o, const float *x, const void *wsplit,
                     const float *bias, const float *residual, int act, float *out, int n, int c,
                     int d, int h, int w, int co, aanet_stream_t stream) {
  if (!x || !wsplit || !out || n <= 0 || c <= 0 || d <= 0 || h <= 0 || w <= 0 || co <= 0 ||
      act < 0 || act > 2)
    return AANET_EINVAL;
  if (!c3_channels(c) || !c3_channels(co)) return AANET_EINVAL;
  if (!c3_volumes_ok((long)d * h * w * c, o.d * o.h * o.w * co)) return AANET_EUNSUPPORTED;
  const unsigned tiles = c3_tiles(t.th, t.tw, t.tr, t.tc, n);
  if (!tiles) return AANET_EUNSUPPORTED;
  C3Args a;
  a.x = x;
  a.wsplit = reinterpret_cast<const bf16x8 *>(wsplit);
  a.bias = bias;
  a.res = residual;
  a.out = out;
  a.N = n, a.C = c, a.D = d, a.H = h, a.W = w, a.Co = co, a.act = act;
  hipLaunchKernelGGL(kernel, dim3(tiles, co / 32), dim3(C3_NT), 0, as_hip(stream), a);
  return aanet_launch_status();
}

// ---- the pre-split weight pack
inline size_t c3_pack_bytes(int co, int c) {
  if (!c3_channels(co) || !c3_channels(c)) return 0;
  return (size_t)(co / 32) * (c / 32) * 27 * 2 * 3 * 1024;
}

// w fp32 -> [Co/32][C/32][9 (kh,kw)][3 kd][2][3 pieces][64 lanes][8 bf16]: lane l of co block m
// holds row 32cb + 16m + l%16, channels 32cc + 8(l/16) + 0..7, as three bf16 pieces (round to
// nearest: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)).  w is [Co][C][3][3][3] (Conv3d),
// or with TRANSPOSED [C][Co][3][3][3] (ConvTranspose3d).
template <bool TRANSPOSED>
__global__ void conv3d_pack_kernel(const float *__restrict__ w, bf16x8 *__restrict__ out, int Co, int C) {
  const int ncc = C / 32, total = (Co / 32) * ncc * 27 * 2 * 64;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int l = e & 63, m = (e >> 6) & 1;
    int r = e >> 7;
    const int kd = r % 3;
    r /= 3;
    const int k = r % 9;
    r /= 9;
    const int cc = r % ncc, cb = r / ncc;
    const int co = 32 * cb + 16 * m + (l & 15), c0 = 32 * cc + 8 * (l >> 4);
    bf16x8 ph, pm, pl;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long row = TRANSPOSED ? (long)(c0 + u) * Co + co : (long)co * C + c0 + u;
      const float v = w[row * 27 + kd * 9 + k];
      const __bf16 h = (__bf16)v;
      const float r1 = v - (float)h;
      const __bf16 mm = (__bf16)r1;
      ph[u] = h;
      pm[u] = mm;
      pl[u] = (__bf16)(r1 - (float)mm);
    }
    const long o = (long)(e >> 6) * 3 * 64 + l;
    out[o] = ph;
    out[o + 64] = pm;
    out[o + 128] = pl;
  }
}

template <bool TRANSPOSED>
inline int c3_pack(const float *w, int co, int c, void *wsplit, aanet_stream_t stream) {
  if (!w || !wsplit || !c3_pack_bytes(co, c)) return AANET_EINVAL;
  const int total = (co / 32) * (c / 32) * 27 * 2 * 64;
  hipLaunchKernelGGL(conv3d_pack_kernel<TRANSPOSED>, dim3(host_div_up(total, 256)), dim3(256), 0,
                     as_hip(stream), w, reinterpret_cast<bf16x8 *>(wsplit), co, c);
  return aanet_launch_status();
}

}  // namespace
