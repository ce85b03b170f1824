// conv3d_common.h -- what the 3x3x3 depth-marching kernels share (conv3d.hip: stride 1;
// conv3d_s2.hip: stride 2; deconv3d.hip: transposed, stride 2): the swizzled LDS halo slot, the
// channel table and the pre-split weight pack with its kernel.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"
#include "split.h"

namespace {

constexpr unsigned C3_OOB = 0x80000000u;  // a buffer offset the range check refuses (volumes < 2^31 B)

// bf16 offset of 16-byte slot q8 (channels 8 q8 .. 8 q8 + 7) of halo position pos (conv_g3.hip)
__device__ __forceinline__ int c3_swz(int pos, int q8) {
  return pos * 32 + ((q8 ^ (((pos >> 2) & 1) << 1)) << 3);
}

inline bool c3_channels(int c) { return c == 32 || c == 64 || c == 96 || c == 128; }

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
