// deconv3d.hip -- the 3-D aggregators' up-sampling convs in eval (nets/aggregation.py:
// ConvTranspose3d 3x3x3, stride 2, padding 1, output padding 1, one group, BN folded by the
// caller) for gfx950:
//   out = act(conv_transpose3d(x, W, stride 2, padding 1, output_padding 1) + bias [+ residual]),
//   x [n][d][h][w][c], residual / out [n][2d][2h][2w][co] channels-last, W [c][co][3][3][3].
//
// Phase form: no im2col, no col2im, no atomics.  Output index o = 2i - 1 + k, so along each axis
// an even output 2a takes k = 1 from input a, and an odd output 2a + 1 takes k = 2 from input a
// and k = 0 from input a + 1.  Input position (a, b) of a plane therefore owns the four outputs
// (2a + ph, 2b + pw), fed by the inputs (a + dy, b + dx), dy, dx in {0, 1}: the in-plane phases
// (ph, pw) have 1, 2, 2 and 4 taps, and with the depth phases 1, 2, 2, 2, 4, 4, 4 and 8 -- the
// 27 taps, each used by exactly one phase, every output written once by its one owner.
//
// Depth marching.  A workgroup (4 waves) owns a 4 x 16 (h x w) INPUT tile (an 8 x 32 output tile
// per plane) of one image and one block of 32 output channels (grid.y), and walks the input
// planes d = 0 .. D-1.  For every plane and 32-channel chunk the tile's 5 x 17 halo (+1 on the
// high side) is loaded once, split into its three bf16 pieces once and stored in LDS (16 KB, the
// swizzled rows of conv3d.hip: unit-stride, conflict-free ds_read_b128).  The staged plane feeds
// three accumulator sets: kd = 0 completes output plane 2d - 1 (started by plane d - 1's kd = 2),
// kd = 1 is plane 2d whole, kd = 2 starts plane 2d + 1.  Planes 2d - 1 and 2d are stored once the
// last chunk of input plane d is consumed; plane 2D - 1 has no d + 1 neighbour.
//
// Wave w owns input rows 2(w & 1), 2(w & 1) + 1 and the 16 output channels of half m = w >> 1:
// 2 rows x 4 in-plane phases x 4 VGPRs = 32 accumulator VGPRs per output plane, 96 in all.  Lane
// (kr = lane / 16, jj = lane % 16) = input column jj, channels 8kr .. 8kr + 7 of the B fragment.
//
// Addressing: one buffer resource per image, 32-bit byte offsets inside it; the entry point
// refuses volumes of 2^31 bytes per image.
//
// Numerics: the split-bf16 contraction of split.h (six piece products, fp32 accumulation); per
// output the order is input plane, chunk, (dy, dx) ascending -- independent of the batch.
#include "conv3d_common.h"

namespace {

constexpr int NT = C3_NT;                   // 4 waves: two input rows x one 16-channel half each
constexpr int TR = 4, TC = 16;              // input tile (h x w)
constexpr int HR = TR + 1, HWW = TC + 1;    // halo 5 x 17
constexpr int NPOS = HR * HWW;              // 85 positions
constexpr int PE = NPOS * 32;               // bf16 per piece plane
constexpr int HIT = (NPOS * 4 + NT - 1) / NT;  // halo octets (8 channels of a position) per thread
constexpr unsigned OOB = C3_OOB;

__global__ __launch_bounds__(NT, 2) void deconv3d2x_kernel(C3Args a) {
  __shared__ __attribute__((aligned(16))) __bf16 sH[3 * PE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rp = wave & 1, m = wave >> 1;
  const int kr = lane >> 4, jj = lane & 15;
  const int C = a.C, D = a.D, H = a.H, W = a.W, Co = a.Co;
  const int Ho = 2 * H, Wo = 2 * W;
  const int tx = (W + TC - 1) / TC, ntiles = tx * ((H + TR - 1) / TR);
  const int n = blockIdx.x / ntiles, tile = blockIdx.x % ntiles, cb = blockIdx.y;
  const int y0 = (tile / tx) * TR, x0 = (tile % tx) * TC;  // input coordinates
  const int ncc = C / 32;
  const long in_img = (long)D * H * W * C, out_img = 8L * D * H * W * Co;  // elements, < 2^29
  const brsrc_t xr = buf_rsrc(a.x + n * in_img, in_img * 4);
  const brsrc_t orr = buf_rsrc(a.out + n * out_img, out_img * 4);
  const unsigned in_plane = (unsigned)(H * W * C) * 4u;  // bytes

  // halo item i of this thread: position e >> 2, channel octet e & 3; its byte offset inside a
  // plane's chunk 0, or OOB outside the image (zeros: inputs past the high side feed nothing)
  unsigned hoff[HIT];
#pragma unroll
  for (int i = 0; i < HIT; ++i) {
    const int e = tid + NT * i, pos = e >> 2;
    const int yy = y0 + pos / HWW, xx = x0 + pos % HWW;
    const bool ok = pos < NPOS && yy < H && xx < W;
    hoff[i] = ok ? (unsigned)(((yy * W + xx) * C + 8 * (e & 3)) * 4) : OOB;
  }
  f32x4 hv[HIT][2];
  auto load_halo = [&](int d, int cc) {
    const unsigned uni = (unsigned)d * in_plane + 128u * (unsigned)cc;  // < 2^31: OOB stays out of range
#pragma unroll
    for (int i = 0; i < HIT; ++i) {
      hv[i][0] = buf_ld4(xr, hoff[i] + uni);
      hv[i][1] = buf_ld4(xr, hoff[i] + uni + 16u);
    }
  };
  auto store_halo = [&]() {
#pragma unroll
    for (int i = 0; i < HIT; ++i) {
      const int e = tid + NT * i, pos = e >> 2;
      if (pos < NPOS) {
        const float v[8] = {hv[i][0][0], hv[i][0][1], hv[i][0][2], hv[i][0][3],
                            hv[i][1][0], hv[i][1][1], hv[i][1][2], hv[i][1][3]};
        bf16x8 b[3];
        split8(v, b);
        const int o = c3_swz(pos, e & 3);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<bf16x8 *>(sH + pc * PE + o) = b[pc];
      }
    }
  };

  // acc[s][r][p]: output plane 2 d_in - 1 + s, input row 2rp + r, in-plane phase p = 2 ph + pw
  // (output pixel (2 row + ph, 2 column + pw)), channels 32cb + 16m + 4kr + 0..3
  f32x4 acc[3][2][4];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int p = 0; p < 4; ++p) acc[s][r][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (a.bias) {
#pragma unroll
    for (int u = 0; u < 4; ++u) bv[u] = a.bias[32 * cb + 16 * m + 4 * kr + u];
  }
  const float *resp = a.res ? a.res + n * out_img : a.out + n * out_img;  // a valid base either way
  const brsrc_t rr = buf_rsrc(resp, out_img * 4);
  const bool has_res = a.res != nullptr;
  const int act = a.act;
  auto store_plane = [&](int dz, const f32x4 (&ac)[2][4]) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int y = y0 + 2 * rp + r, x = x0 + jj;
      const bool ok = y < H && x < W;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int oy = 2 * y + (p >> 1), ox = 2 * x + (p & 1);
        const unsigned off =
            ok ? (unsigned)(((dz * Ho + oy) * Wo + ox) * Co + 32 * cb + 16 * m + 4 * kr) * 4u : OOB;
        f32x4 v = ac[r][p] + bv;
        if (has_res) v += buf_ld4(rr, off);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = act_f(v[u], act);
        buf_st4(orr, off, v);
      }
    }
  };

  load_halo(0, 0);
  for (int d = 0; d < D; ++d) {
    for (int cc = 0; cc < ncc; ++cc) {
      __syncthreads();  // every wave is done reading the previous halo
      store_halo();
      __syncthreads();
      if (cc + 1 < ncc)
        load_halo(d, cc + 1);
      else if (d + 1 < D)
        load_halo(d + 1, 0);
      const bf16x8 *wb = a.wsplit + ((long)(cb * ncc + cc) * (27 * 6)) * 64 + lane;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          bf16x8 B[2][3];
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const __bf16 *bp = sH + c3_swz((2 * rp + r + dy) * HWW + jj + dx, kr);
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) B[r][pc] = *reinterpret_cast<const bf16x8 *>(bp + pc * PE);
          }
          // input (a + dy, b + dx) reaches output (2a + ph, 2b + pw) through kh = ph + 1 - 2 dy:
          // dy = 0 gives kh = 1 (ph 0) and kh = 2 (ph 1), dy = 1 gives kh = 0 (ph 1); kw likewise
#pragma unroll
          for (int ph = dy; ph < 2; ++ph)
#pragma unroll
            for (int pw = dx; pw < 2; ++pw) {
              const int k = (ph + 1 - 2 * dy) * 3 + (pw + 1 - 2 * dx);
#pragma unroll
              for (int kd = 0; kd < 3; ++kd) {
                bf16x8 A[3];
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) A[pc] = wb[(((k * 3 + kd) * 2 + m) * 3 + pc) * 64];
#pragma unroll
                for (int r = 0; r < 2; ++r)
                  acc[kd][r][2 * ph + pw] = mfma_split6(A, B[r], acc[kd][r][2 * ph + pw]);
              }
            }
        }
    }
    if (d >= 1) store_plane(2 * d - 1, acc[0]);
    store_plane(2 * d, acc[1]);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        acc[0][r][p] = acc[2][r][p];
        acc[1][r][p] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[2][r][p] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  }
  store_plane(2 * D - 1, acc[0]);
}

}  // namespace

extern "C" {

int aanet_deconv3d2x_supported(int c, int co, int kd, int kh, int kw, int stride, int pad,
                               int out_pad, int dil, int groups) {
  return c3_supported(2, 1, c, co, kd, kh, kw, stride, pad, out_pad, dil, groups);
}

size_t aanet_deconv3d2x_pack_bytes(int co, int c) { return c3_pack_bytes(co, c); }

int aanet_deconv3d2x_pack_f32(const float *w, int co, int c, void *wsplit, aanet_stream_t stream) {
  return c3_pack<true>(w, co, c, wsplit, stream);
}

int aanet_deconv3d2x_fused_f32(const float *x, const void *wsplit, const float *bias,
                               const float *residual, int act, float *out, int n, int c, int d,
                               int h, int w, int co, aanet_stream_t stream) {
  return c3_launch(deconv3d2x_kernel, C3Tiling{TR, TC, h, w}, C3Extent{2L * d, 2L * h, 2L * w}, x,
                   wsplit, bias, residual, act, out, n, c, d, h, w, co, stream);
}

}  // extern "C"
