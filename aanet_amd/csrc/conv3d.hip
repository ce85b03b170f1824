// conv3d.hip -- the 3-D aggregators' eval convs (nets/aggregation.py:8-21, 52-67: Conv3d 3x3x3,
// stride 1, padding 1, dilation 1, one group, BN folded by the caller) for gfx950:
//   out = act(conv3d(x, W) + bias [+ residual]),  x / residual / out channels-last [n][d][h][w][c].
//
// Depth marching.  A workgroup (4 waves) owns an 8 x 16 (h x w) output tile of one image and one
// block of 32 output channels (grid.y), and walks the input planes d_in = 0 .. D-1.  For every
// plane and 32-channel chunk the tile's 10 x 18 halo is loaded once, split into its three bf16
// pieces once and stored in LDS (34.5 KB, the XOR-swizzled 64-byte rows of the 2-D halo forms:
// conflict-free ds_read_b128 for any tap shift); the next plane's loads are in flight in registers
// while this one is contracted.  The staged plane feeds all 27 taps: the B fragment of in-plane
// tap (ti, tj) serves kd = 2, 1, 0, i.e. the output planes d_in-1, d_in, d_in+1, which are three
// rolling accumulator sets; plane d_in-1 is complete, and stored, once plane d_in is consumed.
// Depth padding is planes that are never staged; h / w padding is the zero a buffer load returns
// past its range.  Every input element is staged and split once per workgroup and output-channel
// block (1.4x for the halo), against 3x for a 2-D tiling with kd outside and 27x for an im2col.
//
// Wave w owns tile rows w and w + 4: lane (kr = lane / 16, jj = lane % 16) = column jj, channels
// 8kr..8kr+7 of the B fragment.  An A fragment (pre-split weights, streamed from L2 / L1 -- the
// four waves read the same lines) feeds both rows, so a step of 27 taps is 162 16-byte A loads,
// 54 ds_read_b128 and 648 MFMAs per wave.
//
// Addressing: one buffer resource per image (64-bit base per n), 32-bit byte offsets inside the
// image's volume; the entry point refuses volumes of 2^31 bytes per image.
//
// Numerics: the split-bf16 contraction of split.h (six piece products, fp32 accumulation); per
// output the order is input plane, chunk, in-plane tap ascending -- independent of the batch.
#include <hip/hip_runtime.h>

#include "conv3d_common.h"

namespace {

constexpr int NT = C3_NT;                   // 4 waves, two tile rows each
constexpr int TR = 8, TC = 16;              // output tile (h x w)
constexpr int HWW = TC + 2, HR = TR + 2;    // halo
constexpr int NPOS = HR * HWW;              // 180 positions
constexpr int PE = NPOS * 32;               // bf16 per piece plane
constexpr int HIT = (NPOS * 4 + NT - 1) / NT;  // halo octets (8 channels of a position) per thread
constexpr unsigned OOB = C3_OOB;

__global__ __launch_bounds__(NT, 2) void conv3d_kernel(C3Args a) {
  __shared__ __attribute__((aligned(16))) __bf16 sH[3 * PE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kr = lane >> 4, jj = lane & 15;
  const int C = a.C, D = a.D, H = a.H, W = a.W, Co = a.Co;
  const int tx = (W + TC - 1) / TC, ntiles = tx * ((H + TR - 1) / TR);
  const int n = blockIdx.x / ntiles, tile = blockIdx.x % ntiles, cb = blockIdx.y;
  const int y0 = (tile / tx) * TR, x0 = (tile % tx) * TC;
  const int ncc = C / 32;
  const long in_img = (long)D * H * W * C, out_img = (long)D * H * W * Co;  // elements, < 2^29
  const brsrc_t xr = buf_rsrc(a.x + n * in_img, in_img * 4);
  const brsrc_t orr = buf_rsrc(a.out + n * out_img, out_img * 4);
  const unsigned in_plane = (unsigned)(H * W * C) * 4u;  // bytes

  // halo item i of this thread: position e >> 2, channel octet e & 3; its byte offset inside a
  // plane's chunk 0, or OOB outside the image (the range check then returns zeros: the padding)
  unsigned hoff[HIT];
#pragma unroll
  for (int i = 0; i < HIT; ++i) {
    const int e = tid + NT * i, pos = e >> 2;
    const int yy = y0 - 1 + pos / HWW, xx = x0 - 1 + pos % HWW;
    const bool ok = pos < NPOS && yy >= 0 && yy < H && xx >= 0 && xx < W;
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

  // acc[s][r][m]: output plane d_in - 1 + s, tile row wave + 4r, channels 32cb + 16m + 4kr + 0..3
  f32x4 acc[3][2][2];
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int m = 0; m < 2; ++m) acc[s][r][m] = f32x4{0.f, 0.f, 0.f, 0.f};

  // epilogue of one finished plane: bias, residual, activation, NDHWC channel-quad stores; pixels
  // past the image get an offset the range check drops
  f32x4 bv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (a.bias) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int u = 0; u < 4; ++u) bv[m][u] = a.bias[32 * cb + 16 * m + 4 * kr + u];
  }
  const float *resp = a.res ? a.res + n * out_img : a.out + n * out_img;  // a valid base either way
  const brsrc_t rr = buf_rsrc(resp, out_img * 4);
  const bool has_res = a.res != nullptr;
  const int act = a.act;
  auto store_plane = [&](int dz, const f32x4 (&ac)[2][2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int y = y0 + wave + 4 * r, x = x0 + jj;
      const bool ok = y < H && x < W;
      const unsigned pix = (unsigned)(((dz * H + y) * W + x) * Co + 32 * cb + 4 * kr) * 4u;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const unsigned off = ok ? pix + 64u * m : OOB;
        f32x4 v = ac[r][m] + bv[m];
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
      for (int k = 0; k < 9; ++k) {
        const int ti = k / 3, tj = k % 3;
        bf16x8 B[2][3];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const __bf16 *bp = sH + c3_swz((wave + 4 * r + ti) * HWW + jj + tj, kr);
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) B[r][pc] = *reinterpret_cast<const bf16x8 *>(bp + pc * PE);
        }
#pragma unroll
        for (int kd = 0; kd < 3; ++kd)
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            bf16x8 A[3];
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) A[pc] = wb[(((k * 3 + kd) * 2 + m) * 3 + pc) * 64];
#pragma unroll
            for (int r = 0; r < 2; ++r) acc[2 - kd][r][m] = mfma_split6(A, B[r], acc[2 - kd][r][m]);
          }
      }
    }
    if (d >= 1) store_plane(d - 1, acc[0]);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        acc[0][r][m] = acc[1][r][m];
        acc[1][r][m] = acc[2][r][m];
        acc[2][r][m] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  }
  store_plane(D - 1, acc[0]);
}

}  // namespace

extern "C" {

int aanet_conv3d_supported(int c, int co, int kd, int kh, int kw, int stride, int pad, int dil,
                           int groups) {
  return c3_supported(1, 0, c, co, kd, kh, kw, stride, pad, 0, dil, groups);
}

size_t aanet_conv3d_pack_bytes(int co, int c) { return c3_pack_bytes(co, c); }

int aanet_conv3d_pack_f32(const float *w, int co, int c, void *wsplit, aanet_stream_t stream) {
  return c3_pack<false>(w, co, c, wsplit, stream);
}

int aanet_conv3d_fused_f32(const float *x, const void *wsplit, const float *bias,
                           const float *residual, int act, float *out, int n, int c, int d, int h,
                           int w, int co, aanet_stream_t stream) {
  return c3_launch(conv3d_kernel, C3Tiling{TR, TC, h, w}, C3Extent{d, h, w}, x, wsplit, bias,
                   residual, act, out, n, c, d, h, w, co, stream);
}

}  // extern "C"
