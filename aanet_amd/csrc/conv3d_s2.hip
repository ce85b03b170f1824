// conv3d_s2.hip -- the 3-D aggregators' down-sampling convs in eval (nets/aggregation.py: Conv3d
// 3x3x3, stride 2, padding 1, dilation 1, one group, BN folded by the caller) for gfx950:
//   out = act(conv3d(x, W, stride 2, padding 1) + bias [+ residual]),
//   x [n][d][h][w][c], residual / out [n][do][ho][wo][co] channels-last, do = (d + 1) / 2 etc.
//
// Depth marching as in conv3d.hip, with two rolling accumulator sets instead of three.  A
// workgroup (4 waves) owns a 4 x 16 (ho x wo) output tile of one image and one block of 32 output
// channels (grid.y) and walks the input planes d_in = 0 .. D-1.  An even plane feeds output plane
// d_in / 2 through kd = 1; an odd plane feeds (d_in - 1) / 2 through kd = 2, which completes it,
// and (d_in + 1) / 2 through kd = 0.  For every plane and 32-channel chunk the tile's 9 x 33 input
// halo is loaded once, split into its three bf16 pieces once and stored in LDS (57 KB: two
// workgroups per CU); the next plane's loads are in flight in registers meanwhile.
//
// B-fragment reads.  Lane jj of a wave reads input column 2jj + tj of its row.  The halo rows are
// stored de-interleaved: the 17 even halo columns first, then the 16 odd ones, so that column
// 2jj + tj is slot (tj & 1) * 17 + jj + (tj >> 1) -- unit stride in jj for every tap, the read
// pattern of conv3d.hip, and the XOR swizzle of c3_swz serves it unchanged.
//
// Wave w owns tile rows 2(w & 1), 2(w & 1) + 1 and the 16 output channels of half m = w >> 1: an A
// fragment (pre-split weights from L2 / L1) feeds both rows.  Lane (kr = lane / 16, jj = lane % 16)
// = column jj, channels 8kr .. 8kr + 7 of the B fragment.
//
// Addressing: one buffer resource per image, 32-bit byte offsets inside it; the entry point
// refuses volumes of 2^31 bytes per image.
//
// Numerics: the split-bf16 contraction of split.h (six piece products, fp32 accumulation); per
// output the order is input plane, chunk, in-plane tap ascending -- independent of the batch.
#include "conv3d_common.h"

namespace {

constexpr int NT = C3_NT;                        // 4 waves: two tile rows x one 16-channel half each
constexpr int TR = 4, TC = 16;                   // output tile (ho x wo)
constexpr int HR = 2 * TR + 1, HWW = 2 * TC + 1; // input halo 9 x 33
constexpr int NEVEN = TC + 1;                    // even halo columns come first in a stored row
constexpr int NPOS = HR * HWW;                   // 297 positions
constexpr int PE = NPOS * 32;                    // bf16 per piece plane
constexpr int HIT = (NPOS * 4 + NT - 1) / NT;    // halo octets (8 channels of a position) per thread
constexpr unsigned OOB = C3_OOB;

// LDS position of halo (row, column): columns de-interleaved by parity
__device__ __forceinline__ int s2_pos(int hr, int hc) { return hr * HWW + (hc & 1) * NEVEN + (hc >> 1); }

__global__ __launch_bounds__(NT, 2) void conv3d_s2_kernel(C3Args a) {
  __shared__ __attribute__((aligned(16))) __bf16 sH[3 * PE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rp = wave & 1, m = wave >> 1;
  const int kr = lane >> 4, jj = lane & 15;
  const int C = a.C, D = a.D, H = a.H, W = a.W, Co = a.Co;
  const int Do = (D + 1) / 2, Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int tx = (Wo + TC - 1) / TC, ntiles = tx * ((Ho + TR - 1) / TR);
  const int n = blockIdx.x / ntiles, tile = blockIdx.x % ntiles, cb = blockIdx.y;
  const int y0 = (tile / tx) * TR, x0 = (tile % tx) * TC;  // output coordinates
  const int ncc = C / 32;
  const long in_img = (long)D * H * W * C, out_img = (long)Do * Ho * Wo * Co;  // elements, < 2^29
  const brsrc_t xr = buf_rsrc(a.x + n * in_img, in_img * 4);
  const brsrc_t orr = buf_rsrc(a.out + n * out_img, out_img * 4);
  const unsigned in_plane = (unsigned)(H * W * C) * 4u;  // bytes

  // halo item i of this thread: position e >> 2 (row-major over the 9 x 33 halo), channel octet
  // e & 3; its byte offset inside a plane's chunk 0, or OOB outside the image (zeros: the padding)
  unsigned hoff[HIT];
#pragma unroll
  for (int i = 0; i < HIT; ++i) {
    const int e = tid + NT * i, p = e >> 2;
    const int yy = 2 * y0 - 1 + p / HWW, xx = 2 * x0 - 1 + p % HWW;
    const bool ok = p < NPOS && yy >= 0 && yy < H && xx >= 0 && xx < W;
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
      const int e = tid + NT * i, p = e >> 2;
      if (p < NPOS) {
        const float v[8] = {hv[i][0][0], hv[i][0][1], hv[i][0][2], hv[i][0][3],
                            hv[i][1][0], hv[i][1][1], hv[i][1][2], hv[i][1][3]};
        bf16x8 b[3];
        split8(v, b);
        const int o = c3_swz(s2_pos(p / HWW, p % HWW), e & 3);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) *reinterpret_cast<bf16x8 *>(sH + pc * PE + o) = b[pc];
      }
    }
  };

  // acc[s][r]: output plane (d_in + s) / 2 (s = 0: the one in progress, 1: the next), tile row
  // 2rp + r, channels 32cb + 16m + 4kr + 0..3
  f32x4 acc[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 2; ++r) acc[s][r] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
  if (a.bias) {
#pragma unroll
    for (int u = 0; u < 4; ++u) bv[u] = a.bias[32 * cb + 16 * m + 4 * kr + u];
  }
  const float *resp = a.res ? a.res + n * out_img : a.out + n * out_img;  // a valid base either way
  const brsrc_t rr = buf_rsrc(resp, out_img * 4);
  const bool has_res = a.res != nullptr;
  const int act = a.act;
  auto store_plane = [&](int dz, const f32x4 (&ac)[2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int y = y0 + 2 * rp + r, x = x0 + jj;
      const bool ok = y < Ho && x < Wo;
      const unsigned off =
          ok ? (unsigned)(((dz * Ho + y) * Wo + x) * Co + 32 * cb + 16 * m + 4 * kr) * 4u : OOB;
      f32x4 v = ac[r] + bv;
      if (has_res) v += buf_ld4(rr, off);
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = act_f(v[u], act);
      buf_st4(orr, off, v);
    }
  };

  load_halo(0, 0);
  for (int d = 0; d < D; ++d) {
    const bool odd = d & 1;
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
          const __bf16 *bp = sH + c3_swz(s2_pos(2 * (2 * rp + r) + ti, 2 * jj + tj), kr);
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) B[r][pc] = *reinterpret_cast<const bf16x8 *>(bp + pc * PE);
        }
        auto tap = [&](int kd, f32x4 (&ac)[2]) {
          bf16x8 A[3];
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) A[pc] = wb[(((k * 3 + kd) * 2 + m) * 3 + pc) * 64];
#pragma unroll
          for (int r = 0; r < 2; ++r) ac[r] = mfma_split6(A, B[r], ac[r]);
        };
        if (odd) {
          tap(2, acc[0]);
          tap(0, acc[1]);
        } else {
          tap(1, acc[0]);
        }
      }
    }
    if (odd) {  // plane (d - 1) / 2 has its three depth taps
      store_plane((d - 1) / 2, acc[0]);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        acc[0][r] = acc[1][r];
        acc[1][r] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  if (D & 1) store_plane(D / 2, acc[0]);  // the last plane's kd = 2 neighbour is padding
}

}  // namespace

extern "C" {

int aanet_conv3d_s2_supported(int c, int co, int kd, int kh, int kw, int stride, int pad, int dil,
                              int groups) {
  return c3_supported(2, 0, c, co, kd, kh, kw, stride, pad, 0, dil, groups);
}

// the pack is the stride-1 conv's
size_t aanet_conv3d_s2_pack_bytes(int co, int c) { return aanet_conv3d_pack_bytes(co, c); }

int aanet_conv3d_s2_pack_f32(const float *w, int co, int c, void *wsplit, aanet_stream_t stream) {
  return aanet_conv3d_pack_f32(w, co, c, wsplit, stream);
}

int aanet_conv3d_s2_fused_f32(const float *x, const void *wsplit, const float *bias,
                              const float *residual, int act, float *out, int n, int c, int d,
                              int h, int w, int co, aanet_stream_t stream) {
  const C3Extent o{((long)d + 1) / 2, ((long)h + 1) / 2, ((long)w + 1) / 2};
  return c3_launch(conv3d_s2_kernel, C3Tiling{TR, TC, o.h, o.w}, o, x, wsplit, bias, residual,
                   act, out, n, c, d, h, w, co, stream);
}

}  // extern "C"
