// conv3d_head.hip -- the one-output-channel 3x3x3 heads of the 3-D aggregators in eval
// (nets/aggregation.py: StereoNet's and PSMNet-basic's final_conv, the hourglass aggregator's
// classif1-3[2], GC-Net's trans_conv5) for gfx950, two forms on channels-last fp32 input
// x [n][d][h][w][c], c in {32, 64, 96, 128}, ONE output channel:
//   head:            out = act(conv3d(x, W, stride 1, pad 1) + bias [+ residual]),  D x H x W
//   transposed head: out = act(conv_transpose3d(x, W, stride 2, pad 1, output_padding 0) + bias
//                            [+ residual]),  (2D-1) x (2H-1) x (2W-1)
// residual / out [n][1][do][ho][wo] contiguous (one channel: NCDHW and NDHWC are the same bytes).
// W is the module's own weight: a Conv3d [1][c][27] and a ConvTranspose3d [c][1][27] are both
// w[c * 27 + k], k = kd * 9 + kh * 3 + kw, so there is no pack launch; neither form flips it.
//
// The problem is memory-bound (2 * 27 FLOP per input float), and the 32-output-channel blocks of
// conv3d.hip / deconv3d.hip would waste 31/32 of their MFMA work on it.  "Taps as M" instead: a
// workgroup (4 waves) owns an 8 x 16 (h x w) tile of one image and marches through the input
// planes; per plane
//   phase 1  T[k][p] = sum_c W[k][c] * x[p][c] for the 27 taps k and every position p of the
//            tile's halo: a GEMM with M = 27 taps (padded to two 16-row blocks), K = C, N = halo
//            positions (12 blocks of 16, 3 per wave), on the exact-fp32 v_mfma_f32_16x16x4_f32.
//            The B operand comes straight from global memory: lane (nn = lane % 16, kq = lane / 16)
//            loads the float4s of channels 16j + 4kq + 0..3 of its position, MFMA step (j, s) uses
//            element s, and the A fragment (registers, loaded once per workgroup) holds
//            W[tap][16j + 4kq + s] to match.  x is read once per workgroup (1.41x for the halo).
//   phase 2  T goes to LDS tap-major ([32][TS], TS = 196: the four kq groups of a write land 16
//            banks apart, the 16 positions of a group on consecutive banks) and is gathered, one
//            owner per output:
//            head: out[q] = sum_k T[k][q + delta_k]; the nine in-plane taps of input plane d feed
//            output planes d+1, d, d-1 through kd = 0, 1, 2 -- three rolling per-pixel accumulators
//            as in conv3d_kernel.
//            transposed: o = 2p - 1 + k per axis, so an even output takes (p = o/2, k = 1) and an
//            odd one (p = (o-1)/2, k = 2) and (p = (o+1)/2, k = 0); input position (a, b) owns the
//            four outputs (2a + ph, 2b + pw), fed by inputs (a + dy, b + dx), dy <= ph, dx <= pw
//            (halo +1 on the high side only).  Input plane d completes output planes 2d - 1 and 2d
//            and carries 2d + 1.  No atomics, no col2im.
// Padding in h / w is the zero a buffer load returns past its range; padding in d is planes that
// are never staged.  The bias is added in the epilogue, never inside T.  The next plane's loads
// are in flight in registers while this one is written to LDS and gathered.
//
// Addressing: one buffer resource per image, 32-bit byte offsets inside it; the entry points
// refuse volumes of 2^31 bytes per image.
//
// Numerics: fp32 products and fp32 accumulation throughout (no bf16 split).  Per output the order
// is input plane ascending, then tap ascending (transposed: (dy, dx) ascending; an odd plane's
// kd = 2 part before its kd = 0 part), each T an MFMA chain over the channels in a fixed order --
// independent of the batch and of the launch.
#include "conv3d_common.h"

namespace {

constexpr int NT = 256;          // 4 waves, three 16-position blocks each
constexpr int TR = 8, TC = 16;   // tile (h x w): outputs (head) or owning input positions (transposed)
constexpr int NB = 3;            // position blocks per wave: 4 * 3 * 16 = 192 >= 180 halo positions
constexpr int TS = 196;          // floats per tap row of T: >= 192, 4 * TS % 64 == 16
constexpr unsigned OOB = C3_OOB;

struct H3Args {
  const float *x;     // [N][D][H][W][C]
  const float *w;     // [C][27]
  const float *bias;  // one float or NULL
  const float *res;   // [N][Do][Ho][Wo] or NULL
  float *out;         // [N][Do][Ho][Wo]
  int N, D, H, W, act;
};

__device__ __forceinline__ void buf_st1(brsrc_t r, unsigned off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)off, 0, 0);
}

// NJ = C / 16; UP: the transposed head
template <int NJ, bool UP>
__global__ __launch_bounds__(NT) void conv3d_head_kernel(H3Args a) {
  constexpr int C = 16 * NJ;
  constexpr int LO = UP ? 0 : 1;                         // halo rows / columns on the low side
  constexpr int HR = TR + 1 + LO, HWW = TC + 1 + LO;     // halo 10 x 18, transposed 9 x 17
  constexpr int NPOS = HR * HWW;                         // 180 / 153 positions
  static_assert(NPOS <= 4 * NB * 16 && 4 * NB * 16 <= TS, "halo positions fit the blocks and a T row");
  __shared__ float sT[32 * TS];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, nn = lane & 15;
  const int D = a.D, H = a.H, W = a.W;
  const int Do = UP ? 2 * D - 1 : D, Ho = UP ? 2 * H - 1 : H, Wo = UP ? 2 * W - 1 : W;
  const int tx = (W + TC - 1) / TC, ntiles = tx * ((H + TR - 1) / TR);
  const int n = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
  const int y0 = (tile / tx) * TR, x0 = (tile % tx) * TC;  // input coordinates (= output, head)
  const long in_img = (long)D * H * W * C, out_img = (long)Do * Ho * Wo;  // elements, < 2^29
  const brsrc_t xr = buf_rsrc(a.x + n * in_img, in_img * 4);
  const brsrc_t orr = buf_rsrc(a.out + n * out_img, out_img * 4);
  const float *resp = a.res ? a.res + n * out_img : a.out + n * out_img;  // a valid base either way
  const brsrc_t rr = buf_rsrc(resp, out_img * 4);
  const bool has_res = a.res != nullptr;
  const int act = a.act;
  const float bias = a.bias ? a.bias[0] : 0.f;
  const unsigned in_plane = (unsigned)(H * W * C) * 4u;  // bytes

  // A fragments: row (tap) 16mb + nn, K index kq of step (j, s) = channel 16j + 4kq + s
  float A[2][NJ][4];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int tap = 16 * mb + nn;
        A[mb][j][s] = tap < 27 ? a.w[(16 * j + 4 * kq + s) * 27 + tap] : 0.f;
      }

  // this lane's position of block b: byte offset of its channel quad 4kq inside a plane, or OOB
  // outside the image / past the halo (the range check then returns zeros: the padding)
  unsigned poff[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int p = 16 * (wave + 4 * b) + nn;
    const int yy = y0 - LO + p / HWW, xx = x0 - LO + p % HWW;
    const bool ok = p < NPOS && yy >= 0 && yy < H && xx >= 0 && xx < W;
    poff[b] = ok ? (unsigned)(((yy * W + xx) * C + 4 * kq) * 4) : OOB;
  }
  f32x4 xv[NB][NJ];
  auto load_plane = [&](int d) {
    const unsigned uni = (unsigned)d * in_plane;  // + 64j < 2^31: OOB stays out of range
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int j = 0; j < NJ; ++j) xv[b][j] = buf_ld4(xr, poff[b] + uni + 64u * j);
  };

  // the gather's pixel: tile row 2 wave + (kq & 1), column nn; lanes 32..63 mirror lanes 0..31
  // (the same LDS addresses, a broadcast) and store nothing
  const int pr = 2 * wave + (kq & 1);
  const bool owner = lane < 32;
  const float *tp = sT + pr * HWW + nn;
  auto epilogue = [&](bool ok, int dz, int oy, int ox, float v) {
    const unsigned off = ok ? (unsigned)((dz * Ho + oy) * Wo + ox) * 4u : OOB;
    v += bias;
    if (has_res) v += buf_ld1(rr, off);
    buf_st1(orr, off, act_f(v, act));
  };

  // head: acc[s] = output plane d_in - 1 + s; transposed: acc[0..3] = the carried odd plane
  // 2 d_in - 1, by in-plane phase 2 ph + pw
  float acc[UP ? 4 : 3];
#pragma unroll
  for (int s = 0; s < (UP ? 4 : 3); ++s) acc[s] = 0.f;

  load_plane(0);
  for (int d = 0; d < D; ++d) {
    // phase 1: t[b][mb][reg] = T[16mb + 4kq + reg][position nn of block wave + 4b]
    f32x4 t[NB][2];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      t[b][0] = t[b][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (16 * (wave + 4 * b) >= NPOS) continue;  // wave-uniform: a block past the halo
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb) t[b][mb] = mfma16x16x4(A[mb][j][s], xv[b][j][s], t[b][mb]);
    }
    if (d + 1 < D) load_plane(d + 1);
    __syncthreads();  // every wave is done gathering the previous plane
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (16 * (wave + 4 * b) >= NPOS) continue;
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sT[(16 * mb + 4 * kq + r) * TS + 16 * (wave + 4 * b) + nn] = t[b][mb][r];
    }
    __syncthreads();

    // phase 2
    if constexpr (!UP) {
#pragma unroll
      for (int kd = 0; kd < 3; ++kd) {
        float s = acc[2 - kd];
#pragma unroll
        for (int k = 0; k < 9; ++k) s += tp[(kd * 9 + k) * TS + (k / 3) * HWW + k % 3];
        acc[2 - kd] = s;
      }
      const int y = y0 + pr, x = x0 + nn;
      if (d >= 1) epilogue(owner && y < H && x < W, d - 1, y, x, acc[0]);
      acc[0] = acc[1];
      acc[1] = acc[2];
      acc[2] = 0.f;
    } else {
      float ev[4], nx[4];
#pragma unroll
      for (int ph = 0; ph < 2; ++ph)
#pragma unroll
        for (int pw = 0; pw < 2; ++pw) {
          float s0 = acc[2 * ph + pw], s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int dy = 0; dy <= ph; ++dy)
#pragma unroll
            for (int dx = 0; dx <= pw; ++dx) {
              // input (a + dy, b + dx) reaches output (2a + ph, 2b + pw) through kh = ph + 1 - 2 dy
              const int k = (ph + 1 - 2 * dy) * 3 + (pw + 1 - 2 * dx), o = dy * HWW + dx;
              s0 += tp[k * TS + o];
              s1 += tp[(9 + k) * TS + o];
              s2 += tp[(18 + k) * TS + o];
            }
          acc[2 * ph + pw] = s0;
          ev[2 * ph + pw] = s1;
          nx[2 * ph + pw] = s2;
        }
      const int ya = y0 + pr, xa = x0 + nn;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int oy = 2 * ya + (p >> 1), ox = 2 * xa + (p & 1);
        const bool ok = owner && oy < Ho && ox < Wo;
        if (d >= 1) epilogue(ok, 2 * d - 1, oy, ox, acc[p]);
        epilogue(ok, 2 * d, oy, ox, ev[p]);
        acc[p] = nx[p];
      }
    }
  }
  if constexpr (!UP) {
    const int y = y0 + pr, x = x0 + nn;
    epilogue(owner && y < H && x < W, D - 1, y, x, acc[0]);
  }
}

int head_supported(bool up, int c, int co, int kd, int kh, int kw, int stride, int pad, int out_pad,
                   int dil, int groups) {
  if (!c3_conv_args_ok(c, co, kd, kh, kw, stride, pad, out_pad, dil, groups)) return AANET_EINVAL;
  const bool ok = co == 1 && kd == 3 && kh == 3 && kw == 3 && stride == (up ? 2 : 1) && pad == 1 &&
                  out_pad == 0 && dil == 1 && groups == 1 && c3_channels(c);
  return ok ? AANET_OK : AANET_EUNSUPPORTED;
}

template <bool UP>
int head_launch(const float *x, const float *w, const float *bias, const float *residual, int act,
                float *out, int n, int c, int d, int h, int w_, aanet_stream_t stream) {
  if (!x || !w || !out || n <= 0 || c <= 0 || d <= 0 || h <= 0 || w_ <= 0 || act < 0 || act > 2)
    return AANET_EINVAL;
  if (!c3_channels(c)) return AANET_EINVAL;
  const long dd = UP ? 2L * d - 1 : d, ho = UP ? 2L * h - 1 : h, wo = UP ? 2L * w_ - 1 : w_;
  if (!c3_volumes_ok((long)d * h * w_ * c, dd * ho * wo)) return AANET_EUNSUPPORTED;
  const unsigned tiles = c3_tiles(h, w_, TR, TC, n);
  if (!tiles) return AANET_EUNSUPPORTED;
  H3Args a;
  a.x = x;
  a.w = w;
  a.bias = bias;
  a.res = residual;
  a.out = out;
  a.N = n, a.D = d, a.H = h, a.W = w_, a.act = act;
  const dim3 grid(tiles), block(NT);
  switch (c) {
    case 32: hipLaunchKernelGGL((conv3d_head_kernel<2, UP>), grid, block, 0, as_hip(stream), a); break;
    case 64: hipLaunchKernelGGL((conv3d_head_kernel<4, UP>), grid, block, 0, as_hip(stream), a); break;
    case 96: hipLaunchKernelGGL((conv3d_head_kernel<6, UP>), grid, block, 0, as_hip(stream), a); break;
    default: hipLaunchKernelGGL((conv3d_head_kernel<8, UP>), grid, block, 0, as_hip(stream), a); break;
  }
  return aanet_launch_status();
}

}  // namespace

extern "C" {

int aanet_conv3d_head_supported(int c, int co, int kd, int kh, int kw, int stride, int pad, int dil,
                                int groups) {
  return head_supported(false, c, co, kd, kh, kw, stride, pad, 0, dil, groups);
}

int aanet_deconv3d_head_supported(int c, int co, int kd, int kh, int kw, int stride, int pad,
                                  int out_pad, int dil, int groups) {
  return head_supported(true, c, co, kd, kh, kw, stride, pad, out_pad, dil, groups);
}

int aanet_conv3d_head_f32(const float *x, const float *w, const float *bias, const float *residual,
                          int act, float *out, int n, int c, int d, int h, int w_,
                          aanet_stream_t stream) {
  return head_launch<false>(x, w, bias, residual, act, out, n, c, d, h, w_, stream);
}

int aanet_deconv3d_head_f32(const float *x, const float *w, const float *bias, const float *residual,
                            int act, float *out, int n, int c, int d, int h, int w_,
                            aanet_stream_t stream) {
  return head_launch<true>(x, w, bias, residual, act, out, n, c, d, h, w_, stream);
}

}  // extern "C"
