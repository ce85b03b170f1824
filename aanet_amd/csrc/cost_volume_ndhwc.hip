// cost_volume_ndhwc.hip -- the concat / difference volume of nets/cost.py:22-38 written
// channels-last: out[b][d][y][x][oc], oc innermost (the memory of a [n, oc, D, h, w] tensor in
// torch.channels_last_3d), which is what the 3-D aggregators' first conv reads.  Values are those
// of the NCDHW kernels of cost_volume.hip bit for bit: x >= d -> left[c][x] and right[c][x - d]
// (concat) or their difference; x < d -> 0.
//
// Write-bound like its NCDHW neighbour: the two feature maps are read (about) once, the volume is
// written once.  The features are NCHW, the output wants all channels of a position together, so
// the workgroup transposes through LDS.
//
// One workgroup owns XS = 64 positions of one (b, y) row and a chunk of <= DCH = 64 disparities,
// and walks the channels in chunks of <= CCH = 32.  Per channel chunk it stages, position-major,
//   sL[XS][cc]           the left segment, and
//   sR[XS + dn - 1][cc]  the right window x0 - d0 - (dn - 1) .. x0 + XS - 1 - d0 (zero left of the
//                        row),
// then every thread keeps the left quad of its (position, channel quad) slot in registers for the
// whole d loop and per d does one 16-byte LDS read of the right quad at position x - d and one
// (difference) or two (concat) 16-byte global stores.  Lanes are consecutive in (position, quad),
// so a wave's stores cover 8 positions x 128 B (c = 32: the left halves, then the right halves, of
// eight 256-B position records: whole 128-B lines), and a (d, y) segment of the stream is
// XS * oc * 4 contiguous bytes (16 KB at c = 32).
//
// Why x segments and not one full row: a full C5 row pair (c = 32, w = 312) is 80 KB of LDS, one
// workgroup of 256 threads per CU, and its size grows with w and c without bound.  A 64-position
// segment with its right window is (64 + 127) * 32 * 4 = 24 KB whatever w, c and D are (six
// workgroups per CU), and the price is that the right window overlaps the neighbouring segment's:
// (64 + dn - 1) / 64 reads of the right row instead of 1, from L2, against D times that in writes.
//
// LDS layout.  The pitch is exactly cc floats (no padding), so the 64 lanes of a ds_read_b128 --
// 8 positions x 8 quads at c = 32 -- read 1 KB of consecutive 16-byte slots: each of the
// instruction's four 16-lane groups covers 64 distinct banks ((a/4) mod 64), conflict-free for
// every d (a shift by d moves the whole 1 KB by d * cc * 4 bytes).  With that pitch a transposing
// ds_write_b32 (bank (a/4) mod 32, two 32-lane groups) of 32 consecutive positions of one channel
// would put all lanes on the 4 banks of one quad.  So the quads of a position are XOR-swizzled
// with the low two bits of the position index, physical quad = q ^ (j & 3), and the staging lanes
// of a 32-lane group are 4 positions x 4 channels-of-a-quad x the 2 quads q and q + 4:
// bank = 4 * ((q ^ j) [+ 4]) + r is 8 distinct quads x 4 = 32 distinct banks.  Only two bits, so
// that the swizzle permutes quads inside each 64-B half of a position and the read argument above
// (which half of which position a 16-lane group touches) is untouched.  The swizzle needs the quad
// count of the chunk to be a multiple of 4 (cc = 16 or 32); other chunk widths are staged
// unswizzled (conflicts on the staging writes only, a few percent of a workgroup's LDS cycles).
#include "common.h"

namespace {

constexpr int XS = 64;    // positions per workgroup
constexpr int DCH = 64;   // disparities per workgroup
constexpr int CCH = 32;   // channels per LDS stage
constexpr int NT = 256;
constexpr int NSLOT = XS * (CCH / 4) / NT;  // (position, quad) slots per thread: 2

template <bool CONCAT>
__global__ __launch_bounds__(NT) void shift_volume_ndhwc_kernel(const float *__restrict__ L,
                                                                const float *__restrict__ R,
                                                                float *__restrict__ out, int C,
                                                                int H, int W, int D, int nseg,
                                                                int nchunk) {
  __shared__ __attribute__((aligned(16))) float sL[XS * CCH];
  __shared__ __attribute__((aligned(16))) float sR[(XS + DCH - 1) * CCH];
  const int tid = threadIdx.x;
  long id = blockIdx.x;
  const int seg = (int)(id % nseg);
  id /= nseg;
  const int chunk = (int)(id % nchunk);
  id /= nchunk;
  const int y = (int)(id % H), b = (int)(id / H);
  const int x0 = seg * XS, d0 = chunk * DCH;
  const int dn = min(DCH, D - d0);       // disparities of this chunk
  const int xr0 = x0 - d0 - (dn - 1);    // first position of the right window
  const int nxr = XS + dn - 1;           // its width
  const int OC = CONCAT ? 2 * C : C;
  const long HW = (long)H * W;
  // staging lane -> (position in a block of 4, channel in a quad, lower / upper quad)
  const int l32 = tid & 31, g32 = tid >> 5;
  const int sj = l32 & 3, sr = (l32 >> 2) & 3, sqh = l32 >> 4;

  for (int c0 = 0; c0 < C; c0 += CCH) {
    const int cc = min(CCH, C - c0), QP = cc >> 2;  // cc % 4 == 0 (launcher)
    const int sw = (QP & 3) == 0 ? 3 : 0;
    if (c0) __syncthreads();  // the previous chunk's reads are done
    // stage: tasks of 4 positions x (quad q, quad q + 4), one per 32-lane group and step
    const float *Lb = L + ((long)b * C + c0) * HW + (long)y * W;
    const float *Rb = R + ((long)b * C + c0) * HW + (long)y * W;
    const int nq0 = min(QP, 4);  // q = q0 + 4 * sqh, q0 < nq0 (QP <= 8)
    const int ntl = (XS / 4) * nq0, ntr = ((nxr + 3) / 4) * nq0;
    for (int t = g32; t < ntl + ntr; t += NT / 32) {
      const bool right = t >= ntl;
      const int u = right ? t - ntl : t;
      const int q = u % nq0 + 4 * sqh;
      const int j = 4 * (u / nq0) + sj;  // position index in the segment / window
      if (q >= QP || j >= (right ? nxr : XS)) continue;
      const int x = (right ? xr0 : x0) + j, ch = 4 * q + sr;
      const float v = (x >= 0 && x < W) ? (right ? Rb : Lb)[(long)ch * HW + x] : 0.f;
      (right ? sR : sL)[j * cc + 4 * (q ^ (j & sw)) + sr] = v;
    }
    __syncthreads();

    int jl[NSLOT], ql[NSLOT], xs[NSLOT];
    f32x4 lv[NSLOT];
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
      const int s = tid + NT * i;
      const bool live = s < XS * QP;
      jl[i] = live ? s / QP : 0;
      ql[i] = live ? s % QP : 0;
      xs[i] = live && x0 + jl[i] < W ? x0 + jl[i] : -1;  // -1: the slot never stores
      lv[i] = *reinterpret_cast<const f32x4 *>(sL + jl[i] * cc + 4 * (ql[i] ^ (jl[i] & sw)));
    }
    for (int dd = 0; dd < dn; ++dd) {
      const int d = d0 + dd;
      float *od = out + (((long)b * D + d) * H + y) * W * OC + c0;
#pragma unroll
      for (int i = 0; i < NSLOT; ++i) {
        if (NT * i >= XS * QP) break;  // uniform
        if (xs[i] < 0) continue;
        const int jr = jl[i] + (dn - 1) - dd;  // window index of x - d: always inside the window
        const f32x4 rv = *reinterpret_cast<const f32x4 *>(sR + jr * cc + 4 * (ql[i] ^ (jr & sw)));
        const bool ok = xs[i] >= d;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        float *o = od + (long)xs[i] * OC + 4 * ql[i];
        if (CONCAT) {
          *reinterpret_cast<f32x4 *>(o) = ok ? lv[i] : zero;
          *reinterpret_cast<f32x4 *>(o + C) = ok ? rv : zero;
        } else {
          *reinterpret_cast<f32x4 *>(o) = ok ? lv[i] - rv : zero;
        }
      }
    }
  }
}

// Any c, any alignment: one output element per thread, oc innermost (consecutive lanes write
// consecutive floats; the feature reads are strided by a plane and come from L2).
template <bool CONCAT>
__global__ __launch_bounds__(256) void shift_volume_ndhwc_scalar_kernel(
    const float *__restrict__ L, const float *__restrict__ R, float *__restrict__ out, int C, int H,
    int W, int D, long total) {
  const int OC = CONCAT ? 2 * C : C;
  const long HW = (long)H * W;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int oc = (int)(e % OC);
    long t = e / OC;
    const int x = (int)(t % W);
    t /= W;
    const int y = (int)(t % H);
    t /= H;
    const int d = (int)(t % D);
    const long b = t / D;
    float v = 0.f;
    if (x >= d) {
      const int c = oc < C ? oc : oc - C;
      const long p = (b * C + c) * HW + (long)y * W + x;
      if (CONCAT)
        v = oc < C ? L[p] : R[p - d];
      else
        v = L[p] - R[p - d];
    }
    out[e] = v;
  }
}

template <bool CONCAT>
int launch_ndhwc(const float *left, const float *right, float *out, int n, int c, int h, int w,
                 int max_disp, hipStream_t st) {
  const int nseg = host_div_up(w, XS), nchunk = host_div_up(max_disp, DCH);
  const long nblk = (long)nseg * nchunk * h * n;
  if (c % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && nblk <= 0x7fffffffL) {
    hipLaunchKernelGGL(shift_volume_ndhwc_kernel<CONCAT>, dim3((unsigned)nblk), dim3(NT), 0, st,
                       left, right, out, c, h, w, max_disp, nseg, nchunk);
  } else {
    const long total = (long)n * (CONCAT ? 2 : 1) * c * max_disp * h * w;
    const long g = (total + 255) / 256;
    hipLaunchKernelGGL(shift_volume_ndhwc_scalar_kernel<CONCAT>,
                       dim3((unsigned)(g > 65536 ? 65536 : g)), dim3(256), 0, st, left, right, out,
                       c, h, w, max_disp, total);
  }
  return aanet_launch_status();
}

}  // namespace

extern "C" int aanet_concat_volume_ndhwc_f32(const float *left, const float *right, float *out,
                                             int n, int c, int h, int w, int max_disp,
                                             aanet_stream_t stream) {
  AANET_HOST_CHECK(left && right && out && n > 0 && c > 0 && h > 0 && w > 0 && max_disp > 0);
  return launch_ndhwc<true>(left, right, out, n, c, h, w, max_disp, as_hip(stream));
}

extern "C" int aanet_diff_volume_ndhwc_f32(const float *left, const float *right, float *out,
                                           int n, int c, int h, int w, int max_disp,
                                           aanet_stream_t stream) {
  AANET_HOST_CHECK(left && right && out && n > 0 && c > 0 && h > 0 && w > 0 && max_disp > 0);
  return launch_ndhwc<false>(left, right, out, n, c, h, w, max_disp, as_hip(stream));
}
