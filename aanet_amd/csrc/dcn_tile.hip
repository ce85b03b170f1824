// dcn_tile.hip -- the deformable bottleneck tail of the cost aggregation (nets/deform.py:207-236:
// DeformConv2d + BN2 + ReLU -> conv3 1x1 + BN3 + identity + ReLU, and the scale-0 cross-scale
// sum of nets/aggregation.py:387-400) in its "window" form, for gfx950.
//
// Why a second DCN kernel.  The generic engine (mdcn.hip conv_fwd_kernel, MODE 1) gathers the
// four bilinear corners of every (pixel, tap, channel quad) straight from L2: 9.2 KB per output
// pixel, 3.9 GB per C2 scale-0 launch, and it ran at about half the L2-served gather rate with
// the matrix pipe 80 % idle.  Here a workgroup owns an 8 x 16 pixel tile and, per
// 32-channel deformable group, stages the tile's input WINDOW once in LDS: every sample whose
// offset lies in [-2, 2) reads its corners from the window (9 taps x 4 corners from one 48 KB
// copy), so L2 sees each input line about three times per launch instead of ~36.  Samples outside
// the window (large offsets) read their corners from global memory, so any offset is handled.
//
// The kernel is templated on the deformable group width: 32 channels (the scale-0 block, C = 64,
// the window of one group per phase) or 16 (the scale-1 block, C = 32: both groups share one
// 32-channel K slice and each lane blends with its own group's sampling state).
//
// Work split.  Wave w owns tile row w (16 output pixels) and all output channels: lane
// (kr = lane / 16, jj = lane % 16) blends pixel jj's channels 8kr..8kr+7 -- exactly the B fragment
// of v_mfma_f32_16x16x32_bf16 -- so the deformable im2col never goes through LDS and needs no
// per-chunk hand-off between waves.  The A fragments (pre-split weights of one tap) are staged
// through registers into a double-buffered LDS slot, one tap ahead.  The sampling state (window position + four mask-folded
// corner weights) of 4 taps is computed at once (lane group kr takes tap t0+kr) and handed to the
// lanes of the other taps with ds_bpermute.
//
// Numerics are those of the generic engine: corner positions, validity and weights follow
// kernel.cu:467-497 / make_samp4 bit for bit (fp contraction off); the blend is
// ((c0 w0 + c1 w1) + c2 w2) + c3 w3 with the mask folded into the weights; the contraction is the
// split-bf16 one (three exact bf16 pieces, six products, fp32 accumulation; split.h).
#include "dcn_tile.h"
#include "split.h"

#include <cstdio>

#include <stdlib.h>

namespace {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

constexpr int NT = 512;          // 8 waves, one tile row each
constexpr int TR = 8, TC = 16;   // tile: 8 rows x 16 columns of output pixels
constexpr int RW = 2;            // window margin beyond the taps: offsets in [-RW, RW) stay inside
constexpr int K = 9;             // 3x3 taps
constexpr int OP = TR * TC + 4;  // epilogue tile pitch (floats)

// the resource of an optional tensor's image planes: an absent tensor gets 0 records (its loads
// return 0, its stores are dropped), on any valid base
__device__ __forceinline__ brsrc_t opt_rsrc(const float *p, const float *any, long img, long bytes) {
  return buf_rsrc(p ? p + img : any, p ? bytes : 0);
}

// Sampling state of one (pixel, tap, deformable group): the window position of the top-left
// corner (-1: a corner lies outside the window -> global gather) and the four corner weights with
// the modulation mask folded in.  Same float steps as mdcn.hip finish_params + make_samp4.
struct TapState {
  int pos;
  float w0, w1, w2, w3;
};

template <int DIL, int WR, int WC>
__device__ __forceinline__ TapState tap_state(float oh, float ow, float ml, int yy, int xx, bool pv,
                                              int t, int H, int W, int wy0, int wx0,
                                              int mask_logits, float mask_scale) {
#pragma clang fp contract(off)
  const int i = t / 3, j = t - 3 * (t / 3);
  float m = mask_logits ? mask_scale * __builtin_amdgcn_rcpf(1.f + __expf(-ml)) : ml;
  if (!pv) m = 0.f;
  const float h = (float)(yy - DIL + i * DIL) + oh;
  const float w = (float)(xx - DIL + j * DIL) + ow;
  const bool valid = h > -1.f && w > -1.f && h < (float)H && w < (float)W;
  const int hl = (int)floorf(h), wl = (int)floorf(w);
  const float lh = h - (float)hl, lw = w - (float)wl;
  const float hh = 1.f - lh, hw = 1.f - lw;
  TapState s;
  const bool ok1 = valid && hl >= 0 && wl >= 0;
  const bool ok2 = valid && hl >= 0 && wl + 1 <= W - 1;
  const bool ok3 = valid && hl + 1 <= H - 1 && wl >= 0;
  const bool ok4 = valid && hl + 1 <= H - 1 && wl + 1 <= W - 1;
  s.w0 = (ok1 ? hh * hw : 0.f) * m;
  s.w1 = (ok2 ? hh * lw : 0.f) * m;
  s.w2 = (ok3 ? lh * hw : 0.f) * m;
  s.w3 = (ok4 ? lh * lw : 0.f) * m;
  const int rh = hl - wy0, rw = wl - wx0;
  const bool inwin = (unsigned)rh <= (unsigned)(WR - 2) && (unsigned)rw <= (unsigned)(WC - 2);
  // an invalid sample has four zero weights: any in-window position will do
  s.pos = !valid ? 0 : (inwin ? rh * WC + rw : -1);
  return s;
}

// CG = channels per deformable group (two groups): 32 (scale 0: C = 64), 16 (scale 1: C = 32) or
// 64 (the feature extractor's DCNs, C = 128, op-level PLAIN form only: each group spans two
// 32-channel phases, which recompute its sampling state; one workgroup per CU for the LDS).
// A chunk is one tap of a 32-channel K slice ("phase"): with CG = 32 a phase is one group, with
// CG = 16 it holds both groups (lane groups kr = 0, 1 carry group 0's channels, kr = 2, 3 group 1's).
// XN: x is NCHW (the op-level forward, ModulatedDeformConvFunction) instead of channels-last.
// PLAIN: no bottleneck tail -- out = act(post_scale * (DCN + bias) + post_shift), NCHW.
template <int DIL, int CG, bool POST, bool XN = false, bool PLAIN = false>
__global__ __launch_bounds__(NT, CG == 64 ? 2 : 4) void dcn_tile_kernel(DcnTileArgs a) {
  constexpr int CT = 2 * CG;             // channels = Co = Co2
  constexpr int NPH = CT / 32;           // phases
  constexpr int NCH = NPH * K;           // chunks
  constexpr int NCO = CT / 16;           // 16-row co blocks
  constexpr int ABUF = NCO * 3 * 1024;   // one chunk's A fragments: NCO blocks x 3 pieces x 64 lanes x 16 B
  static_assert(CG != 64 || PLAIN, "64-channel groups: op-level form only");
  constexpr bool WG = CG >= 32;          // a phase is (part of) ONE group: lane groups = 4 taps
  constexpr int TPP = WG ? 4 : 2;        // taps per sampling pass (x groups per pass = 4 lane groups)
  constexpr int MG = DIL + RW;                     // window margin around the tile
  constexpr int WR = TR + 2 * MG, WC = TC + 2 * MG;
  constexpr int NPOS = (WR * WC + 63) / 64 * 64;   // positions per quad plane (multiple of 64)
  constexpr int NWI = NPOS / 64;                   // window quads staged per thread (8*NPOS/512)
  constexpr int WIN = 8 * NPOS * 16;               // window bytes: [8 channel quads][NPOS][16 B]
  static_assert(WIN >= (CT < 64 ? CT : 64) * OP * 4, "epilogue tile must fit the window");
  // Three LDS objects: the compiler orders a ds_read after an outstanding LDS-DMA only when they
  // may alias, so the DMA of tap c+1's weights into one A slot never holds reads of the window or
  // of the other slot.
  __shared__ __attribute__((aligned(16))) char sWin[WIN];
  __shared__ __attribute__((aligned(16))) char sA0[ABUF];
  __shared__ __attribute__((aligned(16))) char sA1[ABUF];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kr = lane >> 4, jj = lane & 15;
  const int H = a.H, W = a.W, C = a.C;
#ifdef AANET_DCN_SETPRIO  // A/B: static priority for the second-dispatched half (MI355X_MICROARCH.md)
  if (wave >= 4) __builtin_amdgcn_s_setprio(1);
#endif
#ifdef AANET_DEBUG_SWITCHES
  const int dbg = a.dbg;  // timing-attribution switches (debug build only)
#else
  constexpr int dbg = 0;  // product build: every switch branch folds away at compile time
#endif
  const int tx = (W + TC - 1) / TC, ntiles = tx * ((H + TR - 1) / TR);
  // XCD-aware bijective remap: each XCD walks a contiguous range of tiles (shared window rows)
  const int nwg = gridDim.x, b0 = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = b0 & 7;
  const int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b0 >> 3);
  const int n = bid / ntiles, tile = bid % ntiles;
  const int y0 = (tile / tx) * TR, x0 = (tile % tx) * TC;
  const int wy0 = y0 - MG, wx0 = x0 - MG;
  const int py = y0 + wave, px = x0 + jj;  // this lane's output pixel
  const bool pv = py < H && px < W;
  const int P = H * W;
  const int p4 = (pv ? py * W + px : 0) * 4;
  const int img_bytes = C * P * 4;

  const auto xr = __builtin_amdgcn_make_buffer_rsrc((void *)(a.x + (long)n * C * P), (short)0, img_bytes, 0x00020000);
  const auto offr = __builtin_amdgcn_make_buffer_rsrc((void *)(a.offset + (long)n * a.off_bs), (short)0, 0x7ffffff0, 0x00020000);
  const auto mskr = __builtin_amdgcn_make_buffer_rsrc((void *)(a.mask + (long)n * a.mask_bs), (short)0, 0x7ffffff0, 0x00020000);

  // ---- window staging: quad q of window position pos -> LDS [q][pos]; 8 consecutive lanes take
  // one quad of 8 consecutive positions (each wave-instruction covers 8 whole 128-B lines of x,
  // and 8 consecutive lanes write 8 different LDS banks quads).  Outside the image: zeros.
  // NCHW (XN): element e = one 16-byte segment (4 window columns) of one window row of one of
  // the phase's 32 channels, segments fastest (a row's 96 bytes are contiguous); the store
  // scatters its 4 values to the 4 positions' slots of channel quad ch/4.  W % 4 == 0 and
  // wx0 % 4 == 0, so a segment lies wholly inside or wholly outside the image.
  static_assert(!XN || (WC % 4 == 0 && 32 * WR * (WC / 4) == NT * NWI), "NCHW window staging");
  f32x4 wv[NWI] = {};
  auto load_window = [&](int g) {
#pragma unroll
    for (int i = 0; i < NWI; ++i) {
      const int e = tid + NT * i;
      if constexpr (XN) {
        const int seg = e % (WC / 4), rest = e / (WC / 4), row = rest % WR, ch = rest / WR;
        const int wy = wy0 + row, wx = wx0 + 4 * seg;
        const bool ok = wy >= 0 && wy < H && wx >= 0 && wx < W;
        const int off = ok ? (((g * 32 + ch) * H + wy) * W + wx) * 4 : img_bytes;
        if (!(dbg & 32)) wv[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
      } else {
        const int q = (e >> 3) & 7, pos = (e & 7) | ((e >> 6) << 3);
        const int wy = wy0 + pos / WC, wx = wx0 + pos % WC;
        const bool ok = pos < WR * WC && wy >= 0 && wy < H && wx >= 0 && wx < W;
        const int off = ok ? ((wy * W + wx) * C + 4 * q) * 4 : img_bytes;
        if (!(dbg & 32)) wv[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, g * 128, 0));
      }
    }
  };
  auto store_window = [&]() {
#pragma unroll
    for (int i = 0; i < NWI; ++i) {
      const int e = tid + NT * i;
      if constexpr (XN) {
        const int seg = e % (WC / 4), rest = e / (WC / 4), row = rest % WR, ch = rest / WR;
        float *dst = reinterpret_cast<float *>(sWin + ((ch >> 2) * NPOS + row * WC + 4 * seg) * 16) + (ch & 3);
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[4 * u] = wv[i][u];
      } else {
        const int q = (e >> 3) & 7, pos = (e & 7) | ((e >> 6) << 3);
        *reinterpret_cast<f32x4 *>(sWin + (q * NPOS + pos) * 16) = wv[i];
      }
    }
  };

  // ---- A fragments of chunk c = (group g, tap k): 12 KB, lane-linear, by LDS-DMA one tap ahead
  const char *wsp = reinterpret_cast<const char *>(a.wsplit);
  const int ncc = C / 32;
  auto issue_a = [&](int c, char *dst) {
    if (dbg & 64) return;
    const int g = c / K, k = c - K * (c / K);
    // the split pack is 64-row-tile major: blocks 4t .. 4t+3 of chunk (k, g) at tile t's copy
    const char *src = wsp + (long)((k * ncc + g) * 12) * 1024 + lane * 16;
    const long tile = (long)K * ncc * 12 * 1024;
    for (int pc = wave; pc < 3 * NCO; pc += 8)
      __builtin_amdgcn_global_load_lds((const void *)(src + (pc / 12) * tile + (pc % 12) * 1024),
                                       (lds_void *)(dst + pc * 1024), 16, 0, 0);
  };

  // ---- sampling state: lane group kr computes (tap, group) pt(kr) of this lane's pixel: tap
  // t0 + kr of the phase's group (CG = 32), or tap t0 + (kr & 1) of group kr >> 1 (CG = 16)
  const int pt = WG ? kr : (kr & 1);
  const int lgrp = WG ? 0 : (kr >> 1);  // this lane's group within the phase
  constexpr int PPG = CG == 64 ? 2 : 1;  // phases per group
  float poh = 0.f, pow_ = 0.f, pml = 0.f;  // prefetched offsets / mask of the next pass
  // All three byte offsets are formed before the first load, in 32-bit 24-bit-multiply form: as
  // (plane * P * 4 + p4) the compiler chose v_mad_u64_u32 with a 64-bit addend register pair whose
  // high half was the destination of the offset load just issued, i.e. an s_waitcnt vmcnt(0) (a
  // full memory round trip) in every sampling pass.  Plane indices are < 2 * 2 * 9, P * 4 < 2^24.
  auto load_pass = [&](int g, int t0) {
    const int t = min(t0 + pt, K - 1), gr = WG ? g / PPG : (kr >> 1);
    const unsigned P4 = (unsigned)P * 4u;
    const int o_h = (int)__umul24((unsigned)(gr * 2 * K + 2 * t), P4) + p4;
    const int o_w = o_h + (int)P4;
    const int o_m = (int)__umul24((unsigned)(gr * K + t), P4) + p4;
    poh = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(offr, o_h, 0, 0));
    pow_ = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(offr, o_w, 0, 0));
    pml = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(mskr, o_m, 0, 0));
  };
  TapState ps;  // this lane's state for (tap, group) pt(kr) of the current pass
  auto compute_pass = [&](int t0) {
    ps = tap_state<DIL, WR, WC>(poh, pow_, pml, py, px, pv, min(t0 + pt, K - 1), H, W, wy0, wx0,
                                a.mask_logits, a.mask_scale);
  };
  auto get_state = [&](int k, int t0) -> TapState {
    const int src = (((k - t0 + 2 * lgrp) << 4) | jj) << 2;
    TapState s;
    s.pos = __builtin_amdgcn_ds_bpermute(src, ps.pos);
    s.w0 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, ps.w0)));
    s.w1 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, ps.w1)));
    s.w2 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, ps.w2)));
    s.w3 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, ps.w3)));
    return s;
  };

  f32x4 acc[NCO];
#pragma unroll
  for (int m = 0; m < NCO; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one chunk (tap of a 32-channel K slice): corners -> blend -> split -> 6 NCO MFMAs
  auto tap = [&](int g, int k, const char *sAc, const TapState &s, bool reload) {
    f32x4 cq[4][2];  // corners TL, TR, BL, BR x channel quads 2kr, 2kr+1
    const int lpos = (s.pos < 0 || (dbg & 2)) ? 0 : s.pos;
    const char *base = sWin + (lpos + kr * 2 * NPOS) * 16;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      cq[0][h2] = *reinterpret_cast<const f32x4 *>(base + h2 * NPOS * 16);
      cq[1][h2] = *reinterpret_cast<const f32x4 *>(base + h2 * NPOS * 16 + 16);
      cq[2][h2] = *reinterpret_cast<const f32x4 *>(base + h2 * NPOS * 16 + WC * 16);
      cq[3][h2] = *reinterpret_cast<const f32x4 *>(base + h2 * NPOS * 16 + (WC + 1) * 16);
    }
    float v[8];
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float t = cq[0][h2][u] * s.w0;
        t = __builtin_fmaf(cq[1][h2][u], s.w1, t);
        t = __builtin_fmaf(cq[2][h2][u], s.w2, t);
        t = __builtin_fmaf(cq[3][h2][u], s.w3, t);
        v[4 * h2 + u] = t;
      }
    if (!(dbg & 4) && __builtin_amdgcn_ballot_w64(s.pos < 0)) {  // wave-uniform: some sample left the window
      if (s.pos < 0) {
        // global gather of this lane's corners (blended here, so no load is pending at the join)
#pragma clang fp contract(off)
        const int oplane = ((WG ? g / PPG : lgrp) * 2 * K + 2 * k) * P * 4;
        const float oh = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(offr, p4 + oplane, 0, 0));
        const float ow = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(offr, p4 + oplane + P * 4, 0, 0));
        const int i = k / 3, j = k - 3 * (k / 3);
        const float h = (float)(py - DIL + i * DIL) + oh;
        const float w = (float)(px - DIL + j * DIL) + ow;
        const int hl = (int)floorf(h), wl = (int)floorf(w);
        // pos < 0 only for valid samples; corners outside the image carry weight 0, read as 0
        const int rb = XN ? 4 : C * 4, qo = XN ? (g * 32 + 8 * kr) * P * 4 : (g * 8 + 2 * kr) * 16;
        int o[4];
        o[0] = (hl >= 0 && wl >= 0) ? (hl * W + wl) * rb + qo : img_bytes;
        o[1] = (hl >= 0 && wl + 1 <= W - 1) ? (hl * W + wl + 1) * rb + qo : img_bytes;
        o[2] = (hl + 1 <= H - 1 && wl >= 0) ? ((hl + 1) * W + wl) * rb + qo : img_bytes;
        o[3] = (hl + 1 <= H - 1 && wl + 1 <= W - 1) ? ((hl + 1) * W + wl + 1) * rb + qo : img_bytes;
        f32x4 gq[4][2];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            if constexpr (XN) {  // 8 channel planes; an invalid corner stays past the image
              const int pl = o[cc] == img_bytes ? 0 : P * 4;
#pragma unroll
              for (int u = 0; u < 4; ++u)
                gq[cc][h2][u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                    xr, o[cc] + (4 * h2 + u) * pl, 0, 0));
            } else {
              gq[cc][h2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, o[cc], h2 * 16, 0));
            }
          }
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            float t = gq[0][h2][u] * s.w0;
            t = __builtin_fmaf(gq[1][h2][u], s.w1, t);
            t = __builtin_fmaf(gq[2][h2][u], s.w2, t);
            t = __builtin_fmaf(gq[3][h2][u], s.w3, t);
            v[4 * h2 + u] = t;
          }
      }
    }
    bf16x8 B[3];
    split8(v, B);
    if (reload) {
      // the next phase's window and first offsets: issued once this chunk's corners are blended
      // (their registers free) and before its MFMAs, so the load latency overlaps the MFMA run
      __builtin_amdgcn_sched_barrier(0);
      load_window(g + 1);
      load_pass(g + 1, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    const char *ab = sAc + lane * 16;
#pragma unroll
    for (int m = 0; m < NCO; ++m) {
      bf16x8 A[3];
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) A[pc] = *reinterpret_cast<const bf16x8 *>(ab + (m * 3 + pc) * 1024);
      if (!(dbg & 1)) acc[m] = mfma_split6(A, B, acc[m]);
    }
  };

  // ---- main loop: NPH phases x 9 taps (18 or 9 chunks), one barrier per chunk ----------------
  // L2 warm-up loads (one dword per 128-B line, results unused): the next group's window lines
  // during group 0, the epilogue's identity rows during group 1, so those loads hit L2.
  // Order inside a chunk: the ds_bpermute hand-off of the sampling state comes BEFORE any vector
  // memory op of the chunk.  The compiler cannot tell a ds_bpermute from an LDS access that may
  // alias the outstanding LDS-DMA of the next tap's weights, so it puts s_waitcnt vmcnt(0) in
  // front of it; issued after the DMA, that wait exposed the DMA's whole L2 latency every chunk.
  float pf_win = 0.f, pf_res = 0.f;
  auto step = [&](int c, const char *cur, char *nxt) {
    const int g = c / K, k = c - K * g, t0 = k - k % TPP;
    TapState s;
    if (k == 0) {  // group start: its window (loaded in the chunk before) and pass-0 states
      if (g == 1) asm volatile("" ::"v"(pf_win));
      store_window();
      compute_pass(0);
      s = get_state(k, t0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of A(c) landed
      __syncthreads();
      load_pass(g, TPP);
    } else {
      if (k == t0) compute_pass(k);
      s = get_state(k, t0);
      if (k == t0 && k + TPP < K) load_pass(g, k + TPP);
    }
    if (c + 1 < NCH) issue_a(c + 1, nxt);
    if (NPH == 2 && c == 3 && !XN && tid < WR * WC) {
      const int wy = wy0 + tid / WC, wx = wx0 + tid % WC;
      const bool ok = wy >= 0 && wy < H && wx >= 0 && wx < W;
      pf_win = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
          xr, ok ? (wy * W + wx) * C * 4 : img_bytes, 128, 0));
    }
    if (NPH == 2 && c == 3 && XN && tid < 32 * WR) {  // one dword per window row of group 1
      const int wy = wy0 + (tid % WR);
      const bool ok = wy >= 0 && wy < H && wx0 + 4 >= 0;
      pf_win = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
          xr, ok ? (((32 + tid / WR) * H + wy) * W + max(wx0, 0)) * 4 : img_bytes, 0, 0));
    }
    if (!PLAIN && c == NCH - 6 && a.residual) {
      const int yy = min(y0 + (tid & 7), H - 1), co2 = min(tid >> 3, a.Co2 - 1);
      pf_res = a.residual[((long)(n * a.Co2 + co2) * H + yy) * W + x0];
    }
    tap(g, k, cur, s, g + 1 < NPH && k == K - 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of A(c+1) landed ...
    if (!(dbg & 8)) __syncthreads();                 // ... and every other wave's
  };
  load_window(0);
  issue_a(0, sA0);
  load_pass(0, 0);
  // fully unrolled: every chunk's tap / group / pass arithmetic, DMA offsets and phase tests fold
  // at compile time (round 5: SALU per chunk roughly halved; tail alone 386-398 -> 372-377 us)
#pragma unroll
  for (int c = 0; c < NCH - 1; c += 2) {
    step(c, sA0, sA1);
    step(c + 1, sA1, sA0);
  }
  if constexpr (NCH % 2) step(NCH - 1, sA0, sA1);
  asm volatile("" ::"v"(pf_res));

  if constexpr (PLAIN) {
    // ---- op-level DCN: act(post_scale * (acc + bias) + post_shift) -> LDS [co][px] -> NCHW rows
    // (the window is free: every wave passed the last chunk's barrier)
    float *sO = reinterpret_cast<float *>(sWin);
    constexpr int CH = CT < 64 ? CT : 64;  // channels per pass through the LDS tile
#pragma unroll
    for (int h0 = 0; h0 < CT; h0 += CH) {
      if (h0) __syncthreads();  // the previous pass's rows are stored
#pragma unroll
      for (int m = h0 / 16; m < (h0 + CH) / 16; ++m) {
        const int co = 16 * m + 4 * kr;
        const f32x4 bs = a.bias ? *reinterpret_cast<const f32x4 *>(a.bias + co) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 sc = a.post_scale ? *reinterpret_cast<const f32x4 *>(a.post_scale + co) : f32x4{1.f, 1.f, 1.f, 1.f};
        const f32x4 sh = a.post_scale ? *reinterpret_cast<const f32x4 *>(a.post_shift + co) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sO[(co - h0 + r) * OP + wave * 16 + jj] = act_f((acc[m][r] + bs[r]) * sc[r] + sh[r], a.act);
      }
      __syncthreads();
      constexpr int EPP = CH * TR * (TC / 4) / NT;  // 4-pixel items per thread
#pragma unroll
      for (int i = 0; i < EPP; ++i) {
        const int e = tid + NT * i, co = e >> 5, qi = e & 31, yy = y0 + (qi >> 2), xx = x0 + 4 * (qi & 3);
        if (yy < H && xx < W)
          *reinterpret_cast<f32x4 *>(a.out + ((long)(n * CT + h0 + co) * H + yy) * W + xx) =
              *reinterpret_cast<const f32x4 *>(sO + co * OP + (qi >> 2) * 16 + 4 * (qi & 3));
      }
    }
    return;
  }

  // ---- epilogue items (4 pixels x 1 channel): addresses, bias and identity loads, issued before
  // the conv3 tail so their latency overlaps its weight DMA and MFMAs
  constexpr int EPT = CT * TR * (TC / 4) / NT;  // items per thread
  const int Co2 = a.Co2;
  f32x4 er[EPT];
  float eb[EPT];
  unsigned eo[EPT];  // byte offset of the item in image n's [Co2][H][W] planes
  bool eok[EPT];
  const bool res = a.residual && !(dbg & 16), csa = a.csa_out && !(dbg & 16);
  // buffer resources over image n's planes (SGPRs) and 32-bit byte offsets per item (round 6: a
  // 64-bit plane product and pointer per access, as the conv engine's epilogue had before round 5)
  const long img2 = (long)n * Co2 * P, img_b = (long)Co2 * P * 4;
  const brsrc_t ro = opt_rsrc(a.out, a.x, img2, img_b);
  const brsrc_t rcs = opt_rsrc(a.csa_out, a.x, img2, img_b);
  const brsrc_t rre = opt_rsrc(a.residual, a.x, img2, img_b);
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int e = tid + NT * i, co2 = e >> 5, qi = e & 31, yy = y0 + (qi >> 2), xx = x0 + 4 * (qi & 3);
    eok[i] = co2 < Co2 && yy < H && xx < W;
    eo[i] = 4u * (unsigned)(co2 * P + yy * W + xx);
    if (!eok[i]) continue;
    eb[i] = a.tail_b ? a.tail_b[co2] : 0.f;
    if (res) er[i] = buf_ld4(rre, eo[i]);
  }

  // ---- tail: BN2 + act -> conv3 (pointwise, split-bf16) ----------------------------------------
  // conv3's A fragments (24 KB, standard fragment order) by LDS-DMA into the two A slots: K chunk
  // h2 = 0 (pieces 0-11) into sA0, h2 = 1 into sA1.
  {
    const char *src = reinterpret_cast<const char *>(a.tail_wsplit) + lane * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int pc = wave + 8 * r;  // NPH K chunks x NCO blocks x 3 pieces
      if (pc >= 3 * NCO * NPH) break;
      char *dst = pc < 3 * NCO ? sA0 + pc * 1024 : sA1 + (pc - 3 * NCO) * 1024;
      __builtin_amdgcn_global_load_lds((const void *)(src + pc * 1024), (lds_void *)dst, 16, 0, 0);
    }
  }
  // The accumulator of co block m holds channels 16m + 4kr + r of pixel jj: for the conv3 K chunk
  // h2 (channels 32h2..32h2+31) lane group kr supplies {32h2 + 4kr + r, 32h2 + 16 + 4kr + r}, a
  // permutation of the chunk's K index that the A fragments below are read in.
  bf16x8 B2[NPH][3];
#pragma unroll
  for (int h2 = 0; h2 < NPH; ++h2) {
    float v[8];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int m = 2 * h2 + half, co = 16 * m + 4 * kr;
      const f32x4 bs = a.bias ? *reinterpret_cast<const f32x4 *>(a.bias + co) : f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 sc = a.post_scale ? *reinterpret_cast<const f32x4 *>(a.post_scale + co) : f32x4{1.f, 1.f, 1.f, 1.f};
      const f32x4 sh = a.post_scale ? *reinterpret_cast<const f32x4 *>(a.post_shift + co) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * half + r] = act_f((acc[m][r] + bs[r]) * sc[r] + sh[r], a.act);
    }
    split8(v, B2[h2]);
  }
  f32x4 acc2[NCO];
#pragma unroll
  for (int m = 0; m < NCO; ++m) acc2[m] = f32x4{0.f, 0.f, 0.f, 0.f};
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-DMA landed ...
  __syncthreads();                                   // ... and every other wave's
  {
    // standard fragment (cc = h2, blk = m2, piece pc): lane l holds row 16 m2 + (l & 15), channels
    // 32 h2 + 8 (l >> 4) + 0..7.  Channels 32h2 + 4kr + 0..3 are lane (kr/2)*16 + jj, bytes
    // 8 (kr & 1); channels 32h2 + 16 + 4kr + 0..3 the same 32 lanes further.
    const int tl = (((kr >> 1) << 4) | jj) * 16 + 8 * (kr & 1);
#pragma unroll
    for (int m2 = 0; m2 < NCO; ++m2)
#pragma unroll
      for (int h2 = 0; h2 < NPH; ++h2) {
        bf16x8 A[3];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
          const char *f = (h2 ? sA1 : sA0) + tl + (m2 * 3 + pc) * 1024;
          const u32x2 lo = *reinterpret_cast<const u32x2 *>(f);
          const u32x2 hi = *reinterpret_cast<const u32x2 *>(f + 512);
          A[pc] = __builtin_bit_cast(bf16x8, u32x4{lo.x, lo.y, hi.x, hi.y});
        }
        acc2[m2] = mfma_split6(A, B2[h2], acc2[m2]);
      }
  }
  // ---- epilogue: tile -> LDS [co2][px] -> 16-byte row quads (+ bias, identity, act, CSA) ------
  float *sO = reinterpret_cast<float *>(sWin);
#pragma unroll
  for (int m2 = 0; m2 < NCO; ++m2)
#pragma unroll
    for (int r = 0; r < 4; ++r) sO[(16 * m2 + 4 * kr + r) * OP + wave * 16 + jj] = acc2[m2][r];
  __syncthreads();
  // post stage: its own instantiation (POST), so the common form keeps its register allocation
  constexpr bool post = POST && CT == 64;
  // every global load of the thread's items (the CSA terms' source segments; identity and bias
  // above) is issued before the first use: the item loop would otherwise pay one L2/HBM round
  // trip per item and term (the stores may alias the sources, so the compiler cannot hoist them)
  f32x4 ev[EPT], eu[EPT][2][2];
  // every item of a thread has the same 4-pixel quad (qi = tid & 31; NT is a multiple of 32): the
  // CSA source rows, segment start and row weights are computed once per thread (round 5: per
  // item and term, in both passes, before)
  const int qit = tid & 31, yyt = y0 + (qit >> 2), xxt = x0 + 4 * (qit & 3);
  unsigned urow0[2] = {0u, 0u}, urow1[2] = {0u, 0u}, uhw[2] = {0u, 0u};
  int us0[2] = {0, 0}, uiw[2] = {4, 4};
  float uh0[2] = {1.f, 1.f}, uh1[2] = {0.f, 0.f};
  brsrc_t ru[2] = {ro, ro};
  bool sfast = true;
  if (csa) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j >= a.num_up) break;
      const int ih = a.up_h[j], iw = a.up_w[j], r = a.up_r[j];
      ru[j] = buf_rsrc(a.up[j] + (long)n * Co2 * ih * iw, (long)Co2 * ih * iw * 4);
      uhw[j] = 4u * (unsigned)(ih * iw);
      uiw[j] = iw;
      // PyTorch's area_pixel_compute_scale (ih / H) and source row, align_corners=False
      float hr = ((float)ih / (float)H) * ((float)yyt + 0.5f) - 0.5f;
      hr = hr < 0.f ? 0.f : hr;
      const int h1 = (int)hr, h1p = h1 < ih - 1 ? 1 : 0;
      urow0[j] = 4u * (unsigned)(h1 * iw);
      urow1[j] = 4u * (unsigned)((h1 + h1p) * iw);
      us0[j] = r == 2 ? 2 * (xxt >> 2) - 1 : (xxt >> 2) - 1;
      sfast = sfast && us0[j] >= 0 && us0[j] + 3 <= iw - 1;
      uh1[j] = hr - (float)h1;
      uh0[j] = 1.f - uh1[j];
    }
  }
  // the image-edge quads read clamped columns: a wave with one takes the per-column loads
  const bool wfast = __all(sfast || !(yyt < H && xxt < W));
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const int e = tid + NT * i, co2 = e >> 5, qi = e & 31;
    ev[i] = *reinterpret_cast<const f32x4 *>(sO + co2 * OP + (qi >> 2) * 16 + 4 * (qi & 3));
    if (!eok[i]) continue;
    if (csa) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j >= a.num_up) break;
        const unsigned pl = (unsigned)co2 * uhw[j];
        eu[i][j][0] = buf_seg(ru[j], pl + urow0[j], us0[j], uiw[j], wfast);
        eu[i][j][1] = buf_seg(ru[j], pl + urow1[j], us0[j], uiw[j], wfast);
      }
    }
  }
  // post stage (next pointwise conv): its A fragments into the A slots, free since the conv3 MFMAs
  // (every wave passed the barrier before the item loops).  Issued here, after the items' loads:
  // issued before them it raised the register pressure into main-loop spills
  if (post) {
    const char *src = reinterpret_cast<const char *>(a.post_wsplit) + lane * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int pc = wave + 8 * r;  // 2 K chunks x 4 co blocks x 3 pieces
      char *dst = pc < 12 ? sA0 + pc * 1024 : sA1 + (pc - 12) * 1024;
      __builtin_amdgcn_global_load_lds((const void *)(src + pc * 1024), (lds_void *)dst, 16, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    if (!eok[i]) continue;
    if (dbg & 16) {  // no epilogue traffic (keeps the work alive)
      if (ev[i][0] == 12345.f) buf_st4(ro, eo[i], ev[i]);
      continue;
    }
    const int e = tid + NT * i, qi = e & 31;
    f32x4 v = ev[i];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float t = v[u] + eb[i];
      if (res) t += er[i][u];
      v[u] = act_f(t, a.tail_act);
    }
    if (!post || !a.post_skip) buf_st4(ro, eo[i], v);
    if (csa) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j >= a.num_up) break;
        v += uh0[j] * hlerp(eu[i][j][0], a.up_r[j]) + uh1[j] * hlerp(eu[i][j][1], a.up_r[j]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = act_f(v[u], a.csa_act);
      if (!post || !a.post_skip) buf_st4(rcs, eo[i], v);
    }
    if (post)  // the branch output back into the item's own slot: the post stage's B operand
      *reinterpret_cast<f32x4 *>(sO + (e >> 5) * OP + (qi >> 2) * 16 + 4 * (qi & 3)) = v;
  }
  if constexpr (!post) return;

  // ---- post stage: next pointwise conv (+ act) -> NHWC, or final_conv -> soft-argmin ---------
  // B of lane (kr, jj): channels {32h2 + 4kr + r, 32h2 + 16 + 4kr + r} of pixel (wave, jj), the
  // conv3 K permutation (rows 4kr apart: 4 OP = 16 mod 32 banks, conflict-free)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's post-weight DMA landed ...
  __syncthreads();                                   // ... every wave's, and every v slot written
  // lane and pixel coordinates recomputed here (the asm hides tid from CSE): kept live from the
  // prologue, they raised the main loop's register pressure into spills
  int ptid = threadIdx.x;
  asm volatile("" : "+v"(ptid));
  const int plane_ = ptid & 63, pwave = __builtin_amdgcn_readfirstlane(ptid >> 6);
  const int pkr = plane_ >> 4, pjj = plane_ & 15;
  int pn, ppy, ppx;
  {
    const int tx2 = (W + TC - 1) / TC, nt2 = tx2 * ((H + TR - 1) / TR);
    const int nwg2 = gridDim.x, bb = blockIdx.x, q82 = nwg2 >> 3, r82 = nwg2 & 7, xc2 = bb & 7;
    const int bid2 = (xc2 < r82 ? xc2 * (q82 + 1) : r82 * (q82 + 1) + (xc2 - r82) * q82) + (bb >> 3);
    const int t2 = bid2 % nt2;
    pn = bid2 / nt2;
    ppy = (t2 / tx2) * TR + pwave;
    ppx = (t2 % tx2) * TC + pjj;
  }
  const bool ppv = ppy < H && ppx < W;
  bf16x8 B3[2][3];
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2) {
    float v[8];
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * half + r] = sO[(32 * h2 + 16 * half + 4 * pkr + r) * OP + pwave * 16 + pjj];
    split8(v, B3[h2]);
  }
  f32x4 acc3[4];
  {
    const int tl = (((pkr >> 1) << 4) | pjj) * 16 + 8 * (pkr & 1);
#pragma unroll
    for (int m3 = 0; m3 < 4; ++m3) {
      acc3[m3] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        bf16x8 A[3];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
          const char *f = (h2 ? sA1 : sA0) + tl + (m3 * 3 + pc) * 1024;
          const u32x2 lo = *reinterpret_cast<const u32x2 *>(f);
          const u32x2 hi = *reinterpret_cast<const u32x2 *>(f + 512);
          A[pc] = __builtin_bit_cast(bf16x8, u32x4{lo.x, lo.y, hi.x, hi.y});
        }
        acc3[m3] = mfma_split6(A, B3[h2], acc3[m3]);
      }
    }
  }
  // acc3[m3][r]: output channel 16 m3 + 4 pkr + r of pixel (ppy, ppx)
#pragma unroll
  for (int m3 = 0; m3 < 4; ++m3) {
    const f32x4 pb = a.post_b ? *reinterpret_cast<const f32x4 *>(a.post_b + 16 * m3 + 4 * pkr)
                              : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) acc3[m3][r] = act_f(acc3[m3][r] + pb[r], a.post_act);
  }
  if (a.post_out && ppv) {
    float *po = a.post_out + ((long)(pn * H + ppy) * W + ppx) * 64 + 4 * pkr;
#pragma unroll
    for (int m3 = 0; m3 < 4; ++m3) *reinterpret_cast<f32x4 *>(po + 16 * m3) = acc3[m3];
  }
  if (a.post_disp) {
    // soft-argmin over the 64 channels of the pixel (nets/estimation.ppy:13-30, similarity form):
    // the four lanes pjj, pjj+16, pjj+32, pjj+48 hold 16 channels each
    float mx = acc3[0][0];
#pragma unroll
    for (int m3 = 0; m3 < 4; ++m3)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc3[m3][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float z = 0.f, sacc = 0.f;
#pragma unroll
    for (int m3 = 0; m3 < 4; ++m3)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ev = __expf(acc3[m3][r] - mx);
        z += ev;
        sacc += ev * (float)(16 * m3 + 4 * pkr + r);
      }
    z += __shfl_xor(z, 16);
    sacc += __shfl_xor(sacc, 16);
    z += __shfl_xor(z, 32);
    sacc += __shfl_xor(sacc, 32);
    if (pkr == 0 && ppv) a.post_disp[(long)(pn * H + ppy) * W + ppx] = sacc / z;
  }

}

}  // namespace

int dcn_tile_supported(int c, int co, int co2, int kh, int kw, int stride, int pad, int dil,
                       int dg, int groups, int w) {
  return (c == 64 || c == 32 || c == 128) && co == c && co2 == c && kh == 3 && kw == 3 &&
         stride == 1 && pad == dil && dil == 2 && dg == 2 && groups == 1 && w % 4 == 0;
}

int dcn_tile_launch(const DcnTileArgs &a, hipStream_t stream) {
  if (!dcn_tile_supported(a.C, a.Co, a.plain ? a.Co : a.Co2, 3, 3, 1, a.dil, a.dil, a.dg, 1, a.W))
    return AANET_EUNSUPPORTED;
  if (a.plain && (a.post_wsplit || a.csa_out || a.residual)) return AANET_EINVAL;
  if (!a.x || !a.offset || !a.mask || !a.wsplit || (!a.plain && !a.tail_wsplit) || !a.out)
    return AANET_EINVAL;
  if (a.post_scale && !a.post_shift) return AANET_EINVAL;
  if (a.csa_out) {
    if (a.num_up < 0 || a.num_up > 2) return AANET_EUNSUPPORTED;
    for (int j = 0; j < a.num_up; ++j) {
      const int r = a.up_r[j];
      if (!a.up[j] || (r != 2 && r != 4) || a.up_h[j] * r != a.H || a.up_w[j] * r != a.W)
        return AANET_EUNSUPPORTED;
    }
  }
  const long P = (long)a.H * a.W;
  // 32-bit buffer offsets: one image of x, and the offset/mask planes of one image
  if ((long)a.C * P * 4 >= (1L << 31) || (long)(2 * a.dg * 27) * P * 4 >= (1L << 31))
    return AANET_EUNSUPPORTED;
  const long tiles = (long)host_div_up(a.W, TC) * host_div_up(a.H, TR);
  // timing-attribution switches (skip MFMAs / barriers / loads / the epilogue: WRONG results) are
  // read only in a debug build (make AANET_DEBUG=1); the product library always runs the kernel
#ifdef AANET_DEBUG_SWITCHES
  static const int dbg = [] {
    const char *e = getenv("AANET_DCN_DBG");
    const int v = e ? atoi(e) : 0;
    if (v) fprintf(stderr, "aanet: AANET_DCN_DBG=%d -- timing build, outputs are INVALID\n", v);
    return v;
  }();
#else
  constexpr int dbg = 0;
#endif
  DcnTileArgs b = a;
  b.dbg = dbg;
  if (a.post_wsplit && a.C != 64) return AANET_EUNSUPPORTED;
  const dim3 grid((unsigned)(a.N * tiles));
  if (a.C == 128 && !a.plain) return AANET_EUNSUPPORTED;  // 64-channel groups: op-level form only
  if (a.plain) {
    if (a.C == 128 && a.x_nchw)
      hipLaunchKernelGGL((dcn_tile_kernel<2, 64, false, true, true>), grid, dim3(NT), 0, stream, b);
    else if (a.C == 128)
      hipLaunchKernelGGL((dcn_tile_kernel<2, 64, false, false, true>), grid, dim3(NT), 0, stream, b);
    else if (a.C == 64 && a.x_nchw)
      hipLaunchKernelGGL((dcn_tile_kernel<2, 32, false, true, true>), grid, dim3(NT), 0, stream, b);
    else if (a.C == 64)
      hipLaunchKernelGGL((dcn_tile_kernel<2, 32, false, false, true>), grid, dim3(NT), 0, stream, b);
    else if (a.x_nchw)
      hipLaunchKernelGGL((dcn_tile_kernel<2, 16, false, true, true>), grid, dim3(NT), 0, stream, b);
    else
      hipLaunchKernelGGL((dcn_tile_kernel<2, 16, false, false, true>), grid, dim3(NT), 0, stream, b);
    return aanet_launch_status();
  }
  if (a.x_nchw) return AANET_EUNSUPPORTED;  // the bottleneck tail reads conv1's NHWC output
  if (a.C == 64 && a.post_wsplit)
    hipLaunchKernelGGL((dcn_tile_kernel<2, 32, true>), dim3((unsigned)(a.N * tiles)), dim3(NT), 0, stream, b);
  else if (a.C == 64)
    hipLaunchKernelGGL((dcn_tile_kernel<2, 32, false>), dim3((unsigned)(a.N * tiles)), dim3(NT), 0, stream, b);
  else
    hipLaunchKernelGGL((dcn_tile_kernel<2, 16, false>), dim3((unsigned)(a.N * tiles)), dim3(NT), 0, stream, b);
  return aanet_launch_status();
}
