// mdcn.hip -- the implicit-GEMM convolution engine for gfx950 (conv_fwd_kernel: MODE 0 plain
// convolution, MODE 1 modulated deformable convolution, DCNv2), its plan (conv_engine_plan) and
// dispatch (launch_fwd*), the weight packers, the forward C entry points and the two debug
// kernels.  MODE 1 replaces nets/deform_conv/src/deform_conv_cuda.cpp:490-685 and
// deform_conv_cuda_kernel.cu:467-866 (modulated kernels only; AANet never uses DCNv1).  The
// training backward is mdcn_bwd.hip; what the two share is mdcn_common.h.
#include "mdcn_common.h"
#include "dcn_small.h"
#include "dcn_tile.h"
#include "pointwise.h"
#include "small_conv.h"

namespace {

using namespace mdcn;  // NT, PT, KC, CP

__device__ __forceinline__ float apply_act(float v, int act) { return act_f(v, act); }

// ------------------------------------------------------------------------ forward -------
// Implicit-GEMM convolution engine.  MODE 1: modulated deformable (bilinear sampler, the DCN);
// MODE 0: plain convolution (one tap per input element; every other conv of the ISA/CSA
// blocks: 1x1, 3x3, dilated, grouped, strided).
//
// Workgroup = 512 threads (FNT), output tile CO_T channels x PTT pixels of one image.  The K
// dimension is walked in chunks of (<= 32 input channels of one deformable group, tap k),
// taps innermost so a chunk's 32 channel planes stay L2-resident across its 9 taps:
//   stage   : each thread builds PTT*32/512 im2col values of the chunk for ONE pixel -> LDS
//             [pixel][channel]; the sampling state of a (pixel, tap, group) is computed once.
//             Gathers are buffer loads: per-lane 32-bit offset (the tap position) + wave-uniform
//             SGPR offset (the channel plane), so a gather costs no address VALU; the plain
//             conv's zero padding comes from the buffer range check (offset past the image).
//             The weight slice -> LDS [co][channel].
//   contract: wave w owns (CO_T/WC) x (PTT/WP) outputs; per 16 channels one ds_read_b128 per 16-row
//             operand block, then 4 k-steps of v_mfma_f32_16x16x4_f32 -- the reduction index
//             is permuted (lane group kr takes channels 4kr..4kr+3) identically for both operands.
// Software pipeline: LDS double buffer; while the MFMAs of chunk c run, the global loads of
// chunk c+1 are in flight in registers and the offsets/mask of chunk c+2 are being fetched;
// one barrier per chunk.  Blocks are remapped so each XCD gets a contiguous range of tiles
// (neighbouring tiles share input rows -> same L2).
// Epilogue: the tile is transposed through LDS and written as 16-byte row segments:
// y = act(post_scale*(acc + bias) + post_shift + residual).
// grid: x = N * ceil(P/PTT), y = groups * ceil(Cog/CO_T).
constexpr int FNT = 512;  // forward conv engine: 8 waves = 2 (output channels) x 4 (pixels)
constexpr int SP = 40;  // LDS row pitch (floats) of both staging tiles: conflict-free b128 reads

typedef int i2v __attribute__((ext_vector_type(2)));

// K chunk = (tap k, channels [c0, c1)); chunks of ck channels, cut at deformable-group
// boundaries when `cut` (a chunk that spans groups carries one sampling state per group).
template <int CK>
struct ChunkIt {
  int k, c0, c1;
  __device__ __forceinline__ static int next_end(int c0, int cend, int cpg, int cut) {
    int e = min(c0 + CK, cend);
    if (cut) e = min(e, (c0 / cpg + 1) * cpg);
    return e;
  }
  __device__ __forceinline__ void first(int cbeg, int cend, int cpg, int cut) {
    k = 0;
    c0 = cbeg;
    c1 = next_end(cbeg, cend, cpg, cut);
  }
  __device__ __forceinline__ void advance(int K, int cend, int cpg, int cut) {
    if (++k == K) {
      k = 0;
      c0 = c1;
      c1 = next_end(c0, cend, cpg, cut);
    }
  }
};

// Pair-gather sampling state with the corner selection and the modulation mask folded into the
// weights: val = (wa_t*t.x + wa_b*b.x) + (wb_t*t.y + wb_b*b.y), evaluated with two packed-fp32
// ops and one add (kernel.cu:494-496 computes the same sum in another order: the values agree
// to rounding; the sampling positions and corner indices are bit-exact).  f32 MFMA and VALU
// never co-issue on gfx950, so every VALU op here is taken from the matrix pipe.
typedef float f2v __attribute__((ext_vector_type(2)));
struct SampW {
  int ot, ob;  // byte offsets of the 2-wide pairs in rows hl, hl+1
  f2v wt, wb;  // (wa_t, wb_t) * m, (wa_b, wb_b) * m
};

__device__ __forceinline__ void make_sampw(SampW &s, float h, float w, int H, int W, float m) {
#pragma clang fp contract(off)
  const bool valid = h > -1.f && w > -1.f && h < (float)H && w < (float)W;
  const int hl = (int)floorf(h), wl = (int)floorf(w);
  const float lh = h - (float)hl, lw = w - (float)wl;
  const float hh = 1.f - lh, hw = 1.f - lw;
  const bool ok1 = valid && hl >= 0 && wl >= 0;
  const bool ok2 = valid && hl >= 0 && wl + 1 <= W - 1;
  const bool ok3 = valid && hl + 1 <= H - 1 && wl >= 0;
  const bool ok4 = valid && hl + 1 <= H - 1 && wl + 1 <= W - 1;
  const float w1 = ok1 ? hh * hw : 0.f, w2 = ok2 ? hh * lw : 0.f;
  const float w3 = ok3 ? lh * hw : 0.f, w4 = ok4 ? lh * lw : 0.f;
  const int pb = valid ? min(max(wl, 0), W - 2) : 0;
  const int rt = valid ? min(max(hl, 0), H - 1) : 0;
  const int rb = valid ? min(max(hl + 1, 0), H - 1) : 0;
  s.ot = (rt * W + pb) * 4;
  s.ob = (rb * W + pb) * 4;
  const bool swap = valid && pb != wl;  // wl == -1: pair = (wl+1, wl+2); wl == W-1: (wl-1, wl)
  const bool left = wl < pb;             // wl == -1
  const float wat = swap ? (left ? w2 : 0.f) : w1;
  const float wbt = swap ? (left ? 0.f : w1) : w2;
  const float wab = swap ? (left ? w4 : 0.f) : w3;
  const float wbb = swap ? (left ? 0.f : w3) : w4;
  s.wt = f2v{wat, wbt} * m;
  s.wb = f2v{wab, wbb} * m;
}

// NHWC sampling state: byte offsets of the 4 corners (`oob` for an invalid corner: the buffer
// range check reads it as 0) and their weights with the mask folded in.  Same validity rules
// and corner indices as make_samp (kernel.cu:467-497).
__device__ __forceinline__ void make_samp4(int o[4], f32x4 &wv, float h, float w, int H, int W,
                                           int rowb, int oob, float m) {
#pragma clang fp contract(off)
  const bool valid = h > -1.f && w > -1.f && h < (float)H && w < (float)W;
  const int hl = (int)floorf(h), wl = (int)floorf(w);
  const float lh = h - (float)hl, lw = w - (float)wl;
  const float hh = 1.f - lh, hw = 1.f - lw;
  const bool ok1 = valid && hl >= 0 && wl >= 0;
  const bool ok2 = valid && hl >= 0 && wl + 1 <= W - 1;
  const bool ok3 = valid && hl + 1 <= H - 1 && wl >= 0;
  const bool ok4 = valid && hl + 1 <= H - 1 && wl + 1 <= W - 1;
  wv = f32x4{ok1 ? hh * hw : 0.f, ok2 ? hh * lw : 0.f, ok3 ? lh * hw : 0.f, ok4 ? lh * lw : 0.f} * m;
  o[0] = ok1 ? (hl * W + wl) * rowb : oob;
  o[1] = ok2 ? (hl * W + wl + 1) * rowb : oob;
  o[2] = ok3 ? ((hl + 1) * W + wl) * rowb : oob;
  o[3] = ok4 ? ((hl + 1) * W + wl + 1) * rowb : oob;
}

// ---- split-bf16 contraction (PREC 1; split.h) -------------------------------------------------
// Activations are split two values at a time by common.h split_pair (x = h + m + l exactly).
__device__ __forceinline__ void split3(f32x4 v, bf16x4 &h, bf16x4 &m, bf16x4 &l) {
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  u32x2 hh, mm, ll;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    unsigned a, b, c;
    split_pair(v[2 * i], v[2 * i + 1], a, b, c);
    hh[i] = a;
    mm[i] = b;
    ll[i] = c;
  }
  h = __builtin_bit_cast(bf16x4, hh);
  m = __builtin_bit_cast(bf16x4, mm);
  l = __builtin_bit_cast(bf16x4, ll);
}

// Element offset of (row, 16-byte quad q8) in a [rows][32] bf16 piece plane.  Four 64-byte rows
// fill the 256-byte bank row; quads are XOR-swizzled by bit 2 of the row (q8 ^ 2 on rows 4-7 of
// every 8).  An MFMA operand read (ds_read_b128, lane (kr, jj) = quad kr of row base + jj) is
// serviced in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32):
// MI355X_MICROARCH.md §LDS), and with this swizzle every group hits 16 distinct 16-byte bank
// quads for ANY base row (the halo taps' shifts included); the previous row>>2 & 3 swizzle was
// conflict-free for 16 lanes at one quad, which is not how the hardware groups them (2-way
// conflicts on most reads: SQ_LDS_BANK_CONFLICT 31-41 % of the LDS cycles of the halo kernels).
__device__ __forceinline__ int swz(int row, int q8) { return row * 32 + ((q8 ^ (((row >> 2) & 1) << 1)) << 3); }

// channels 4*q4 .. 4*q4+3 of one row, as its three pieces (planes `pe` elements apart)
// The tail kernels' B staging (PAIRED: lanes write whole 16-byte quads, ds_write_b128 in lane
// groups of 8 consecutive lanes = 8 consecutive rows at one quad): quads XOR-swizzled by bits 1-2
// of the row, so those 8 lanes hit 8 distinct 16-byte bank slots, and the MFMA operand reads
// (lane groups as in swz) still hit 16 distinct ones (checked for every base row % 16 == 0).
__device__ __forceinline__ int swz_tail(int row, int q8) { return row * 32 + ((q8 ^ ((row >> 1) & 3)) << 3); }
// 8 values -> three bf16x8 pieces, the element-wise split of split3
__device__ __forceinline__ void split8_t(const float (&v)[8], bf16x8_t (&p)[3]) {
  bf16x4 h0, m0, l0, h1, m1, l1;
  split3(f32x4{v[0], v[1], v[2], v[3]}, h0, m0, l0);
  split3(f32x4{v[4], v[5], v[6], v[7]}, h1, m1, l1);
  p[0] = bf16x8_t{h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
  p[1] = bf16x8_t{m0[0], m0[1], m0[2], m0[3], m1[0], m1[1], m1[2], m1[3]};
  p[2] = bf16x8_t{l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
}

__device__ __forceinline__ void put_split(__bf16 *plane, int pe, int row, int q4, f32x4 v) {
  bf16x4 h, m, l;
  split3(v, h, m, l);
  const int o = swz(row, q4 >> 1) + ((q4 & 1) << 2);
  *reinterpret_cast<bf16x4 *>(plane + o) = h;
  *reinterpret_cast<bf16x4 *>(plane + pe + o) = m;
  *reinterpret_cast<bf16x4 *>(plane + 2 * pe + o) = l;
}

// FULL: every chunk holds KC channels (Cg % KC == 0, and cpg % KC == 0 for the DCN), so the
// staging code has no per-row guards.  Those guards are wave-uniform, and the compiler turns
// them into scalar branches, which split the loop body and defeat the MFMA/staging interleave.
// LAYOUT bit 0: input NHWC (channels-last; each staging item is one 16-byte load of 4 channels
// at one position, so a DCN corner or a conv tap of 32 channels is 8 lanes x 16 B = one 128-B
// line; needs FULL).  Bit 1: output NHWC.
// CFG: chunk shape.  0: 32 channels of one deformable group; 1: 16 channels (16-channel conv
// groups: the second MFMA half of a chunk is skipped); 2: 32 channels spanning two 16-channel
// deformable groups (one sampling state per (pixel, group)).
// HALO (plain 3x3, stride 1, pad = dil <= 2, NHWC input, PREC 1): the tile is 8 rows x 16
// columns of outputs; per 32-channel chunk its (8+2d) x (16+2d) input halo is loaded, split and
// stored to LDS ONCE, and all nine taps read their B operand from it at shifted positions (the
// im2col form stages, splits and synchronises once per tap).  The next chunk's halo is in flight
// in registers during the nine taps; A fragments are double-buffered across taps.
// POST (HALO 1/2 tails with the CSA epilogue, CO_T = Co2 = 64): the post stage of
// aanet_post_stage_t on the CSA output, NHWC out only (the next module's conv1).
template <int MODE, int CO_T, int PTT, int PACKED, int TAIL, int SCHED, int FULL, int LAYOUT,
          int CFG = 0, int PREC = 0, int HALO = 0, int POST = 0>
__global__ __launch_bounds__(FNT, 4) void conv_fwd_kernel(MdcnArgs a) {
  constexpr int CK = CFG == 1 ? 16 : 32;   // channels per K chunk
  constexpr int GPC = CFG == 2 ? 2 : 1;    // deformable groups per chunk
  constexpr int WC = CO_T >= 32 ? 2 : 1;   // waves along the output channels
  constexpr int WP = FNT / 64 / WC;        // waves along the pixels
  constexpr int NCB = CO_T / 16 / WC;      // 16-row output-channel blocks per wave
  constexpr int NPB = PTT / 16 / WP;       // 16-col pixel blocks per wave
  constexpr int CPT = CK * PTT / FNT;      // im2col values staged per thread per chunk
  constexpr int WPT = CK * CO_T / FNT;     // weights staged per thread per chunk
  static_assert(NCB >= 1 && NPB >= 1 && WPT >= 1 && CPT % 4 == 0, "tile shape");
  static_assert(CFG == 0 || FULL, "chunk configurations 1/2 need full chunks");
  constexpr bool INH = (LAYOUT & 1) != 0, ONH = (LAYOUT & 2) != 0;
  constexpr int NIT = INH ? PTT * (CK / 4) / FNT : 1;  // NHWC staging items per thread
  static_assert(!INH || (FULL && NIT >= 1 && FNT % (CK / 4) == 0), "NHWC staging needs full chunks");
  static_assert(!(ONH && TAIL), "NHWC output with a pointwise tail is not instantiated");
  // PREC 1 (split-bf16 contraction, see split4 / SplitLds): both operand tiles as three bf16
  // piece planes of 32-channel rows, 64 B per row (XOR-swizzled 16-byte quads, no padding)
  constexpr bool SPL = PREC == 1;
  // (partial chunks: plain NCHW convs whose group width is a multiple of 16 but not 32 -- the
  // zero-padded split pack, rows past the group staged as zeros)
  static_assert(!SPL || (CK == 32 && (FULL || (MODE == 0 && !INH && !TAIL)) && PACKED && CO_T >= 32),
                "split-bf16 configuration");
  constexpr int BUF = SPL ? PTT * 48 : (PTT + CO_T) * SP; // floats per LDS buffer
  constexpr int OP = PTT + 4;            // epilogue tile pitch
  static_assert(CO_T * OP <= 2 * BUF, "epilogue tile must fit the staging buffers");
  // DCN: the sampling state of a (pixel, tap, deformable group) is computed once, by the threads
  // tid < GPC*PTT (group gi = tid / PTT of the chunk), and published through a double-buffered
  // LDS slot to the threads that stage channels of that pixel and group (the VALU it saves is
  // matrix-pipe time).
  constexpr int PSLOT = GPC * PTT * 8;
  __shared__ __attribute__((aligned(16))) float smem[2 * BUF + (MODE ? 2 * PSLOT : 0)];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool pwave = __builtin_amdgcn_readfirstlane(wave) < GPC * PTT / 64;  // tid < GPC*PTT
  const int pgi = MODE ? __builtin_amdgcn_readfirstlane(wave / (PTT / 64)) : 0;  // param group
  const int wc0 = __builtin_amdgcn_readfirstlane((wave / WP) * NCB);  // first co block of the wave
  const int wp0 = __builtin_amdgcn_readfirstlane((wave % WP) * NPB);  // first px block of the wave
  const long P = (long)a.Ho * a.Wo;
  static_assert(!HALO || (MODE == 0 && PREC == 1 && (HALO <= 2 || HALO == 4) && PTT == 128 && (LAYOUT & 1)),
                "halo configuration");
  // HALO 4: the phase-strided halo tile.  A 3x3 conv of dilation D (= pad, stride 1) is D x D
  // independent dilation-1 convs, one per phase (pixels y % D = pa, x % D = pb): the tile is
  // 8 x 16 outputs of one phase, its halo the (8+2) x (16+2) phase positions around them, so
  // dilations 4 / 8 (nets/refinement.py:60-106) stage 1.4 positions per output instead of the
  // (8+2D)(16+2D)/128 of a plain halo or the nine of im2col.  NHWC in and out only.
  constexpr bool PH = HALO == 4;
  static_assert(!PH || (LAYOUT == 3 && !TAIL && !POST), "phase-strided halo: NHWC in/out, no tail");
  constexpr int TRH = 8;  // output rows of a halo tile (16 columns)
  const int pd = PH ? a.dil : 1;                       // phase stride
  const int hWo = PH ? (a.Wo + pd - 1) / pd : a.Wo;    // (largest) phase image size
  const int hHo = PH ? (a.Ho + pd - 1) / pd : a.Ho;
  const int htx = HALO ? (hWo + 15) / 16 : 1;
  const int hty = HALO ? (hHo + TRH - 1) / TRH : 1;
  const int ntiles = HALO ? pd * pd * htx * hty : (int)((P + PTT - 1) / PTT);
  // XCD-aware remap of the pixel-tile index (bijective for any grid size)
  const int nwg = gridDim.x, b0 = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = b0 & 7;
  const int bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b0 >> 3);
  const int n = bid / ntiles, tile0 = bid % ntiles;
  const int ph = PH ? tile0 / (htx * hty) : 0, tile = PH ? tile0 - ph * (htx * hty) : tile0;
  const int pa = PH ? ph / pd : 0, pb = PH ? ph - pa * pd : 0;  // the tile's phase
  // HALO tile origin (phase coordinates for HALO 4: image row pa + pd * y)
  const int hy0 = HALO ? (tile / htx) * TRH : 0, hx0 = HALO ? (tile % htx) * 16 : 0;
  const int Cg = a.C / a.groups, Cog = a.Co / a.groups, K = a.kh * a.kw, cpg = a.C / a.dg;
  const int ncot = (Cog + CO_T - 1) / CO_T;
  const int gc = blockIdx.y / ncot, cot = blockIdx.y % ncot;
  const int co0 = gc * Cog + cot * CO_T, co_end = min(co0 + CO_T, (gc + 1) * Cog);
  const int cbeg = gc * Cg, cend = (gc + 1) * Cg;
  const long HW = (long)a.H * a.W;
  const int img_bytes = (int)(a.C * HW * 4);
  const auto xr = __builtin_amdgcn_make_buffer_rsrc((void *)(a.x + (long)n * a.C * HW), (short)0,
                                                     img_bytes, 0x00020000);
  const int plane_bytes = (int)(HW * 4);

  // staging role: one pixel, CPT consecutive channels of the chunk (wave-uniform base)
  const int spx = tid % PTT;
  const int scb = __builtin_amdgcn_readfirstlane((tid / PTT) * CPT);
  const long p = (long)tile * PTT + spx;
  const bool pvalid = p < P;
  const int ho = pvalid ? (int)(p / a.Wo) : 0, wo = pvalid ? (int)(p % a.Wo) : 0;
  const long psafe = pvalid ? p : 0;
  // NHWC staging roles: lane quad nq = channels 4nq..4nq+3, pixels npx[i]
  const int nq = tid & (CK / 4 - 1);
  int npx[NIT], nho[NIT], nwo[NIT];
  bool nval[NIT];
#pragma unroll
  for (int i = 0; i < NIT; ++i) {
    npx[i] = tid / (CK / 4) + (FNT / (CK / 4)) * i;
    const long pp = (long)tile * PTT + npx[i];
    nval[i] = pp < P;
    nho[i] = nval[i] ? (int)(pp / a.Wo) : 0;
    nwo[i] = nval[i] ? (int)(pp % a.Wo) : 0;
  }
  f32x4 nv[INH && MODE == 0 ? NIT : 1];        // conv tap values (NHWC)
  f32x4 nc[INH && MODE ? NIT : 1][4];          // DCN corner values (NHWC)
  int noff[INH && MODE ? NIT : 1][4];          // DCN corner byte offsets (NHWC)
  f32x4 nw[INH && MODE ? NIT : 1];             // DCN corner weights (mask folded)

  float wreg[WPT];
  float vraw[MODE ? 1 : CPT];
  i2v traw[MODE ? CPT : 1], braw[MODE ? CPT : 1];
  SampW snext;                                 // sampling state of the chunk being loaded
  float off_h = 0.f, off_w = 0.f, mlog = 0.f;  // raw offsets/mask of the chunk after it

  // offsets / mask / weights through buffer descriptors too: per-lane part fixed for the whole
  // kernel, chunk-dependent part in an SGPR.
  const auto offr = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(MODE ? a.offset + (long)n * a.off_bs : a.x), (short)0, 0x7ffffff0, 0x00020000);
  const auto mskr = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(MODE ? a.mask + (long)n * a.mask_bs : a.x), (short)0, 0x7ffffff0, 0x00020000);
  const int w_bytes = (int)((long)a.Co * Cg * K * 4);
  const auto wr = __builtin_amdgcn_make_buffer_rsrc((void *)a.weight, (short)0, w_bytes, 0x00020000);
  int wlane[WPT];  // per-lane weight byte offsets (chunk-invariant)
#pragma unroll
  for (int i = 0; i < WPT; ++i) {
    const int e = tid + FNT * i, co = e / CK, cl = e % CK;
    // rows past the chunk read a neighbouring channel (multiplied by a zero im2col value);
    // reads past the tensor are out of range -> 0; co past co_end is never stored
    wlane[i] = PACKED ? (co * Cg + cl) * 4 : (co * Cg * K + cl * K) * 4;
  }
  const int pl4 = (int)psafe * 4;
  // PREC 1: the wave's A fragments (its NCB 16-row blocks x 3 pieces) come from the pre-split
  // weight fragments in global memory (L2-resident), loaded one chunk ahead of their MFMAs
  bf16x8 fa[SPL ? NCB : 1][3];
  const int sT = (Cog + 63) / 64, sNCC = (Cg + 31) / 32;
  const int st64 = (cot * CO_T) / 64, sbb = ((cot * CO_T) % 64) / 16 + wc0;
  auto load_a = [&](const bf16x8 *frag, long tile_base) {
#pragma unroll
    for (int m = 0; m < NCB; ++m)
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) fa[m][pc] = frag[((tile_base + sbb + m) * 3 + pc) * 64 + lane];
  };
  auto load_a_chunk = [&](const ChunkIt<CK> &c) {
    load_a(a.wsplit, ((((long)gc * sT + st64) * K + c.k) * sNCC + ((c.c0 - cbeg) >> 5)) * 4);
  };

  auto load_params_raw = [&](const ChunkIt<CK> &c) {
    const int g = c.c0 / cpg + pgi;
    const int ob = __builtin_amdgcn_readfirstlane((int)(((long)g * 2 * K + 2 * c.k) * P * 4));
    const int mb = __builtin_amdgcn_readfirstlane((int)(((long)g * K + c.k) * P * 4));
    off_h = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(offr, pl4, ob, 0));
    off_w = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(offr, pl4, ob + (int)(P * 4), 0));
    mlog = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(mskr, pl4, mb, 0));
  };
  auto finish_params = [&](const ChunkIt<CK> &c, int slot) {
#pragma clang fp contract(off)
    const int i = c.k / a.kw, j = c.k % a.kw;
    float m = a.mask_logits ? a.mask_scale * __builtin_amdgcn_rcpf(1.f + __expf(-mlog)) : mlog;
    if (!pvalid) m = 0.f;
    const float h = (float)(ho * a.stride - a.pad + i * a.dil) + off_h;
    const float w = (float)(wo * a.stride - a.pad + j * a.dil) + off_w;
    float *d = smem + 2 * BUF + slot * PSLOT + (pgi * PTT + spx) * 8;
    if constexpr (INH) {
      int o[4];
      f32x4 wv;
      make_samp4(o, wv, h, w, a.H, a.W, a.C * 4, img_bytes, m);
      *reinterpret_cast<f32x4 *>(d) = f32x4{__builtin_bit_cast(float, o[0]), __builtin_bit_cast(float, o[1]),
                                            __builtin_bit_cast(float, o[2]), __builtin_bit_cast(float, o[3])};
      *reinterpret_cast<f32x4 *>(d + 4) = wv;
    } else {
      SampW sw;
      make_sampw(sw, h, w, a.H, a.W, m);
      *reinterpret_cast<f32x4 *>(d) = f32x4{__builtin_bit_cast(float, sw.ot),
                                            __builtin_bit_cast(float, sw.ob), sw.wt.x, sw.wt.y};
      *reinterpret_cast<f2v *>(d + 4) = sw.wb;
    }
  };
  auto get_params = [&](int slot) {
    if constexpr (INH) {
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        const int gi = GPC == 2 ? nq >> 2 : 0;  // 16-channel group of this lane's quad
        const float *d = smem + 2 * BUF + slot * PSLOT + (gi * PTT + npx[i]) * 8;
        const f32x4 q = *reinterpret_cast<const f32x4 *>(d);
        const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];  // see below
        noff[i][0] = __builtin_bit_cast(int, q0);
        noff[i][1] = __builtin_bit_cast(int, q1);
        noff[i][2] = __builtin_bit_cast(int, q2);
        noff[i][3] = __builtin_bit_cast(int, q3);
        nw[i] = *reinterpret_cast<const f32x4 *>(d + 4);
      }
      return;
    }
    const int gi = GPC == 2 ? scb >> 4 : 0;  // scb: multiple of CPT (8) -> one group per thread
    const float *d = smem + 2 * BUF + slot * PSLOT + (gi * PTT + spx) * 8;
    const f32x4 q = *reinterpret_cast<const f32x4 *>(d);
    // copy the elements to scalars first: __builtin_bit_cast of an ext-vector element lvalue
    // (q[1]) reads element 0 with this clang
    const float q0 = q[0], q1 = q[1];
    snext.ot = __builtin_bit_cast(int, q0);
    snext.ob = __builtin_bit_cast(int, q1);
    snext.wt = f2v{q[2], q[3]};
    snext.wb = *reinterpret_cast<const f2v *>(d + 4);
  };
  auto issue_loads = [&](const ChunkIt<CK> &c) {
    const int rows = c.c1 - c.c0;
    const int wbase = PACKED ? (((c.k * a.Co + co0) * Cg + (c.c0 - cbeg)) * 4)
                             : (((co0 * Cg + (c.c0 - cbeg)) * K + c.k) * 4);
    if constexpr (!SPL) {
#pragma unroll
      for (int i = 0; i < WPT; ++i)
        wreg[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wr, wlane[i], wbase, 0));
    }
    if constexpr (INH) {
      const int soff = __builtin_amdgcn_readfirstlane(c.c0 * 4);
      if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
          const int hi = nho[i] * a.stride - a.pad + (c.k / a.kw) * a.dil;
          const int wi = nwo[i] * a.stride - a.pad + (c.k % a.kw) * a.dil;
          const bool ok = nval[i] && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
          const int voff = ok ? (hi * a.W + wi) * (a.C * 4) + nq * 16 : img_bytes;
          nv[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, voff, soff, 0));
        }
      } else {
#pragma unroll
        for (int i = 0; i < NIT; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            nc[i][j] = __builtin_bit_cast(
                f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, noff[i][j] + nq * 16, soff, 0));
      }
      return;
    }
    const int cbase = __builtin_amdgcn_readfirstlane((c.c0 + scb) * plane_bytes);
    if (MODE == 0) {
      const int hi = ho * a.stride - a.pad + (c.k / a.kw) * a.dil;
      const int wi = wo * a.stride - a.pad + (c.k % a.kw) * a.dil;
      const bool ok = pvalid && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
      const int voff = ok ? (hi * a.W + wi) * 4 : img_bytes;  // past the end -> reads 0
#pragma unroll
      for (int e = 0; e < CPT; ++e) {
        const int soff = cbase + e * plane_bytes;
        vraw[e] = (FULL || scb + e < rows)
                      ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, voff, soff, 0))
                      : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < CPT; ++e) {
        const int soff = cbase + (FULL ? e : min(e, rows - 1 - scb)) * plane_bytes;
        traw[e] = __builtin_amdgcn_raw_buffer_load_b64(xr, snext.ot, soff, 0);
        braw[e] = __builtin_amdgcn_raw_buffer_load_b64(xr, snext.ob, soff, 0);
      }
    }
  };
  auto store_stage = [&](const ChunkIt<CK> &c, int buf) {
    float *sC = smem + buf * BUF, *sW = sC + PTT * SP;
    __bf16 *sB = reinterpret_cast<__bf16 *>(smem + buf * BUF);
    const int rows = c.c1 - c.c0;
    if constexpr (!SPL) {
#pragma unroll
      for (int i = 0; i < WPT; ++i) {
        const int e = tid + FNT * i;
        sW[(e / CK) * SP + e % CK] = wreg[i];
      }
    }
    if constexpr (INH) {
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        f32x4 v;
        if (MODE == 0) {
          v = nv[i];
        } else {
          // Bilinear blend of the 4 corner quads: ((c0 w0 + c1 w1) + c2 w2) + c3 w3 per channel,
          // as scalar v_mul/v_fma_f32 in asm.  The packed form the compiler picks for this
          // (v_pk_fma_f32 with a broadcast weight) gave non-reproducible results in the split
          // DCN tail kernel: pixels staged by lanes 48-63 read a stale broadcast weight register
          // written by the VALU instruction just before (tools/diag_race3.py).
          const float w0 = nw[i][0], w1 = nw[i][1], w2 = nw[i][2], w3 = nw[i][3];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            float t;
            asm("v_mul_f32 %0, %1, %2" : "=v"(t) : "v"(nc[i][0][u]), "v"(w0));
            asm("v_fma_f32 %0, %1, %2, %0" : "+v"(t) : "v"(nc[i][1][u]), "v"(w1));
            asm("v_fma_f32 %0, %1, %2, %0" : "+v"(t) : "v"(nc[i][2][u]), "v"(w2));
            asm("v_fma_f32 %0, %1, %2, %0" : "+v"(t) : "v"(nc[i][3][u]), "v"(w3));
            v[u] = t;
          }
        }
        if constexpr (SPL)
          put_split(sB, PTT * 32, npx[i], nq, v);
        else
          *reinterpret_cast<f32x4 *>(sC + npx[i] * SP + 4 * nq) = v;
      }
      return;
    }
    float v[CPT];
#pragma unroll
    for (int e = 0; e < CPT; ++e) {
      if (MODE == 0) {
        v[e] = vraw[e];
      } else {
        const f2v p = __builtin_elementwise_fma(snext.wb, __builtin_bit_cast(f2v, braw[e]),
                                                snext.wt * __builtin_bit_cast(f2v, traw[e]));
        float r;  // scalar add of the two halves (keeps the vectorizer from re-pairing them)
        asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(p.x), "v"(p.y));
        v[e] = (FULL || scb + e < rows) ? r : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < CPT / 4; ++q) {
      const f32x4 vq = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
      if constexpr (SPL)
        put_split(sB, PTT * 32, spx, scb / 4 + q, vq);
      else
        *reinterpret_cast<f32x4 *>(sC + spx * SP + scb + 4 * q) = vq;
    }
  };

  f32x4 acc[NCB][NPB];
#pragma unroll
  for (int m = 0; m < NCB; ++m)
#pragma unroll
    for (int b = 0; b < NPB; ++b) acc[m][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kr = lane >> 4, jj = lane & 15;
  constexpr int CUT = MODE && GPC == 1;  // chunks stop at deformable-group boundaries
  ChunkIt<CK> cur, nxt, nn;
  bool has_next = false;
  int slot = 1;  // parameter slot of `nxt`
  if constexpr (!HALO) {
  cur.first(cbeg, cend, cpg, CUT);
  if (MODE) {
    if (pwave) {
      load_params_raw(cur);
      finish_params(cur, 0);
    }
    __syncthreads();
    get_params(0);
  }
  issue_loads(cur);
  if constexpr (SPL) load_a_chunk(cur);
  store_stage(cur, 0);
  nxt = cur;
  nxt.advance(K, cend, cpg, CUT);
  has_next = nxt.c0 < cend;
  if (MODE && has_next && pwave) {
    load_params_raw(nxt);
    finish_params(nxt, 1);
  }
  __syncthreads();
  }

  struct Frag {
    f32x4 A[NCB], B[NPB];
  };
  auto read_frag = [&](int buf, int h, Frag &f) {
    const float *sC = smem + buf * BUF, *sW = sC + PTT * SP;
#pragma unroll
    for (int m = 0; m < NCB; ++m)
      f.A[m] = *reinterpret_cast<const f32x4 *>(sW + (16 * (wc0 + m) + jj) * SP + 16 * h + 4 * kr);
#pragma unroll
    for (int b = 0; b < NPB; ++b)
      f.B[b] = *reinterpret_cast<const f32x4 *>(sC + (16 * (wp0 + b) + jj) * SP + 16 * h + 4 * kr);
  };
  auto mma = [&](const Frag &f) {
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int m = 0; m < NCB; ++m)
#pragma unroll
        for (int b = 0; b < NPB; ++b) {
          acc[m][b] = mfma16x16x4(f.A[m][s4], f.B[b][s4], acc[m][b]);
        }
  };
  auto mfma_half = [&](int buf, int h) {
    Frag f;
    read_frag(buf, h, f);
    mma(f);
  };
  // PREC 1: the whole 32-channel chunk is one K step of v_mfma_f32_16x16x32_bf16 per piece pair.
  // A: the fragments in fa; B: read one 16-pixel block at a time (12 VGPRs live, not 24).
  auto mma_s = [&](int buf) {
    const __bf16 *sB = reinterpret_cast<const __bf16 *>(smem + buf * BUF);
#pragma unroll
    for (int b = 0; b < NPB; ++b) {
      bf16x8 fb[3];
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
        fb[pc] = *reinterpret_cast<const bf16x8 *>(sB + pc * PTT * 32 + swz(16 * (wp0 + b) + jj, kr));
#pragma unroll
      for (int m = 0; m < NCB; ++m) acc[m][b] = mfma_split6(fa[m], fb, acc[m][b]);
    }
  };
  auto mfma_chunk = [&](int buf) {
    if constexpr (SPL) {
      mma_s(buf);
    } else {
      mfma_half(buf, 0);
      mfma_half(buf, 1);
    }
  };

  if constexpr (!HALO) for (int buf = 0;; buf ^= 1) {
    nn = nxt;
    nn.advance(K, cend, cpg, CUT);
    const bool has_nn = has_next && nn.c0 < cend;
    if (has_next) {
      if (MODE) get_params(slot);
      issue_loads(nxt);
    }
    if (MODE && has_nn && pwave) load_params_raw(nn);
    if (SPL && SCHED && MODE == 0) {
      // all B fragments of chunk c first; then chunk c+1's staging (split, LDS writes) is
      // interleaved with chunk c's bf16 MFMAs.  (The DCN variants keep the sequential order: the
      // extra 12 live VGPRs of this form spill them past the 128-VGPR cap.)
      const __bf16 *sB = reinterpret_cast<const __bf16 *>(smem + buf * BUF);
      bf16x8 fb[NPB][3];
#pragma unroll
      for (int b = 0; b < NPB; ++b)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
          fb[b][pc] = *reinterpret_cast<const bf16x8 *>(sB + pc * PTT * 32 + swz(16 * (wp0 + b) + jj, kr));
      if (has_next) store_stage(nxt, buf ^ 1);
#pragma unroll
      for (int b = 0; b < NPB; ++b)
#pragma unroll
        for (int m = 0; m < NCB; ++m) acc[m][b] = mfma_split6(fa[m], fb[b], acc[m][b]);
      if (has_next) {
#pragma unroll
        for (int i = 0; i < 6 * NCB * NPB; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
          __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);  // VALU
          if (i % 3 == 0) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // DS_WRITE
        }
      }
      if (!has_next) break;
      load_a_chunk(nxt);
    } else if (SPL) {
      mma_s(buf);
      if (!has_next) break;
      load_a_chunk(nxt);
      store_stage(nxt, buf ^ 1);
    } else if (SCHED) {
      // chunk c+1's staging math + LDS writes are interleaved with the second half of chunk c's
      // MFMAs (different LDS buffers), so each wave keeps its matrix pipe busy by itself.
      // The half-1 operands are read before the staging writes: LDS reads and writes of the two
      // buffers cannot be proven disjoint, so reads issued after the writes would hold every
      // MFMA of half 1 behind the whole staging store.
      Frag f1;
      if (CK == 32) {
        mfma_half(buf, 0);
        read_frag(buf, 1, f1);
      } else {  // 16-channel chunks: one half, which carries the staging interleave
        read_frag(buf, 0, f1);
      }
      if (!has_next) {
        mma(f1);
        break;
      }
      store_stage(nxt, buf ^ 1);
      mma(f1);
#pragma unroll
      for (int i = 0; i < 4 * NCB * NPB; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);  // VALU
        if (i % 2 == 0) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // DS_WRITE
      }
    } else {
      mfma_half(buf, 0);
      if (CK == 32) mfma_half(buf, 1);
      if (!has_next) break;
      store_stage(nxt, buf ^ 1);
    }
    if (MODE && has_nn && pwave) finish_params(nn, slot ^ 1);
    __syncthreads();
    slot ^= 1;
    nxt = nn;
    has_next = has_nn;
  }

  if constexpr (HALO) {
    // stride 1, dilation = padding = d (the round-3 stride-2 NCHW form, HALO 3, was removed in
    // round 4: faster alone, slower in the two-stream step)
    constexpr int d = PH ? 1 : HALO;  // tap spacing in the halo
    constexpr int hw = 16 + 2 * d, npos = (8 + 2 * d) * hw;
    const int hy = hy0 - d, hx = hx0 - d;
    constexpr int HIT = (npos * 8 + FNT - 1) / FNT;  // halo quads per thread (NHWC)
    f32x4 hv[HIT];
    // 64-channel tiles recompute the halo quad offsets per chunk (a few VALU) rather than hold
    // them across the chunk loop: held, they were spilled to scratch and re-read every chunk
    // (76 B/lane at the 128-VGPR cap).  32-channel tiles have the registers to hold them.
    auto load_halo = [&](int c0) {
      const int soff = __builtin_amdgcn_readfirstlane(c0 * 4);
      int t = tid;
      if constexpr (CO_T >= 64) asm volatile("" : "+v"(t));  // keep the arithmetic in the loop
#pragma unroll
      for (int i = 0; i < HIT; ++i) {
        const int e = t + FNT * i, pos = e >> 3;
        const int yy = hy + pos / hw, xx = hx + pos % hw;
        const int iy = PH ? pa + pd * yy : yy, ix = PH ? pb + pd * xx : xx;  // image position
        const bool ok = pos < npos && yy >= 0 && iy < a.H && xx >= 0 && ix < a.W;
        const int off = ok ? ((iy * a.W + ix) * a.C + 4 * (e & 7)) * 4 : img_bytes;  // zero padding: OOB
        hv[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, off, soff, 0));
      }
    };
    bf16x8 ha0[NCB][3], ha1[NCB][3];  // A fragments of two taps (double buffer)
    // A fragments by buffer loads: per-lane offset lane*16 (one VGPR), everything else in the
    // wave-uniform SGPR offset, so no per-tap address lives in VGPRs
    const auto war = __builtin_amdgcn_make_buffer_rsrc((void *)a.wsplit, (short)0, 0x7ffffff0, 0x00020000);
    auto load_ha = [&](bf16x8 (&ha)[NCB][3], int c0, int k) {
      const int base = ((((gc * sT + st64) * K + k) * sNCC + ((c0 - cbeg) >> 5)) * 4 + sbb) * 3;
#pragma unroll
      for (int m = 0; m < NCB; ++m)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
          ha[m][pc] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
              war, lane * 16, __builtin_amdgcn_readfirstlane((base + 3 * m + pc) * 1024), 0));
    };
    // B fragment LDS address of (tile row r, column jj) at halo row/column shift (si, sj)
    const int jjd = jj;
    // tap k of the chunk at c0: prefetch the next tap's A (the next chunk's tap 0 after tap 8),
    // then the B fragments at the tap's shifted halo positions and the MFMAs
    auto tap = [&](bf16x8 (&cur)[NCB][3], bf16x8 (&nxt)[NCB][3], int k, int c0, bool more) {
      // keep the scheduler from hoisting later taps' work (SSA values, no WAR on the buffers)
      // above this tap: 9 taps of fragments and addresses would not fit the 128-VGPR budget
      __builtin_amdgcn_sched_barrier(0);
      if (k < 8)
        load_ha(nxt, c0, k + 1);
      else if (more)
        load_ha(nxt, c0 + 32, 0);
      const int ti = k / 3, tj = k % 3;
      int col = jjd;
      asm volatile("" : "+v"(col));  // recomputed per tap (not hoisted as 18 live addresses)
#pragma unroll
      for (int b = 0; b < NPB; ++b) {
        const int pos = (wp0 + b + ti * d) * hw + col + tj * d;
        const __bf16 *sH = reinterpret_cast<const __bf16 *>(smem) + swz(pos, kr);
        bf16x8 fb[3];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) fb[pc] = *reinterpret_cast<const bf16x8 *>(sH + pc * npos * 32);
#pragma unroll
        for (int m = 0; m < NCB; ++m) acc[m][b] = mfma_split6(cur[m], fb, acc[m][b]);
      }
    };
    auto stage = [&](int c0) {
      __syncthreads();  // every wave is done with the previous chunk's halo
#pragma unroll
      for (int i = 0; i < HIT; ++i) {
        const int pos = (tid + FNT * i) >> 3;
        if (pos < npos) put_split(reinterpret_cast<__bf16 *>(smem), npos * 32, pos, tid & 7, hv[i]);
      }
      __syncthreads();
      const bool more = c0 + 32 < cend;
      if (more) load_halo(c0 + 32);
      return more;
    };
    load_halo(cbeg);
    load_ha(ha0, cbeg, 0);
    // nine taps per chunk: the A buffers alternate, so consecutive chunks start on opposite ones
    for (int c0 = cbeg; c0 < cend; c0 += 64) {
      bool more = stage(c0);
      tap(ha0, ha1, 0, c0, more); tap(ha1, ha0, 1, c0, more); tap(ha0, ha1, 2, c0, more);
      tap(ha1, ha0, 3, c0, more); tap(ha0, ha1, 4, c0, more); tap(ha1, ha0, 5, c0, more);
      tap(ha0, ha1, 6, c0, more); tap(ha1, ha0, 7, c0, more); tap(ha0, ha1, 8, c0, more);
      if (!more) break;
      more = stage(c0 + 32);
      tap(ha1, ha0, 0, c0 + 32, more); tap(ha0, ha1, 1, c0 + 32, more); tap(ha1, ha0, 2, c0 + 32, more);
      tap(ha0, ha1, 3, c0 + 32, more); tap(ha1, ha0, 4, c0 + 32, more); tap(ha0, ha1, 5, c0 + 32, more);
      tap(ha1, ha0, 6, c0 + 32, more); tap(ha0, ha1, 7, c0 + 32, more); tap(ha1, ha0, 8, c0 + 32, more);
    }
  }

  if (TAIL) {
    // act(post_scale*(acc+bias)+post_shift) -> LDS as the B operand [px][c] of a second GEMM with
    // the pointwise weights [co2][c] (channels 32h..32h+31 in buffer h), then re-contract.
    // The per-channel parameters of the wave's accumulator rows (and, PREC 1, every A fragment
    // of the pointwise weights) are loaded as one batch ahead of the barrier: element-wise
    // guarded loads would each wait out an L2 round trip.
    constexpr int NH = (CO_T + 31) / 32;  // channel chunks of the pointwise GEMM
    float pb[NCB][4], ps[NCB][4], ph[NCB][4];
#pragma unroll
    for (int m = 0; m < NCB; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int cc = min(co0 + 16 * (wc0 + m) + 4 * kr + r, co_end - 1);
        pb[m][r] = a.bias ? a.bias[cc] : 0.f;
        ps[m][r] = a.post_scale ? a.post_scale[cc] : 1.f;
        ph[m][r] = a.post_scale ? a.post_shift[cc] : 0.f;
      }
    bf16x8 ta[SPL ? NH : 1][SPL ? NCB : 1][3];
    if constexpr (SPL) {
#pragma unroll
      for (int h2 = 0; h2 < NH; ++h2)
#pragma unroll
        for (int m = 0; m < NCB; ++m)
#pragma unroll
          for (int pc = 0; pc < 3; ++pc)
            ta[h2][m][pc] = a.tail_wsplit[((h2 * 4 + sbb + m) * 3 + pc) * 64 + lane];
    }
    __syncthreads();
    // SPL with two co blocks per wave (the 64-channel tails): the wave's blocks are the lower and
    // upper 16 channels of one 32-channel chunk, and lane (kr, jj) holds 4 channels of each: half
    // of a 16-byte piece quad.  Lanes kr and kr ^ 1 (16 apart, same pixel) swap one half so that
    // each holds a whole quad -- the even lane quad kr / 2 of the lower block, the odd lane quad
    // 2 + kr / 2 of the upper -- and the pieces go to LDS as ds_write_b128 under swz_tail.  The
    // round-3 form wrote each half with ds_write_b64 (16 rows at one quad per lane group: 4-way
    // bank conflicts, 144 conflict cycles per wave; MI355X_MICROARCH.md §LDS lane groups).
#ifndef AANET_TAIL_PAIRED  // A/B build switch (tools/build_variant.sh): 0 = the round-3 b64 staging
#define AANET_TAIL_PAIRED 1
#endif
    constexpr bool PAIRED = AANET_TAIL_PAIRED && SPL && NCB == 2;
    if constexpr (PAIRED) {
      float *sC = smem + (wc0 >> 1) * BUF;
      const bool odd = (kr & 1) != 0;
      const int unit = odd ? 2 + (kr >> 1) : (kr >> 1);
#pragma unroll
      for (int b = 0; b < NPB; ++b) {
        f32x4 v[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int co = co0 + 16 * (wc0 + m) + 4 * kr + r;
            const float t = apply_act((acc[m][b][r] + pb[m][r]) * ps[m][r] + ph[m][r], a.act);
            v[m][r] = co < co_end ? t : 0.f;
          }
        float f8[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float recv = __shfl_xor(odd ? v[0][r] : v[1][r], 16);
          f8[r] = odd ? recv : v[0][r];
          f8[4 + r] = odd ? v[1][r] : recv;
        }
        bf16x8_t pcs[3];
        split8_t(f8, pcs);
        __bf16 *plane = reinterpret_cast<__bf16 *>(sC);
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
          *reinterpret_cast<bf16x8_t *>(plane + pc * PTT * 32 + swz_tail(16 * (wp0 + b) + jj, unit)) = pcs[pc];
        acc[0][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[1][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int m = 0; m < NCB && !PAIRED; ++m) {
      const int mg = wc0 + m;
      float *sC = smem + (mg >> 1) * BUF;
#pragma unroll
      for (int b = 0; b < NPB; ++b) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = co0 + 16 * mg + 4 * kr + r;
          const float t = apply_act((acc[m][b][r] + pb[m][r]) * ps[m][r] + ph[m][r], a.act);
          v[r] = co < co_end ? t : 0.f;
        }
        if constexpr (SPL)
          put_split(reinterpret_cast<__bf16 *>(sC), PTT * 32, 16 * (wp0 + b) + jj, 4 * (mg & 1) + kr, v);
        else
          *reinterpret_cast<f32x4 *>(sC + (16 * (wp0 + b) + jj) * SP + 16 * (mg & 1) + 4 * kr) = v;
        acc[m][b] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int h2 = 0; h2 < NH; ++h2) {
      if constexpr (SPL) continue;  // tail weights: pre-split fragments (tail_wsplit)
      float *sW = smem + h2 * BUF + PTT * SP;
      for (int e = tid; e < KC * CO_T; e += FNT) {
        const int co2 = e / KC, cl = e % KC, c = 32 * h2 + cl;
        sW[co2 * SP + cl] = (co2 < a.Co2 && c < a.Co) ? a.tail_w[(long)co2 * a.Co + c] : 0.f;
      }
      if (CO_T == 16) {  // channels 16..31 of the single chunk were never written
        float *sC = smem;
        for (int e = tid; e < PTT * 16; e += FNT) sC[(e / 16) * SP + 16 + e % 16] = 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int h2 = 0; h2 < NH; ++h2) {
      if constexpr (SPL) {
        const __bf16 *sB = reinterpret_cast<const __bf16 *>(smem + h2 * BUF);
#pragma unroll
        for (int b = 0; b < NPB; ++b) {
          bf16x8 fb[3];
#pragma unroll
          for (int pc = 0; pc < 3; ++pc)
            fb[pc] = *reinterpret_cast<const bf16x8 *>(
                sB + pc * PTT * 32 + (PAIRED ? swz_tail(16 * (wp0 + b) + jj, kr) : swz(16 * (wp0 + b) + jj, kr)));
#pragma unroll
          for (int m = 0; m < NCB; ++m) acc[m][b] = mfma_split6(ta[h2][m], fb, acc[m][b]);
        }
      } else {
        mfma_chunk(h2);
      }
    }
  }

  // Epilogue: accumulators -> LDS [co][px] -> 16-byte row segments (+ residual) -> HBM.
  constexpr int QPR = PTT / 4;  // float4 per tile row
  constexpr int CQ = CO_T / 4;  // channel quads (NHWC output rows)
  constexpr int NE = ONH ? PTT * CQ : CO_T * QPR;
  constexpr int EPT = (NE + FNT - 1) / FNT;
  const int cout = TAIL ? a.Co2 : a.Co;
  const int cend_o = TAIL ? a.Co2 : co_end;
  const float *ebias = TAIL ? a.tail_b : a.bias;
  const float *esc = TAIL ? nullptr : a.post_scale;
  const float *esh = TAIL ? nullptr : a.post_shift;
  const int eact = TAIL ? a.tail_act : a.act;
  __syncthreads();
  float *sO = smem;
#pragma unroll
  for (int m = 0; m < NCB; ++m)
#pragma unroll
    for (int b = 0; b < NPB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        sO[(16 * (wc0 + m) + 4 * kr + r) * OP + 16 * (wp0 + b) + jj] = acc[m][b][r];
  static_assert(!ONH || FNT % CQ == 0, "NHWC epilogue: one channel quad per thread");
  // NHWC output: the 4 channels of the thread's quad (the NCHW form loads per item: holding its
  // parameters here costs the DCN tail kernel spills)
  float eb[4] = {0.f, 0.f, 0.f, 0.f}, es[4] = {1.f, 1.f, 1.f, 1.f}, eh[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (ONH) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cc = min(co0 + 4 * (tid % CQ) + i, cend_o - 1);
      eb[i] = ebias ? ebias[cc] : 0.f;
      es[i] = esc ? esc[cc] : 1.f;
      eh[i] = esc ? esh[cc] : 0.f;
    }
  }
  __syncthreads();
  const long p0 = (long)tile * PTT;
  // output pixel of tile-local index px (flattened, -1 outside the image); quad q = px 4q..4q+3
  auto pix = [&](int px) -> long {
    if constexpr (HALO) {
      int y = hy0 + (px >> 4), x = hx0 + (px & 15);
      if constexpr (PH) y = pa + pd * y, x = pb + pd * x;
      return (y < a.Ho && x < a.Wo) ? (long)y * a.Wo + x : -1;
    } else {
      return p0 + px < P ? p0 + px : -1;
    }
  };
  const bool vec = HALO ? (a.Wo & 3) == 0 : (P & 3) == 0;
  auto quad_ok = [&](int q) -> bool {  // the quad is inside the image and 16-byte aligned
    if constexpr (HALO)
      return vec && hy0 + (q >> 2) < a.Ho && hx0 + 4 * (q & 3) + 3 < a.Wo;
    else
      return vec && p0 + 4 * q + 3 < P;
  };
  if constexpr (ONH) {  // [px][co] rows of 16-byte channel quads
    for (int e = tid; e < PTT * CQ; e += FNT) {
      const int px = e / CQ, cq = e % CQ, co = co0 + 4 * cq;
      const long pe = pix(px);
      if (co >= co_end || pe < 0) continue;
      f32x4 v;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float t = sO[(4 * cq + u) * OP + px] + eb[u];
        if (a.post_scale) t = t * es[u] + eh[u];
        v[u] = t;
      }
      const long o = ((long)n * P + pe) * a.Co + co;
      if (a.residual) v += *reinterpret_cast<const f32x4 *>(a.residual + o);
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = apply_act(v[u], a.act);
      *reinterpret_cast<f32x4 *>(a.out + o) = v;
    }
    return;
  }
  // Items (4 pixels x 1 channel) are processed two at a time with every global load of the pair
  // (residual, CSA source segments) issued before any use: a per-item load->use chain would
  // expose the HBM / L2 latency once per item.
  constexpr int EB = EPT >= 2 ? 2 : 1;
  const bool csa = TAIL && a.csa_out;
  // Every item of a thread has the same quad q = tid % QPR (FNT is a multiple of QPR): its pixel,
  // and for the CSA terms the source rows, segment start and row weights, are computed once per
  // thread here (round 5: they were recomputed per item in both passes -- an integer division and
  // 64-bit address math per item and term); per item only the channel plane changes.
  static_assert(FNT % QPR == 0, "items of a thread share their quad");
  const int qt = tid % QPR;
  const long pet = pix(4 * qt);
  const bool qokt = quad_ok(qt);
  // buffer resources over image n's planes (SGPRs) and 32-bit byte offsets per item: the output,
  // CSA output and residual at (co P + pixel) * 4, the CSA sources at (co ih iw + row + column) * 4
  // (round 5: per item a 64-bit plane product and pointer per access)
  const long img = (long)n * cout * P;
  const brsrc_t ro = buf_rsrc(a.out + img, (long)cout * P * 4);
  const brsrc_t rcs = buf_rsrc(csa ? a.csa_out + img : a.out + img, (long)cout * P * 4);
  const brsrc_t rre = buf_rsrc(a.residual ? a.residual + img : a.out + img, (long)cout * P * 4);
  const unsigned pq = qokt ? 4u * (unsigned)pet : 0u;
  brsrc_t ru[2] = {ro, ro};
  unsigned urow0[2] = {0u, 0u}, urow1[2] = {0u, 0u}, uhw[2] = {0u, 0u};
  int us0[2] = {0, 0}, uiw[2] = {4, 4};
  float uh0[2] = {1.f, 1.f}, uh1[2] = {0.f, 0.f};
  bool sfast = true;
  if (csa) {
    // (the halo tile knows its row and column; the flat form divides in 32 bits: a 64-bit
    // division here was ~150 instructions of the epilogue)
    int y, qq;
    if constexpr (HALO) {
      y = hy0 + ((4 * qt) >> 4);
      qq = (hx0 + 4 * (qt & 3)) >> 2;
    } else {
      y = qokt ? (int)pet / a.Wo : 0;
      qq = qokt ? ((int)pet % a.Wo) >> 2 : 0;  // Wo % 4 == 0 (launcher)
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j >= a.num_up) break;
      const int ih = a.up_h[j], iw = a.up_w[j], r = a.up_r[j];
      ru[j] = buf_rsrc(a.up[j] + (long)n * cout * ih * iw, (long)cout * ih * iw * 4);
      uhw[j] = 4u * (unsigned)(ih * iw);
      uiw[j] = iw;
      // PyTorch's area_pixel_compute_scale (ih / Ho) and source row, align_corners=False
      float hr = ((float)ih / (float)a.Ho) * ((float)y + 0.5f) - 0.5f;
      hr = hr < 0.f ? 0.f : hr;
      const int h1 = (int)hr, h1p = h1 < ih - 1 ? 1 : 0;
      urow0[j] = 4u * (unsigned)(h1 * iw);
      urow1[j] = 4u * (unsigned)((h1 + h1p) * iw);
      us0[j] = r == 2 ? 2 * qq - 1 : qq - 1;
      sfast = sfast && us0[j] >= 0 && us0[j] + 3 <= iw - 1;
      uh1[j] = hr - (float)h1;
      uh0[j] = 1.f - uh1[j];
    }
  }
  // the image-edge quads read clamped columns: a wave with one takes the per-column loads
  const bool wfast = __all(sfast || !qokt);
#pragma unroll
  for (int i0 = 0; i0 < EPT; i0 += EB) {
    f32x4 ev[EB], er[EB], eu[EB][2][2];
    float pbi[EB], psc[EB], psh[EB];
    bool eok[EB];
#pragma unroll
    for (int b = 0; b < EB; ++b) {
      const int e = tid + (i0 + b) * FNT;
      const int col = e / QPR, co = co0 + col;
      eok[b] = (NE % FNT == 0 || e < NE) && co < cend_o && qokt;
      if (!eok[b]) continue;
      // the channel's parameters in this load pass too: loaded in the use pass, each item
      // waited for its own
      pbi[b] = ebias ? ebias[co] : 0.f;
      psc[b] = esc ? esc[co] : 1.f;
      psh[b] = esc ? esh[co] : 0.f;
      ev[b] = *reinterpret_cast<const f32x4 *>(sO + col * OP + 4 * qt);
      if (a.residual) er[b] = buf_ld4(rre, 4u * (unsigned)(co * (int)P) + pq);
      if (csa) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (j >= a.num_up) break;
          const unsigned pl = (unsigned)co * uhw[j];
          eu[b][j][0] = buf_seg(ru[j], pl + urow0[j], us0[j], uiw[j], wfast);
          eu[b][j][1] = buf_seg(ru[j], pl + urow1[j], us0[j], uiw[j], wfast);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < EB; ++b) {
      if (!eok[b]) continue;
      const int e = tid + (i0 + b) * FNT;
      const int col = e / QPR, co = co0 + col;
      const unsigned po = 4u * (unsigned)(co * (int)P) + pq;
      const float bias = pbi[b], sc = psc[b], sh = psh[b];
      f32x4 v = ev[b];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float t = v[u] + bias;
        if (esc) t = t * sc + sh;
        if (a.residual) t += er[b][u];
        v[u] = apply_act(t, eact);
      }
      buf_st4(ro, po, v);
      if (csa) {
        // cross-scale sum of this output branch (nets/aggregation.py:387-400): the block output
        // (the identity term) + exact 2x/4x upsamplings of the coarser exchange terms, LeakyReLU
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (j >= a.num_up) break;
          v += uh0[j] * hlerp(eu[b][j][0], a.up_r[j]) + uh1[j] * hlerp(eu[b][j][1], a.up_r[j]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = apply_act(v[u], a.csa_act);
        buf_st4(rcs, po, v);
        // post stage: the CSA output back into the item's own slot (its B operand)
        if constexpr (POST) *reinterpret_cast<f32x4 *>(sO + col * OP + 4 * qt) = v;
      }
    }
  }
  // pixels the quad path does not cover (P % 4 != 0, ragged last tile): one element at a time
  if (!quad_ok(QPR - 1) || !quad_ok(0)) {
    for (int e = tid; e < NE; e += FNT) {
      const int col = e / QPR, q = e % QPR, co = co0 + col;
      if (co >= cend_o || quad_ok(q)) continue;
      const float bias = ebias ? ebias[co] : 0.f;
      const float sc = esc ? esc[co] : 1.f;
      const float sh = esc ? esh[co] : 0.f;
      const f32x4 v = *reinterpret_cast<const f32x4 *>(sO + col * OP + 4 * q);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long pe = pix(4 * q + u);
        if (pe < 0) continue;
        const long o = ((long)n * cout + co) * P + pe;
        float t = v[u] + bias;
        if (esc) t = t * sc + sh;
        if (a.residual) t += a.residual[o];
        a.out[o] = apply_act(t, eact);
      }
    }
  }
  if constexpr (POST && TAIL && HALO && CO_T == 64 && PTT == 128 && SPL) {
    // ---- post stage (aanet_post_stage_t, NHWC out): t = W . csa + b, act, channels-last ------
    // The wave keeps its (co blocks wc0.., px blocks wp0..) layout.  B of lane (kr, jj): channels
    // {32h2 + 4kr + r, 32h2 + 16 + 4kr + r} of the pixel (rows 4kr apart in sO: 4 OP = 16 mod 32
    // banks); A: the same permutation read from the standard fragments in global memory.
    __syncthreads();  // every item's CSA value is in sO
    bf16x8 pb3[NPB][2][3];
#pragma unroll
    for (int b = 0; b < NPB; ++b)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        f32x4 lo4, hi4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          lo4[r] = sO[(32 * h2 + 4 * kr + r) * OP + 16 * (wp0 + b) + jj];
          hi4[r] = sO[(32 * h2 + 16 + 4 * kr + r) * OP + 16 * (wp0 + b) + jj];
        }
        bf16x4 h0, m0, l0, h1, m1, l1;
        split3(lo4, h0, m0, l0);
        split3(hi4, h1, m1, l1);
        pb3[b][h2][0] = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
        pb3[b][h2][1] = __builtin_shufflevector(m0, m1, 0, 1, 2, 3, 4, 5, 6, 7);
        pb3[b][h2][2] = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
      }
    const char *pw = a.post_w + ((((kr >> 1) << 4) | jj) * 16 + 8 * (kr & 1));
    typedef unsigned pu32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned pu32x4 __attribute__((ext_vector_type(4)));
    f32x4 pacc[NCB][NPB];
#pragma unroll
    for (int m = 0; m < NCB; ++m) {
#pragma unroll
      for (int b = 0; b < NPB; ++b) pacc[m][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        bf16x8 A[3];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
          const char *f = pw + ((h2 * 4 + wc0 + m) * 3 + pc) * 1024;
          const pu32x2 lo = *reinterpret_cast<const pu32x2 *>(f);
          const pu32x2 hi = *reinterpret_cast<const pu32x2 *>(f + 512);
          A[pc] = __builtin_bit_cast(bf16x8, pu32x4{lo.x, lo.y, hi.x, hi.y});
        }
#pragma unroll
        for (int b = 0; b < NPB; ++b) pacc[m][b] = mfma_split6(A, pb3[b][h2], pacc[m][b]);
      }
    }
#pragma unroll
    for (int m = 0; m < NCB; ++m) {
      const int co = 16 * (wc0 + m) + 4 * kr;
      const f32x4 bb = a.post_b ? *reinterpret_cast<const f32x4 *>(a.post_b + co)
                                : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int b = 0; b < NPB; ++b) {
        const long pe = pix(16 * (wp0 + b) + jj);
        if (pe < 0) continue;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = apply_act(pacc[m][b][r] + bb[r], a.post_act);
        *reinterpret_cast<f32x4 *>(a.post_out + ((long)n * P + pe) * 64 + co) = v;
      }
    }
  }
}

// --------------------------------------------------------------- debug: im2col / index --
__global__ void mdcn_im2col_kernel(MdcnArgs a, float *__restrict__ col) {
  const long P = (long)a.Ho * a.Wo;
  const int K = a.kh * a.kw, cpg = a.C / a.dg;
  const long total = (long)a.C * K * P;
  const long HW = (long)a.H * a.W;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x) {
    const long p = e % P;
    const int ck = (int)(e / P), c = ck / K, k = ck % K;
    Samp2 s;
    pixel_samp2(s, a, 0, c / cpg, k, p, (int)(p / a.Wo), (int)(p % a.Wo));
    col[e] = samp_val2(a.x + (long)c * HW, s);
  }
}

__global__ void mdcn_sample_index_kernel(MdcnArgs a, int *__restrict__ hl, int *__restrict__ wl,
                                         int *__restrict__ vd) {
#pragma clang fp contract(off)
  const long P = (long)a.Ho * a.Wo;
  const int K = a.kh * a.kw;
  const long total = (long)a.N * a.dg * K * P;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x) {
    const long p = e % P;
    long t = e / P;
    const int k = (int)(t % K);
    t /= K;
    const int g = (int)(t % a.dg), n = (int)(t / a.dg);
    const int i = k / a.kw, j = k % a.kw, ho = (int)(p / a.Wo), wo = (int)(p % a.Wo);
    const float *off = a.offset + (long)n * a.off_bs + (long)g * 2 * K * P;
    const float h = (float)(ho * a.stride - a.pad + i * a.dil) + off[(long)(2 * k) * P + p];
    const float w = (float)(wo * a.stride - a.pad + j * a.dil) + off[(long)(2 * k + 1) * P + p];
    hl[e] = (int)floorf(h);
    wl[e] = (int)floorf(w);
    vd[e] = (h > -1.f && w > -1.f && h < (float)a.H && w < (float)a.W) ? 1 : 0;
  }
}

int check_sizes(int N, int C, int H, int W, int Co, int kh, int kw, int stride, int pad, int dil,
                int groups, int dg, int Ho, int Wo) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || Co <= 0 || kh <= 0 || kw <= 0 || stride <= 0 ||
      pad < 0 || dil <= 0 || groups <= 0 || dg <= 0)
    return AANET_EINVAL;
  if (C % groups || Co % groups || C % dg) return AANET_EINVAL;
  if (Ho <= 0 || Wo <= 0) return AANET_EINVAL;
  // one image's planes are addressed by 32-bit buffer offsets (the epilogues)
  if ((long)C * H * W * 4 >= (1L << 31) || (long)Co * Ho * Wo * 4 >= (1L << 31))
    return AANET_EUNSUPPORTED;
  return AANET_OK;
}

}  // namespace

int check_shapes(const MdcnArgs &a) {
  return check_sizes(a.N, a.C, a.H, a.W, a.Co, a.kh, a.kw, a.stride, a.pad, a.dil, a.groups, a.dg,
                     a.Ho, a.Wo);
}

MdcnArgs make_args(const float *x, const float *offset, long off_bs, const float *mask,
                   long mask_bs, int mask_logits, float mask_scale, const float *weight,
                   const float *bias, const float *ps, const float *psh, int act, float *out,
                   int n, int c, int h, int w, int co, int kh, int kw, int stride, int pad,
                   int dil, int groups, int dg) {
  MdcnArgs a;
  a.x = x;
  a.offset = offset;
  a.mask = mask;
  a.mask_logits = mask_logits;
  a.mask_scale = mask_scale;
  a.weight = weight;
  a.bias = bias;
  a.post_scale = ps;
  a.post_shift = psh;
  a.residual = nullptr;
  a.tail_w = nullptr;
  a.tail_b = nullptr;
  a.tail_act = 0;
  a.Co2 = co;
  a.act = act;
  a.out = out;
  a.N = n;
  a.C = c;
  a.H = h;
  a.W = w;
  a.Co = co;
  a.kh = kh;
  a.kw = kw;
  a.stride = stride;
  a.pad = pad;
  a.dil = dil;
  a.groups = groups;
  a.dg = dg;
  a.layout = 0;
  a.split = 0;
  a.halo = 0;
  a.dbg_noatom = 0;
  a.csa_out = nullptr;
  a.num_up = 0;
  a.csa_act = 0;
  a.post = nullptr;
  a.post_w = nullptr;
  a.post_b = nullptr;
  a.post_act = 0;
  a.post_out = nullptr;
  for (int j = 0; j < 3; ++j) {
    a.up[j] = nullptr;
    a.up_h[j] = a.up_w[j] = a.up_r[j] = 1;
  }
  // stride <= 0 is refused by check_shapes; the output size must not divide by it first
  a.Ho = stride > 0 ? conv_out_size(h, kh, stride, pad, dil) : 0;
  a.Wo = stride > 0 ? conv_out_size(w, kw, stride, pad, dil) : 0;
  const long P = (long)a.Ho * a.Wo, K = (long)kh * kw;
  a.off_bs = off_bs >= 0 ? off_bs : (long)dg * 2 * K * P;
  a.mask_bs = mask_bs >= 0 ? mask_bs : (long)dg * K * P;
  return a;
}

namespace {

// DcnSmallArgs of the op-level form (no tail) from the engine's arguments
DcnSmallArgs small_args(const MdcnArgs &a, const float *weight, int packed) {
  DcnSmallArgs t{};
  t.x = a.x;
  t.offset = a.offset;
  t.off_bs = a.off_bs;
  t.mask = a.mask;
  t.mask_bs = a.mask_bs;
  t.mask_logits = a.mask_logits;
  t.mask_scale = a.mask_scale;
  t.w = weight;
  t.packed = packed;
  t.bias = a.bias;
  t.post_scale = a.post_scale;
  t.post_shift = a.post_shift;
  t.act = a.act;
  t.out = a.out;
  t.N = a.N;
  t.C = a.C;
  t.H = a.H;
  t.W = a.W;
  t.Co = a.Co;
  t.Co2 = a.Co;
  t.pad = a.pad;
  t.dil = a.dil;
  t.dg = a.dg;
  return t;
}

// Every run-time choice below reads the plan (conv_engine_plan), never the arguments.
template <int MODE, int CO_T, int PTT, int FULL, int CFG>
void launch_fwd_f(const MdcnArgs &a, const aanet_conv_plan_t &pl, dim3 grid, hipStream_t st) {
  const dim3 blk(FNT);
  if constexpr (!FULL && MODE == 0 && CFG == 0 && CO_T >= 32) {
    // plain NCHW conv, group width 16 (mod 32): split-bf16 over zero-padded 32-channel chunks
    if (pl.prec) {
      hipLaunchKernelGGL((conv_fwd_kernel<0, CO_T, PTT, 1, 0, 1, 0, 0, 0, 1>), grid, blk, 0, st, a);
      return;
    }
  }
  if constexpr (FULL && CFG == 0 && CO_T >= 32) {  // split-bf16 contraction (PREC 1)
    if constexpr (MODE == 0 && PTT == 128) {
      if (pl.halo == 4) {  // phase-strided halo tile (dilation > 2)
        if (pl.layout == 3)
          hipLaunchKernelGGL((conv_fwd_kernel<0, CO_T, 128, 1, 0, 1, 1, 3, CFG, 1, 4>), grid, blk, 0, st, a);
        return;
      }
      if (pl.halo == 1 || pl.halo == 2) {  // 3x3 stride-1 halo-tile form (NHWC input), HALO = dil
        if (pl.halo == 1) {
          if (pl.tail && pl.post && CO_T == 64)
            hipLaunchKernelGGL((conv_fwd_kernel<0, CO_T, 128, 1, 1, 1, 1, 1, CFG, 1, 1, 1>), grid, blk, 0, st, a);
          else if (pl.tail)
            hipLaunchKernelGGL((conv_fwd_kernel<0, CO_T, 128, 1, 1, 1, 1, 1, CFG, 1, 1>), grid, blk, 0, st, a);
          else if (pl.layout == 3)
            hipLaunchKernelGGL((conv_fwd_kernel<0, CO_T, 128, 1, 0, 1, 1, 3, CFG, 1, 1>), grid, blk, 0, st, a);
          else
            hipLaunchKernelGGL((conv_fwd_kernel<0, CO_T, 128, 1, 0, 1, 1, 1, CFG, 1, 1>), grid, blk, 0, st, a);
        } else {
          if (pl.tail)
            hipLaunchKernelGGL((conv_fwd_kernel<0, CO_T, 128, 1, 1, 1, 1, 1, CFG, 1, 2>), grid, blk, 0, st, a);
          else if (pl.layout == 3)
            hipLaunchKernelGGL((conv_fwd_kernel<0, CO_T, 128, 1, 0, 1, 1, 3, CFG, 1, 2>), grid, blk, 0, st, a);
          else
            hipLaunchKernelGGL((conv_fwd_kernel<0, CO_T, 128, 1, 0, 1, 1, 1, CFG, 1, 2>), grid, blk, 0, st, a);
        }
        return;
      }
    }
    if (pl.prec) {
      if (pl.tail) {
        if (pl.layout == 1)
          hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 1, 1, 1, 1, CFG, 1>), grid, blk, 0, st, a);
        else
          hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 1, 1, 1, 0, CFG, 1>), grid, blk, 0, st, a);
        return;
      }
      switch (pl.layout) {
        case 1: hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 0, 1, 1, 1, CFG, 1>), grid, blk, 0, st, a); break;
        case 2: hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 0, 1, 1, 2, CFG, 1>), grid, blk, 0, st, a); break;
        case 3: hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 0, 1, 1, 3, CFG, 1>), grid, blk, 0, st, a); break;
        default: hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 0, 1, 1, 0, CFG, 1>), grid, blk, 0, st, a); break;
      }
      return;
    }
  }
  if (pl.tail) {
    if (FULL && pl.layout == 1)
      hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 1, 1, FULL, FULL ? 1 : 0, CFG>), grid, blk, 0, st, a);
    else
      hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 1, 1, FULL, 0, CFG>), grid, blk, 0, st, a);
  } else if (pl.packed) {
    if constexpr (FULL) {
      switch (pl.layout) {
        case 1: hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 0, 1, 1, 1, CFG>), grid, blk, 0, st, a); break;
        case 2: hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 0, 1, 1, 2, CFG>), grid, blk, 0, st, a); break;
        case 3: hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 0, 1, 1, 3, CFG>), grid, blk, 0, st, a); break;
        default: hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 0, 1, 1, 0, CFG>), grid, blk, 0, st, a); break;
      }
    } else {  // guarded chunks exist in LAYOUT 0 only (conv_engine_plan)
      hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 1, 0, 1, 0, 0, CFG>), grid, blk, 0, st, a);
    }
  } else {
    hipLaunchKernelGGL((conv_fwd_kernel<MODE, CO_T, PTT, 0, 0, 0, FULL, 0, CFG>), grid, blk, 0, st, a);
  }
}

// Chunk configuration (conv_fwd_kernel CFG) for which every chunk is full, or -1.
int full_cfg(int C, int groups, int dg, int mode, int co_t) {
  const int Cg = C / groups, cpg = C / dg;
  if (Cg % KC == 0 && (!mode || cpg % KC == 0)) return 0;
  if (mode && Cg % KC == 0 && cpg == 16) return 2;
  if (co_t >= 32 && Cg % 16 == 0 && (!mode || cpg % 16 == 0)) return 1;
  return -1;
}

int split_selected(int flags, int packed);

// Every decision of the engine's launch (aanet_conv_engine_plan, include/aanet_mi355x.h): the
// size checks, the tile (co_t x ptt), the chunk configuration, the halo form, the contraction,
// the instance's layout and the grid.  Pure host code; launch_fwd launches what it returns.
// -> the status the launch would return; pl's other members are filled when it is AANET_OK.
int conv_engine_plan(const aanet_conv_plan_query_t &q, aanet_conv_plan_t &pl) {
  const int mode = q.mode;
  if (mode != 0 && mode != 1) return AANET_EINVAL;
  const int dg = mode ? q.dg : 1;
  if (q.stride <= 0) return AANET_EINVAL;  // before the output size divides by it
  const int Ho = conv_out_size(q.h, q.kh, q.stride, q.pad, q.dil);
  const int Wo = conv_out_size(q.w, q.kw, q.stride, q.pad, q.dil);
  const int rc = check_sizes(q.n, q.c, q.h, q.w, q.co, q.kh, q.kw, q.stride, q.pad, q.dil, q.groups,
                             dg, Ho, Wo);
  if (rc) return rc;
  if (mode && q.w < 2) return AANET_EUNSUPPORTED;  // pair-gather sampler needs 2 columns
  const int layout = q.layout & ~(AANET_CONV_EXACT_F32 | AANET_CONV_WEIGHTS_SPLIT |
                                  (mode ? AANET_CONV_GENERIC_DCN : 0));
  if (layout < 0 || layout > 3) return AANET_EINVAL;
  const int packed = q.packed != 0, split = split_selected(q.layout, packed), tail = q.co2 != 0;
  const long P = (long)Ho * Wo;
  const int Cog = q.co / q.groups;
  if (q.csa) {  // CSA epilogue: tail kernels, quad-aligned rows, exact 2x / 4x terms
    if (!tail || Wo % 4 || q.num_up < 0 || q.num_up > 2) return AANET_EUNSUPPORTED;
    for (int j = 0; j < q.num_up; ++j) {
      const int r = q.up_h[j] > 0 ? Ho / q.up_h[j] : 0;
      if ((r != 2 && r != 4) || q.up_h[j] * r != Ho || q.up_w[j] * r != Wo)
        return AANET_EUNSUPPORTED;
    }
  }
  int co_t = Cog <= 16 ? 16 : (Cog <= 32 ? 32 : 64);
  if (tail) {  // the whole conv output column of a pixel must sit in one workgroup
    if (q.groups != 1 || q.co > 64 || q.co2 <= 0 || q.co2 > 64 || !packed) return AANET_EUNSUPPORTED;
    co_t = max(q.co, q.co2) <= 16 ? 16 : (max(q.co, q.co2) <= 32 ? 32 : 64);
  }
  const int cfg = full_cfg(q.c, q.groups, dg, mode, co_t);
  if (layout) {  // NHWC paths: packed weights, full chunks (full_cfg), 4-channel quads
    if (!packed || q.c % 4 || cfg < 0) return AANET_EUNSUPPORTED;
    if ((layout & 2) && (tail || Cog % 4)) return AANET_EUNSUPPORTED;
  }
  const int ncot = host_div_up(Cog, co_t);
  // 128-pixel tiles when they still give >= 2 workgroups per CU (the scale-1 convs of the C2
  // pyramid, 832 tiles: stride-2 64->64 exchange conv 93 -> 86 us), else 64
  int ptt = co_t == 16 || (long)q.n * host_div_up(P, 128) * q.groups * ncot >= 512 ? 128 : 64;
  if (cfg == 1) ptt = 128;  // 16-channel chunks are staged 4 per thread
  const bool s1_3x3 = mode == 0 && split && q.kh == 3 && q.kw == 3 && q.stride == 1 &&
                      q.pad == q.dil && co_t >= 32 && cfg == 0;
  // 3x3 stride-1 halo tile on NHWC input, HALO = dil (1 or 2)
  int halo = s1_3x3 && (layout & 1) && q.dil <= 2 ? q.dil : 0;
  // dilations > 2 (the refinement's dilated blocks): the phase-strided halo tile (HALO 4),
  // NHWC in and out, no tail
  if (!halo && s1_3x3 && layout == 3 && q.dil > 2 && !tail && !q.csa && !q.post) halo = 4;
  if (halo) ptt = 128;
  // post stage (aanet_post_stage_t): the HALO 1 tail with the CSA epilogue, 64 -> 64 channels,
  // NHWC output only; anything else is left to the caller before any launch
  if (q.post && (mode != 0 || !q.csa || halo != 1 || co_t != 64 || q.co2 != 64 || q.post != 1 || !split))
    return AANET_EUNSUPPORTED;
  // the instance: guarded or full chunks (a split pack of group width 16 mod 32 runs the plain
  // NCHW conv over zero-padded 32-channel chunks, FULL 0 with PREC 1)
  const bool padded = mode == 0 && co_t >= 32 && split && !tail && layout == 0 && (q.c / q.groups) % 32;
  pl.full = !padded && (cfg == 0 || (cfg == 1 && co_t >= 32 && ptt == 128) || (cfg == 2 && mode));
  pl.cfg = pl.full ? cfg : 0;
  pl.prec = padded || (pl.full && pl.cfg == 0 && co_t >= 32 && split);
  pl.halo = halo;
  pl.tail = tail;
  pl.post = halo == 1 && tail && q.post && co_t == 64;
  pl.packed = packed;
  if (halo)
    pl.layout = tail ? 1 : (layout == 3 ? 3 : 1);
  else if (tail)
    pl.layout = pl.full && layout == 1 ? 1 : 0;
  else
    pl.layout = packed && pl.full ? layout : 0;
  pl.co_t = co_t;
  pl.ptt = ptt;
  const int hd = halo == 4 ? q.dil : 1;  // phase stride (HALO 4)
  const int wh = host_div_up(Wo, hd), hh = host_div_up(Ho, hd);
  pl.grid_x = (int)(unsigned)(halo ? (long)q.n * hd * hd * host_div_up(wh, 16) * host_div_up(hh, 8)
                                   : q.n * host_div_up(P, ptt));
  pl.grid_y = q.groups * ncot;
  if (halo) {
    pl.last_tile_cols = wh % 16;
    pl.last_tile_rows = hh % 8;
    pl.last_tile_pixels = pl.last_tile_cols || pl.last_tile_rows
                              ? (pl.last_tile_cols ? pl.last_tile_cols : 16) *
                                    (pl.last_tile_rows ? pl.last_tile_rows : 8)
                              : 0;
  } else {
    pl.last_tile_cols = pl.last_tile_rows = 0;
    pl.last_tile_pixels = (int)(P % ptt);
  }
  return AANET_OK;
}

template <int MODE, int CO_T, int PTT>
void launch_fwd_t(const MdcnArgs &a, const aanet_conv_plan_t &pl, dim3 grid, hipStream_t st) {
  constexpr bool C1 = CO_T >= 32 && PTT == 128;  // 16-channel chunks: 4 staged values per thread
  if (!pl.full)
    launch_fwd_f<MODE, CO_T, PTT, 0, 0>(a, pl, grid, st);
  else if (pl.cfg == 1 && C1)
    launch_fwd_f<MODE, CO_T, PTT, 1, C1 ? 1 : 0>(a, pl, grid, st);
  else if (pl.cfg == 2 && MODE)
    launch_fwd_f<MODE, CO_T, PTT, 1, MODE ? 2 : 0>(a, pl, grid, st);
  else
    launch_fwd_f<MODE, CO_T, PTT, 1, 0>(a, pl, grid, st);
}

template <int MODE>
int launch_fwd(const MdcnArgs &a_in, int packed, hipStream_t st) {
  MdcnArgs a = a_in;
  const int rc = check_shapes(a);
  if (rc) return rc;
  if (!a.x || !a.weight || !a.out) return AANET_EINVAL;
  if (MODE && (!a.offset || !a.mask)) return AANET_EINVAL;
  if (a.post_scale && !a.post_shift) return AANET_EINVAL;
  // everything else is decided by conv_engine_plan, from the sizes alone
  aanet_conv_plan_query_t q{};
  q.struct_size = sizeof(q);
  q.mode = MODE;
  q.n = a.N;
  q.c = a.C;
  q.h = a.H;
  q.w = a.W;
  q.co = a.Co;
  q.co2 = a.tail_w ? (a.Co2 > 0 ? a.Co2 : -1) : 0;
  q.kh = a.kh;
  q.kw = a.kw;
  q.stride = a.stride;
  q.pad = a.pad;
  q.dil = a.dil;
  q.groups = a.groups;
  q.dg = a.dg;
  q.layout = a.layout | (a.split ? AANET_CONV_WEIGHTS_SPLIT : 0);
  q.packed = packed;
  q.csa = a.csa_out != nullptr;
  q.num_up = a.num_up;
  for (int j = 0; j < 3; ++j) {
    q.up_h[j] = a.up_h[j];
    q.up_w[j] = a.up_w[j];
  }
  q.post = a.post ? (a.post->disp || !a.post->out_nhwc || a.post->skip_outputs ? 2 : 1) : 0;
  aanet_conv_plan_t pl{};
  pl.struct_size = sizeof(pl);
  pl.status = conv_engine_plan(q, pl);
  if (pl.status) return pl.status;
  a.halo = pl.halo == 4 ? 4 : (pl.halo ? 1 : 0);
  const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y);
  if (pl.ptt == 128) {
    switch (pl.co_t) {
      case 16: launch_fwd_t<MODE, 16, 128>(a, pl, grid, st); break;
      case 32: launch_fwd_t<MODE, 32, 128>(a, pl, grid, st); break;
      default: launch_fwd_t<MODE, 64, 128>(a, pl, grid, st); break;
    }
  } else {
    switch (pl.co_t) {
      case 16: break;  // unreachable: 16-channel tiles always take 128-pixel tiles
      case 32: launch_fwd_t<MODE, 32, 64>(a, pl, grid, st); break;
      default: launch_fwd_t<MODE, 64, 64>(a, pl, grid, st); break;
    }
  }
  return aanet_launch_status();
}

__global__ void pack_weight_kernel(const float *__restrict__ w, float *__restrict__ wp, int Co,
                                   int Cg, int K) {
  const long total = (long)Co * Cg * K;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x) {
    const int k = (int)(e % K);
    const long t = e / K;
    const int c = (int)(t % Cg), co = (int)(t / Cg);
    wp[((long)k * Co + co) * Cg + c] = w[e];
  }
}

// PREC 1 needs weight buffers from aanet_conv_weight_pack_split_f32 (AANET_CONV_WEIGHTS_SPLIT)
// and the split arithmetic selected (AANET_CONV_EXACT_F32 clear); a tail kernel's pointwise
// weights then carry their fragments too.
int split_selected(int flags, int packed) {
  return packed && (flags & AANET_CONV_WEIGHTS_SPLIT) && !(flags & AANET_CONV_EXACT_F32);
}

void set_split(MdcnArgs &a, int flags, int packed) {
  a.split = split_selected(flags, packed);
  if (!a.split) return;
  const int cg = a.C / a.groups, kk = a.kh * a.kw;
  a.wsplit = reinterpret_cast<const bf16x8_t *>(reinterpret_cast<const char *>(a.weight) +
                                                split_frag_offset(a.Co, cg, kk));
  if (a.tail_w)
    a.tail_wsplit = reinterpret_cast<const bf16x8_t *>(reinterpret_cast<const char *>(a.tail_w) +
                                                       split_frag_offset(a.Co2, a.Co, 1));
}

// one thread per (g, t, k, cc, blk, lane): 8 weights -> their three bf16 pieces
__global__ void pack_split_kernel(const float *__restrict__ w, bf16x8_t *__restrict__ frag, int Co,
                                  int Cg, int K, int groups) {
  const int Cog = Co / groups, T = (Cog + 63) / 64, NCC = (Cg + 31) / 32;  // zero-padded chunks
  const long total = (long)groups * T * K * NCC * 4 * 64;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int lane = (int)(e & 63);
    long r = e >> 6;
    const int blk = (int)(r & 3);
    r >>= 2;
    const int cc = (int)(r % NCC);
    r /= NCC;
    const int k = (int)(r % K);
    r /= K;
    const int t = (int)(r % T), g = (int)(r / T);
    const int row = 64 * t + 16 * blk + (lane & 15);
    const int co = g * Cog + row;
    bf16x8_t ph, pm, pl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 32 * cc + 8 * (lane >> 4) + j;
      const float v = row < Cog && c < Cg ? w[((long)co * Cg + c) * K + k] : 0.f;
      const __bf16 h = (__bf16)v;
      const float r1 = v - (float)h;
      const __bf16 m = (__bf16)r1;
      ph[j] = h;
      pm[j] = m;
      pl[j] = (__bf16)(r1 - (float)m);
    }
    const long o = (((((long)g * T + t) * K + k) * NCC + cc) * 4 + blk) * 3 * 64 + lane;
    frag[o] = ph;
    frag[o + 64] = pm;
    frag[o + 128] = pl;
  }
}

int set_csa(MdcnArgs &a, const aanet_csa_epilogue_t *csa) {
  if (!csa) return AANET_OK;
  if (csa->struct_size != sizeof(aanet_csa_epilogue_t)) return AANET_EABI;
  a.post = csa->post;
  if (a.post && a.post->struct_size != sizeof(aanet_post_stage_t)) return AANET_EABI;
  if (a.post && ((!a.post->out_nhwc && !a.post->disp) || !a.post->weight || a.post->act < 0 ||
                 a.post->act > 2))
    return AANET_EINVAL;
  if (a.post) {  // copied by value: the kernel never dereferences the host descriptor
    a.post_w = reinterpret_cast<const char *>(a.post->weight) + split_frag_offset(64, 64, 1);
    a.post_b = a.post->bias;
    a.post_act = a.post->act;
    a.post_out = a.post->out_nhwc;
  }
  if (!csa->out || csa->num_up < 0 || csa->num_up > 3 || csa->act < 0 || csa->act > 2)
    return AANET_EINVAL;
  a.csa_out = csa->out;
  a.num_up = csa->num_up;
  a.csa_act = csa->act;
  for (int j = 0; j < csa->num_up; ++j) {
    if (!csa->up[j] || csa->up_h[j] <= 0 || csa->up_w[j] <= 0) return AANET_EINVAL;
    a.up[j] = csa->up[j];
    a.up_h[j] = csa->up_h[j];
    a.up_w[j] = csa->up_w[j];
    a.up_r[j] = csa->up_h[j] > 0 ? a.Ho / csa->up_h[j] : 0;
  }
  return AANET_OK;
}

}  // namespace

int round_pitch(int v, int mod32) {  // smallest p >= v with p % 32 == mod32
  int p = v;
  while (p % 32 != mod32) ++p;
  return p;
}

extern "C" int aanet_mdcn_fwd_f32(const float *x, const float *offset, const float *mask,
                                  const float *weight, const float *bias, float *out, int n, int c,
                                  int h, int w, int co, int kh, int kw, int stride, int pad,
                                  int dil, int groups, int dg, aanet_stream_t stream) {
  MdcnArgs a = make_args(x, offset, -1, mask, -1, 0, 1.f, weight, bias, nullptr, nullptr, 0, out,
                         n, c, h, w, co, kh, kw, stride, pad, dil, groups, dg);
  // 16 channels in two 8-channel groups (the aggregation's coarsest scale): direct fp32 form
  if (!check_shapes(a) && groups == 1 && a.Ho == h && a.Wo == w &&
      dcn_small_supported(c, co, 0, kh, kw, stride, pad, dil, dg, groups)) {
    const int rc = dcn_small_launch(small_args(a, weight, 0), as_hip(stream));
    if (rc != AANET_EUNSUPPORTED) return rc;
  }
  return launch_fwd<1>(a, 0, as_hip(stream));
}

extern "C" int aanet_conv2d_fused_f32(const float *x, const float *weight, const float *bias,
                                      const float *post_scale, const float *post_shift,
                                      const float *residual, int act, int weight_packed,
                                      float *out, int n, int c, int h, int w, int co, int kh,
                                      int kw, int stride, int pad, int dil, int groups, int layout,
                                      aanet_stream_t stream) {
  if (act < 0 || act > 2) return AANET_EINVAL;
  // the argument checks of launch_fwd, before any of the specialised kernels below is chosen
  if (!x || !weight || !out || (post_scale && !post_shift)) return AANET_EINVAL;
  MdcnArgs a = make_args(x, nullptr, 0, nullptr, 0, 0, 1.f, weight, bias, post_scale, post_shift,
                         act, out, n, c, h, w, co, kh, kw, stride, pad, dil, groups, 1);
  a.residual = residual;
  set_split(a, layout, weight_packed);
  a.layout = layout & ~(AANET_CONV_EXACT_F32 | AANET_CONV_WEIGHTS_SPLIT);
  // few-channel convs (Cin <= 6 or Co == 1): the direct VALU kernel (small_conv.hip)
  if ((a.layout == 0 || a.layout == 1) && groups == 1 && kh == kw && !check_shapes(a)) {
    DirectArgs d;
    d.x = x;
    d.w = weight;
    d.bias = bias;
    d.post_scale = post_scale;
    d.post_shift = post_shift;
    d.residual = residual;
    d.out = out;
    d.act = act;
    d.packed = weight_packed != 0;
    d.in_nhwc = a.layout & 1;
    d.N = n;
    d.C = c;
    d.H = h;
    d.W = w;
    d.Co = co;
    d.Ho = a.Ho;
    d.Wo = a.Wo;
    d.pad = pad;
    const int rc = conv_direct_launch(d, kh, stride, dil, as_hip(stream));
    if (rc != AANET_EUNSUPPORTED) return rc;
  }
  if (a.split && a.layout >= 0 && a.layout <= 3 && !check_shapes(a) &&
      pw_conv_supported(c, co, kh, kw, stride, pad, groups, (long)n * h * w, a.layout >> 1, h * w)) {
    PwArgs p;  // 1x1: the streaming kernel (pointwise.hip)
    p.x = x;
    p.wsplit = a.wsplit;
    p.bias = bias;
    p.post_scale = post_scale;
    p.post_shift = post_shift;
    p.residual = residual;
    p.act = act;
    p.out = out;
    p.N = n;
    p.C = c;
    p.P = h * w;
    p.Co = co;
    p.in_nhwc = a.layout & 1;
    p.out_nhwc = a.layout >> 1;
    const int rc = pw_conv_launch(p, as_hip(stream));
    if (rc != AANET_EUNSUPPORTED) return rc;
  }
  return launch_fwd<0>(a, weight_packed, as_hip(stream));
}

extern "C" int aanet_conv2d_pw_f32(const float *x, const float *weight_packed, const float *bias,
                                   const float *post_scale, const float *post_shift, int act,
                                   const float *pw_weight_packed, const float *pw_bias,
                                   const float *residual, int pw_act, int co2, float *out, int n,
                                   int c, int h, int w, int co, int kh, int kw, int stride,
                                   int pad, int dil, const aanet_csa_epilogue_t *csa, int layout,
                                   aanet_stream_t stream) {
  if (act < 0 || act > 2 || pw_act < 0 || pw_act > 2 || !pw_weight_packed) return AANET_EINVAL;
  const int flags = layout;
  layout &= ~(AANET_CONV_EXACT_F32 | AANET_CONV_WEIGHTS_SPLIT);
  if (layout != 0 && layout != 1) return AANET_EINVAL;
  MdcnArgs a = make_args(x, nullptr, 0, nullptr, 0, 0, 1.f, weight_packed, bias, post_scale,
                         post_shift, act, out, n, c, h, w, co, kh, kw, stride, pad, dil, 1, 1);
  a.layout = layout;
  const int rc = set_csa(a, csa);
  if (rc) return rc;
  a.tail_w = pw_weight_packed;
  a.tail_b = pw_bias;
  a.tail_act = pw_act;
  a.Co2 = co2;
  a.residual = residual;
  set_split(a, flags, 1);
  return launch_fwd<0>(a, 1, as_hip(stream));
}

extern "C" int aanet_mdcn_pw_f32(const float *x, const float *offset, long offset_batch_stride,
                                 const float *mask, long mask_batch_stride, int mask_logits,
                                 float mask_scale, const float *weight_packed, const float *bias,
                                 const float *post_scale, const float *post_shift, int act,
                                 const float *pw_weight_packed, const float *pw_bias,
                                 const float *residual, int pw_act, int co2, float *out, int n,
                                 int c, int h, int w, int co, int kh, int kw, int stride, int pad,
                                 int dil, int dg, const aanet_csa_epilogue_t *csa, int layout,
                                 aanet_stream_t stream) {
  if (act < 0 || act > 2 || pw_act < 0 || pw_act > 2 || !pw_weight_packed) return AANET_EINVAL;
  const int flags = layout;
  const bool generic = (layout & AANET_CONV_GENERIC_DCN) != 0;
  layout &= ~(AANET_CONV_EXACT_F32 | AANET_CONV_WEIGHTS_SPLIT | AANET_CONV_GENERIC_DCN);
  if (layout != 0 && layout != 1) return AANET_EINVAL;
  MdcnArgs a = make_args(x, offset, offset_batch_stride, mask, mask_batch_stride, mask_logits,
                         mask_scale, weight_packed, bias, post_scale, post_shift, act, out, n, c,
                         h, w, co, kh, kw, stride, pad, dil, 1, dg);
  a.layout = layout;
  const int rc = set_csa(a, csa);
  if (rc) return rc;
  a.tail_w = pw_weight_packed;
  a.tail_b = pw_bias;
  a.tail_act = pw_act;
  a.Co2 = co2;
  a.residual = residual;
  set_split(a, flags, 1);
  // the deformable bottleneck tail of the aggregation: LDS-window form (dcn_tile.hip)
  if (!generic && a.split && layout == 1 && a.Ho == h && a.Wo == w &&
      dcn_tile_supported(c, co, co2, kh, kw, stride, pad, dil, dg, 1, w)) {
    DcnTileArgs t{};
    t.x = x;
    t.offset = a.offset;
    t.off_bs = a.off_bs;
    t.mask = a.mask;
    t.mask_bs = a.mask_bs;
    t.mask_logits = mask_logits;
    t.mask_scale = mask_scale;
    t.wsplit = a.wsplit;
    t.bias = bias;
    t.post_scale = post_scale;
    t.post_shift = post_shift;
    t.act = act;
    t.tail_wsplit = a.tail_wsplit;
    t.tail_b = pw_bias;
    t.tail_act = pw_act;
    t.residual = residual;
    t.out = out;
    t.csa_out = a.csa_out;
    t.num_up = a.csa_out ? a.num_up : 0;
    t.csa_act = a.csa_act;
    for (int j = 0; j < 2; ++j) {
      t.up[j] = a.up[j];
      t.up_h[j] = a.up_h[j];
      t.up_w[j] = a.up_w[j];
      t.up_r[j] = a.up_r[j];
    }
    t.N = n;
    t.C = c;
    t.H = h;
    t.W = w;
    t.Co = co;
    t.Co2 = co2;
    t.dil = dil;
    t.dg = dg;
    t.dbg = 0;
    t.post_wsplit = nullptr;
    t.post_b = nullptr;
    t.post_act = 0;
    t.post_out = t.post_disp = nullptr;
    t.post_skip = 0;
    if (a.post) {
      if (co2 != 64) return AANET_EUNSUPPORTED;
      t.post_wsplit = reinterpret_cast<const char *>(a.post->weight) + split_frag_offset(64, 64, 1);
      t.post_b = a.post->bias;
      t.post_act = a.post->act;
      t.post_out = a.post->out_nhwc;
      t.post_disp = a.post->disp;
      t.post_skip = a.post->skip_outputs != 0;
    }
    const int rc2 = (a.csa_out && a.num_up > 2) ? AANET_EUNSUPPORTED : dcn_tile_launch(t, as_hip(stream));
    if (rc2 != AANET_EUNSUPPORTED) return rc2;
  }
  if (a.post) return AANET_EUNSUPPORTED;  // the generic engine has no post stage
  // the coarsest scale's 16-channel block (two 8-channel groups): direct fp32 form (dcn_small.hip)
  if (!generic && layout == 0 && !a.csa_out && a.Ho == h && a.Wo == w &&
      dcn_small_supported(c, co, co2, kh, kw, stride, pad, dil, dg, 1)) {
    DcnSmallArgs t = small_args(a, weight_packed, 1);
    t.tail_w = pw_weight_packed;
    t.tail_b = pw_bias;
    t.tail_act = pw_act;
    t.residual = residual;
    t.Co2 = co2;
    const int rc2 = dcn_small_launch(t, as_hip(stream));
    if (rc2 != AANET_EUNSUPPORTED) return rc2;
  }
  return launch_fwd<1>(a, 1, as_hip(stream));
}

extern "C" int aanet_mdcn_fwd_fused_f32(const float *x, const float *offset,
                                        long offset_batch_stride, const float *mask,
                                        long mask_batch_stride, int mask_logits, float mask_scale,
                                        const float *weight, int weight_packed, const float *bias,
                                        const float *post_scale, const float *post_shift, int act,
                                        float *out, int n, int c, int h, int w, int co, int kh,
                                        int kw, int stride, int pad, int dil, int groups, int dg,
                                        int layout, aanet_stream_t stream) {
  if (act < 0 || act > 2) return AANET_EINVAL;
  MdcnArgs a = make_args(x, offset, offset_batch_stride, mask, mask_batch_stride, mask_logits,
                         mask_scale, weight, bias, post_scale, post_shift, act, out, n, c, h, w,
                         co, kh, kw, stride, pad, dil, groups, dg);
  set_split(a, layout, weight_packed);
  const bool generic = (layout & AANET_CONV_GENERIC_DCN) != 0;
  a.layout = layout & ~(AANET_CONV_EXACT_F32 | AANET_CONV_WEIGHTS_SPLIT | AANET_CONV_GENERIC_DCN);
  // the aggregation's deformable convs (3x3, dil 2, two groups of 16 / 32 channels): LDS-window
  // form with the plain epilogue (dcn_tile.hip), NCHW or channels-last x, NCHW out
  if (!generic && a.split && (a.layout == 0 || a.layout == 1) && groups == 1 && a.Ho == h &&
      a.Wo == w && dcn_tile_supported(c, co, co, kh, kw, stride, pad, dil, dg, 1, w)) {
    DcnTileArgs t{};
    t.x = x;
    t.offset = a.offset;
    t.off_bs = a.off_bs;
    t.mask = a.mask;
    t.mask_bs = a.mask_bs;
    t.mask_logits = mask_logits;
    t.mask_scale = mask_scale;
    t.wsplit = a.wsplit;
    t.bias = bias;
    t.post_scale = post_scale;
    t.post_shift = post_shift;
    t.act = act;
    t.out = out;
    t.N = n;
    t.C = c;
    t.H = h;
    t.W = w;
    t.Co = co;
    t.Co2 = co;
    t.dil = dil;
    t.dg = dg;
    t.x_nchw = a.layout == 0;
    t.plain = 1;
    const int rc = dcn_tile_launch(t, as_hip(stream));
    if (rc != AANET_EUNSUPPORTED) return rc;
  }
  if (!generic && a.layout == 0 && groups == 1 && a.Ho == h && a.Wo == w &&
      dcn_small_supported(c, co, 0, kh, kw, stride, pad, dil, dg, groups)) {
    const int rc = dcn_small_launch(small_args(a, weight, weight_packed), as_hip(stream));
    if (rc != AANET_EUNSUPPORTED) return rc;
  }
  return launch_fwd<1>(a, weight_packed, as_hip(stream));
}

extern "C" int aanet_conv_engine_plan(const aanet_conv_plan_query_t *q, aanet_conv_plan_t *plan) {
  if (!q || !plan) return AANET_EINVAL;
  if (q->struct_size != sizeof(*q) || plan->struct_size != sizeof(*plan)) return AANET_EABI;
  aanet_conv_plan_t pl{};
  pl.struct_size = sizeof(pl);
  pl.status = conv_engine_plan(*q, pl);
  *plan = pl;
  return AANET_OK;
}

extern "C" int aanet_mdcn_window_fwd_supported(int c, int co, int kh, int kw, int stride, int pad,
                                               int dil, int groups, int dg, int w) {
  return groups == 1 && dcn_tile_supported(c, co, co, kh, kw, stride, pad, dil, dg, 1, w);
}

// The data gradient's weight straight into the engine layout: wt[g*cg + i][j][k] =
// w[g*(co/groups) + j][i][K-1-k] (per-group transpose, spatial flip), stored [k][co'][cg'] with
// co' = groups*cg, cg' = co/groups -- what pack_weight_kernel makes of the transposed, flipped
// copy, in one pass over w.
__global__ void pack_weight_dgrad_kernel(const float *__restrict__ w, float *__restrict__ wp, int Co,
                                         int Cg, int K, int groups) {
  const int Cot = groups * Cg, Cgt = Co / groups;
  const long total = (long)Cot * Cgt * K;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % Cgt);  // wt's input channel j (output order: [k][co'][cg'])
    const long t = e / Cgt;
    const int cot = (int)(t % Cot), k = (int)(t / Cot);
    const int g = cot / Cg, i = cot - g * Cg;
    wp[e] = w[((long)(g * Cgt + c) * Cg + i) * K + (K - 1 - k)];
  }
}

extern "C" int aanet_conv_weight_pack_dgrad_f32(const float *weight, float *weight_packed, int co,
                                                int cg, int kh, int kw, int groups,
                                                aanet_stream_t stream) {
  AANET_HOST_CHECK(weight && weight_packed && co > 0 && cg > 0 && kh > 0 && kw > 0 && groups > 0 &&
                   co % groups == 0);
  const long total = (long)co * cg * kh * kw;
  hipLaunchKernelGGL(pack_weight_dgrad_kernel,
                     dim3(host_div_up(total, 256) > 4096 ? 4096 : host_div_up(total, 256)), dim3(256),
                     0, as_hip(stream), weight, weight_packed, co, cg, kh * kw, groups);
  return aanet_launch_status();
}

extern "C" int aanet_conv_weight_pack_f32(const float *weight, float *weight_packed, int co,
                                          int cg, int kh, int kw, aanet_stream_t stream) {
  AANET_HOST_CHECK(weight && weight_packed && co > 0 && cg > 0 && kh > 0 && kw > 0);
  const long total = (long)co * cg * kh * kw;
  hipLaunchKernelGGL(pack_weight_kernel, dim3(host_div_up(total, 256) > 4096 ? 4096 : host_div_up(total, 256)),
                     dim3(256), 0, as_hip(stream), weight, weight_packed, co, cg, kh * kw);
  return aanet_launch_status();
}

extern "C" long aanet_conv_weight_pack_split_bytes(int co, int cg, int kh, int kw, int groups) {
  // cg a multiple of 32, or of 16 past 32 (48, 80, ...: the last chunk zero-padded; plain NCHW
  // convs only take the split form then)
  if (co <= 0 || cg <= 0 || kh <= 0 || kw <= 0 || groups <= 0 || co % groups) return 0;
  if (cg % 32 && (cg % 16 || cg < 48)) return 0;
  return split_frag_offset(co, cg, kh * kw) + split_frag_count(co, cg, kh * kw, groups) * 16;
}

extern "C" int aanet_conv_weight_pack_split_f32(const float *weight, void *out, int co, int cg,
                                                int kh, int kw, int groups,
                                                aanet_stream_t stream) {
  AANET_HOST_CHECK(weight && out);
  if (aanet_conv_weight_pack_split_bytes(co, cg, kh, kw, groups) == 0) return AANET_EUNSUPPORTED;
  const int rc = aanet_conv_weight_pack_f32(weight, static_cast<float *>(out), co, cg, kh, kw, stream);
  if (rc) return rc;
  const int kk = kh * kw;
  const long n = split_frag_count(co, cg, kk, groups) / 3;
  hipLaunchKernelGGL(pack_split_kernel, dim3(host_div_up(n, 256) > 4096 ? 4096 : host_div_up(n, 256)),
                     dim3(256), 0, as_hip(stream), weight,
                     reinterpret_cast<bf16x8_t *>(static_cast<char *>(out) + split_frag_offset(co, cg, kk)),
                     co, cg, kk, groups);
  return aanet_launch_status();
}

extern "C" int aanet_mdcn_im2col_f32(const float *x, const float *offset, const float *mask,
                                     float *col, int c, int h, int w, int kh, int kw, int stride,
                                     int pad, int dil, int dg, aanet_stream_t stream) {
  MdcnArgs a = make_args(x, offset, -1, mask, -1, 0, 1.f, nullptr, nullptr, nullptr, nullptr, 0,
                         nullptr, 1, c, h, w, 1, kh, kw, stride, pad, dil, 1, dg);
  const int rc = check_shapes(a);
  if (rc) return rc;
  if (!x || !offset || !mask || !col) return AANET_EINVAL;
  if (w < 2) return AANET_EUNSUPPORTED;
  const long total = (long)c * kh * kw * a.Ho * a.Wo;
  hipLaunchKernelGGL(mdcn_im2col_kernel, dim3(host_div_up(total, 256) > 8192 ? 8192 : host_div_up(total, 256)),
                     dim3(256), 0, as_hip(stream), a, col);
  return aanet_launch_status();
}

extern "C" int aanet_mdcn_sample_index(const float *offset, int *h_low, int *w_low, int *valid,
                                       int n, int h, int w, int kh, int kw, int stride, int pad,
                                       int dil, int dg, aanet_stream_t stream) {
  MdcnArgs a = make_args(nullptr, offset, -1, nullptr, -1, 0, 1.f, nullptr, nullptr, nullptr,
                         nullptr, 0, nullptr, n, dg, h, w, 1, kh, kw, stride, pad, dil, 1, dg);
  const int rc = check_shapes(a);
  if (rc) return rc;
  if (!offset || !h_low || !w_low || !valid) return AANET_EINVAL;
  const long total = (long)n * dg * kh * kw * a.Ho * a.Wo;
  hipLaunchKernelGGL(mdcn_sample_index_kernel,
                     dim3(host_div_up(total, 256) > 8192 ? 8192 : host_div_up(total, 256)), dim3(256),
                     0, as_hip(stream), a, h_low, w_low, valid);
  return aanet_launch_status();
}
