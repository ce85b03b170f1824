// split.h -- the split-bf16 contraction shared by the conv engine (mdcn.hip), dcn_tile.hip
// and pointwise.hip, and the layout of the split weight pack they read.
//
// x = h + m + l exactly, three bf16 pieces carrying x's 24 significand bits (weights: round to
// nearest even, h = bf16(x), m = bf16(x - h), l = x - h - m; activations: truncation, common.h
// split_pair).  A product a*b = sum_{i,j} a_i b_j; the six terms down to 2^-16 relative (mm, hl,
// lh, hm, mh, hh -- small first) run as v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  Every
// bf16 x bf16 product is exact in fp32 and the three dropped terms (ml, lm, ll) are below
// 2^-23 |a b|, i.e. under one fp32 rounding of the product: the contraction is fp32-accurate, not
// a reduced-precision one.  Measured on the C2 scale-0 3x3 conv against an fp64 reference
// (tools/split_lab.hip): max error 8.7e-6 (split) vs 1.0e-5 (exact f32 MFMA fma chain), mean
// 3.9e-7 vs 4.8e-7; keeping all nine terms changed no output.  bf16 MFMA runs at 16x the f32-MFMA
// rate, so the six products take 6/16 of the matrix-pipe time of the f32 contraction.
#pragma once

#include "common.h"

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Weights are split once (aanet_conv_weight_pack_split_f32) into MFMA A-operand fragments,
// streamed from L2 straight into registers: frag(g, t, k, cc, blk, pc, lane) = the 8 bf16 of
// piece pc of rows co = g*Cog + 64t + 16blk + (lane & 15), channels 32cc + 8(lane >> 4) + 0..7 of
// tap k (zero past the group's Cog).  They follow the f32 packed weights in the same buffer, at a
// 256-byte aligned offset, so the f32 engine reads the buffer unchanged.
__host__ __device__ inline long split_frag_offset(int co, int cg, int kk) {
  return ((long)co * cg * kk * 4 + 255) / 256 * 256;
}
__host__ __device__ inline long split_frag_count(int co, int cg, int kk, int groups) {
  const int cog = co / groups;
  return (long)groups * ((cog + 63) / 64) * kk * ((cg + 31) / 32) * 4 * 3 * 64;
}

// 8 values -> their three exact bf16 pieces (activations: common.h split_pair)
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 (&b)[3]) {
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  u32x4_t hh, mm, ll;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned h, m, l;
    split_pair(v[2 * i], v[2 * i + 1], h, m, l);
    hh[i] = h;
    mm[i] = m;
    ll[i] = l;
  }
  b[0] = __builtin_bit_cast(bf16x8, hh);
  b[1] = __builtin_bit_cast(bf16x8, mm);
  b[2] = __builtin_bit_cast(bf16x8, ll);
}
// sum of the six piece products, smallest first
__device__ __forceinline__ f32x4 mfma_split6(const bf16x8 (&A)[3], const bf16x8 (&B)[3], f32x4 t) {
  t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], B[1], t, 0, 0, 0);
  t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[2], t, 0, 0, 0);
  t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[2], B[0], t, 0, 0, 0);
  t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[1], t, 0, 0, 0);
  t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[1], B[0], t, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[0], B[0], t, 0, 0, 0);
}
