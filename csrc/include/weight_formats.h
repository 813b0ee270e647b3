// Weight-format policies of the decode kernels (csrc/kernels/gemv.hip, skinny_gemm.hip): what a 16-byte
// weight load holds and how it becomes bf16 operands.
//   bf16   W as stored;
//   e4m3   the fp8 weight-only image: Wq OCP e4m3 [N, K], S uint8 E8M0 [N/128, K/128], w = q * 2^(S - 127);
//   mxfp4  the OCP MXFP4 weight-only image: Wq uint8 [N, K/2], two e2m1 codes per byte (k = 2j in bits 3:0,
//          k = 2j + 1 in bits 7:4), S uint8 E8M0 [N, K/32].
// The formats and why the conversions are exact in bf16: the head of gemv.hip.
#pragma once
#include "spa_common.h"

namespace spa {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Weight formats. elem: storage type, holding 1 << SH weights; raw: one 16-byte load = H * 8 weights;
// BLOCKED: whole scale blocks, contiguous (no row tail to clamp, row stride K >> SH); ROW_SCALES: every
// weight row of a wave has its own scale byte per chunk (else the wave's rows share one); U, UG: passes in
// flight of the dense and the grouped GEMV kernel (their template argument); scale_row: the scales of weight
// row `row` of expert `e` (N rows each); scale: the scale byte of row `row` + r's chunk at k + ahead
// (ahead: a compile-time multiple of the block width, kept apart so that the look-ahead loads share one
// address register); prepare: raw chunk -> H bf16x8 in K order.
// ROW_AT_A_TIME<M, RW>: the dense GEMV kernel's statement order for a chunk (accumulate_rows). The
// arithmetic is the same either way; hipcc's load schedule is not, and it decides 1-5 % of the time
// of these kernels (profiles/gemv_unify.txt). e4m3 converts one weight row at a time (8 VGPRs of
// converted operands live, not 8 RW); bf16 has nothing to convert and takes that order only at
// M = RW = 4, where the other one measured 1 % slower. After a toolchain update, rerun
// tools/kres.sh csrc/kernels/gemv.hip and the timing of that profile: neither is pinned by a test.
struct WBf16 {
  using elem = bf16;
  using raw = bf16x8;
  static constexpr int H = 1, SH = 0, U = 4, UG = 4;
  static constexpr bool BLOCKED = false, ROW_SCALES = false;
  template <int M, int RW> static constexpr bool ROW_AT_A_TIME = M * RW == 16;
  static __device__ __forceinline__ const uint8_t* scale_row(const uint8_t*, int, int, int, int) { return nullptr; }
  static __device__ __forceinline__ uint8_t scale(const uint8_t*, int, int, int, int) { return 0; }
  static __device__ __forceinline__ void prepare(const raw& q, uint8_t, bf16x8 (&w)[H]) { w[0] = q; }
};

struct WE4m3 {
  using elem = uint8_t;
  using raw = u32x4;
  static constexpr int H = 2, SH = 0, U = 4, UG = 4;
  static constexpr bool BLOCKED = true, ROW_SCALES = false;
  template <int M, int RW> static constexpr bool ROW_AT_A_TIME = true;
  static __device__ __forceinline__ const uint8_t* scale_row(const uint8_t* s, int e, int N, int row, int K) {
    return s + ((long)e * (N >> 7) + (row >> 7)) * (K >> 7);
  }
  static __device__ __forceinline__ uint8_t scale(const uint8_t* sr, int, int, int k, int ahead) {
    return sr[(k >> 7) + (ahead >> 7)];
  }
  // dword j holds k = 4j .. 4j + 3, low half first
  static __device__ __forceinline__ void prepare(const raw& q, uint8_t sb, bf16x8 (&w)[H]) {
    const float sc = __builtin_bit_cast(float, (unsigned)sb << 23);
    bf16x4 p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      p[j] = __builtin_shufflevector(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[j], sc, false),
                                     __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[j], sc, true), 0, 1, 2, 3);
    w[0] = __builtin_shufflevector(p[0], p[1], 0, 1, 2, 3, 4, 5, 6, 7);
    w[1] = __builtin_shufflevector(p[2], p[3], 0, 1, 2, 3, 4, 5, 6, 7);
  }
};

struct WMxfp4 {
  using elem = uint8_t;
  using raw = u32x4;
  static constexpr int H = 4, SH = 1, U = 8, UG = 1;
  static constexpr bool BLOCKED = true, ROW_SCALES = true;
  template <int M, int RW> static constexpr bool ROW_AT_A_TIME = true;
  static __device__ __forceinline__ const uint8_t* scale_row(const uint8_t* s, int e, int N, int row, int K) {
    return s + ((long)e * N + row) * (K >> 5);
  }
  static __device__ __forceinline__ uint8_t scale(const uint8_t* sr, int r, int K, int k, int ahead) {
    return sr[r * (K >> 5) + (k >> 5) + (ahead >> 5)];
  }
  // dword j holds k = 8j .. 8j + 7: byte b is k = 8j + 2b (low nibble) and 8j + 2b + 1 (high nibble)
  static __device__ __forceinline__ void prepare(const raw& q, uint8_t sb, bf16x8 (&w)[H]) {
    const float sc = __builtin_bit_cast(float, (unsigned)sb << 23);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x4 lo = __builtin_shufflevector(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q[j], sc, 0),
                                                __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q[j], sc, 1), 0, 1, 2, 3);
      const bf16x4 hi = __builtin_shufflevector(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q[j], sc, 2),
                                                __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q[j], sc, 3), 0, 1, 2, 3);
      w[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
  }
};

}  // namespace spa
