// Device helpers of the block-scaled e4m3 recipe (OCP e4m3 values, E8M0 power-of-two scales): one
// scale 2^e per tile, e the smallest exponent with amax / 2^e <= 448, the scaled values clamped to
// +-448 and rounded by the hardware convert. Shared by the MoE quantisers (moe_fp8.hip: 1 x 128 and
// 128 x 128 tiles), the fp8 KV-cache writers (rope.hip: one head row per tile) and the fp8 decode
// attention (decode.hip); ops/moe.py _e8m0 is the bit-exact torch form.
#pragma once
#include "spa_common.h"

namespace spa {

__device__ __forceinline__ int e8m0_exp(float amax) {       // e with amax / 2^e <= 448, minimal
  if (!(amax > 0.f)) return 0;
  const unsigned b = __float_as_uint(amax * (1.f / 448.f));
  int e = (int)((b >> 23) & 0xff) - 127;
  if (b & 0x7fffff) ++e;                                     // round the power up
  return max(-126, min(127, e));
}
__device__ __forceinline__ float e8m0_inv(int e) { return __uint_as_float((unsigned)(127 - e) << 23); }
// 2^(s - 127) of a stored scale byte (s in [1, 254]; a never-written row's 0 gives 0.f)
__device__ __forceinline__ float e8m0_val(unsigned s) { return __uint_as_float(s << 23); }
__device__ __forceinline__ int2 q8(const float (&v)[8], float inv) {
  float w[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = fminf(fmaxf(v[i] * inv, -448.f), 448.f);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(w[0], w[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(w[2], w[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(w[4], w[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(w[6], w[7], hi, true);
  return make_int2(lo, hi);
}

}  // namespace spa
