// OCP MXFP4 weight-only image of a bf16 weight [E, N, K], K % 32 == 0, for the decode GEMV
// (gemv.hip, policy WMxfp4): wq uint8 [E, N, K/2], two e2m1 codes per byte (k = 2j in bits 3:0,
// k = 2j + 1 in bits 7:4; code = sign << 3 | mag, mag 0..7 = 0, .5, 1, 1.5, 2, 3, 4, 6), and
// s uint8 E8M0 [E, N, K/32], one scale 2^(s - 127) per 32 consecutive k of one row.
//
// The scale rule is the project's e4m3 recipe (fp8_quant.h) with 6 in place of 448: e is the smallest
// integer with amax <= 6 * 2^e over the block, clamped to [-126, 125], 0 for an all-zero block. Read
// off amax's bits: amax = m * 2^p with m in [1, 2) needs 6 * 2^e = 1.5 * 2^(e + 2) >= m * 2^p, so
// e = p - 2 when m <= 1.5 and p - 1 otherwise (no division, no rounding). |w| / 2^e is exact in fp32
// and is rounded to the nearest magnitude, a tie to the even code, by comparing with the seven
// midpoints; above 6 (only past the upper clamp) it saturates. The sign bit is the weight's own.
// ops/reference.py quant_mxfp4 is the bit-exact torch form.
//
// One pass: a lane loads 16 bytes (8 weights), the four lanes of a block take its amax with two
// shuffles, every lane packs its 8 codes into one dword store. Weights, codes and scales are all
// contiguous, so lane i of the flat grid owns weights 8i .. 8i + 7, bytes 4i .. 4i + 3 and, with
// its three neighbours, scale i / 4.
#include "spa_common.h"

namespace spa {

__device__ __forceinline__ int mx_e2m1_exp(float amax) {  // e with amax <= 6 * 2^e, minimal
  if (!(amax > 0.f)) return 0;
  const unsigned b = __float_as_uint(amax);
  const int e = (int)((b >> 23) & 0xff) - 127 - ((b & 0x7fffff) <= 0x400000 ? 2 : 1);
  return max(-126, min(125, e));
}

__device__ __forceinline__ unsigned e2m1_code(float v) {  // v >= 0: nearest magnitude, ties to even
  return (v > 0.25f) + (v >= 0.75f) + (v > 1.25f) + (v >= 1.75f) + (v > 2.5f) + (v >= 3.5f) + (v > 5.f);
}

__global__ __launch_bounds__(256) void quant_weight_mxfp4_kernel(const bf16* __restrict__ w,
                                                                 unsigned* __restrict__ wq,
                                                                 uint8_t* __restrict__ s, long chunks) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < chunks;  // chunks % 4 == 0: the four lanes of a block are live together
  u16x8 raw = {};
  if (live) raw = *reinterpret_cast<const u16x8*>(w + 8 * i);
  float a[8], amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = __uint_as_float((unsigned)(raw[j] & 0x7fff) << 16);  // |w|, exact
    amax = fmaxf(amax, a[j]);
  }
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
  const int e = mx_e2m1_exp(amax);
  const float inv = __uint_as_float((unsigned)(127 - e) << 23);  // 2^-e, a normal number for every e
  unsigned q = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) q |= (e2m1_code(a[j] * inv) | ((unsigned)(raw[j] >> 15) << 3)) << (4 * j);
  if (live) {
    wq[i] = q;
    if ((i & 3) == 0) s[i >> 2] = (uint8_t)(e + 127);
  }
}

// w bf16 [E, N, K] -> (wq uint8 [E, N, K/2], s uint8 [E, N, K/32])
std::vector<at::Tensor> quant_weight_mxfp4(const at::Tensor& w_) {
  TORCH_CHECK(w_.is_cuda() && w_.scalar_type() == at::kBFloat16 && w_.dim() == 3,
              "quant_weight_mxfp4: bf16 [E, N, K] HIP tensor");
  auto w = w_.contiguous();
  if ((uintptr_t)w.data_ptr() % 16) w = w.clone();  // a view at an odd offset: 16-byte loads need a copy
  const int64_t E = w.size(0), N = w.size(1), K = w.size(2);
  TORCH_CHECK(K % 32 == 0, "quant_weight_mxfp4: K % 32 == 0 (got K = ", K, ")");
  DeviceGuard g(w.device());
  auto wq = at::empty({E, N, K / 2}, w.options().dtype(at::kByte));
  auto s = at::empty({E, N, K / 32}, w.options().dtype(at::kByte));
  const int64_t chunks = E * N * K / 8;
  if (chunks == 0) return {wq, s};
  const int64_t blocks = (chunks + 255) / 256;
  TORCH_CHECK(blocks < ((int64_t)1 << 31), "quant_weight_mxfp4: tensor too large");
  quant_weight_mxfp4_kernel<<<(unsigned)blocks, 256, 0, stream()>>>((const bf16*)w.data_ptr(), (unsigned*)wq.data_ptr(),
                                                                   (uint8_t*)s.data_ptr(), chunks);
  SPA_LAUNCH_CHECK();
  return {wq, s};
}

}  // namespace spa

TORCH_LIBRARY_FRAGMENT(spa, m) { m.def("quant_weight_mxfp4(Tensor w) -> Tensor[]"); }
TORCH_LIBRARY_IMPL(spa, CUDA, m) { m.impl("quant_weight_mxfp4", &spa::quant_weight_mxfp4); }
