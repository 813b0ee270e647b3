// fp8 weight-only GEMV for decode: y[M, N] = x[M, K] @ dequant(Wq, S)[N, K]^T with
//   Wq  OCP e4m3 [N, K], S uint8 E8M0 [N/128, K/128] (DeepSeek-V3's 128 x 128 block scales, the
//   image quant_weight_fp8_blk writes): w = q * 2^(S - 127);
//   x, y bf16, fp32 accumulation, M <= 4 (the decode batch).
//
// Decode is weight streaming (gemv.hip); this kernel streams half the bytes. Same structure as
// gemv_kernel -- weights straight to VGPRs, U x RW non-temporal 16-byte loads in flight per lane
// before any is consumed, no LDS, one xor reduction per output at the end -- with these changes:
//  * a 16-byte load is 16 weights: lane l reads k = 16 l + 1024 i, so one wave-instruction still
//    reads 1 KB contiguous of a row and eight consecutive lanes share one K block's scale;
//  * RW (2 or 4) divides 128, so a wave's rows sit in ONE 128-row block: one scale byte per lane
//    per 1 KB pass, whatever RW is;
//  * v_cvt_scalef32_pk_bf16_fp8 turns two e4m3 bytes times a float scale into a bf16 pair; with
//    2^(S - 127) as that scale the block scale is free, and e4m3 times a power of two is exact in
//    bf16, so the products feed v_dot2_f32_bf16 exactly as the bf16 kernel's do. The conversion
//    is done once per weight row and reused by all M token rows.
// N % 128 == 0 and K % 128 == 0: no row tail, and a lane's 16 weights never leave the row. The
// block exponents are 1..254 (quant_weight_fp8_blk clamps to +-126), so S << 23 is the scale's
// fp32 bit pattern.
#include "spa_common.h"

namespace spa {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4 ld_stream_q(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

__device__ __forceinline__ float e8m0_scale(uint8_t s) { return __builtin_bit_cast(float, (unsigned)s << 23); }

// 16 e4m3 bytes * sc -> 8 bf16 pairs, in K order (dword j holds k = 4j .. 4j + 3, low half first)
__device__ __forceinline__ void cvt16(const u32x4& q, const float sc, bf16x2 (&w2)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w2[2 * j] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[j], sc, false);
    w2[2 * j + 1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[j], sc, true);
  }
}

__device__ __forceinline__ float dot16(const bf16x8& xa, const bf16x8& xb, const bf16x2 (&w2)[8], float c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bf16x2 a2 = {xa[2 * j], xa[2 * j + 1]};
    c = __builtin_amdgcn_fdot2_f32_bf16(a2, w2[j], c, false);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bf16x2 b2 = {xb[2 * j], xb[2 * j + 1]};
    c = __builtin_amdgcn_fdot2_f32_bf16(b2, w2[4 + j], c, false);
  }
  return c;
}

template <int M, int RW, int U>
__global__ __launch_bounds__(256) void gemv_w8_kernel(const bf16* __restrict__ x, const uint8_t* __restrict__ wq,
                                                      const uint8_t* __restrict__ s, bf16* __restrict__ y, int N,
                                                      int K, long ldx) {
  static_assert(128 % RW == 0, "a wave's rows must share one 128-row scale block");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int row0 = wave * RW;
  if (row0 >= N) return;  // wave-uniform; N % 128 == 0, so row0 + RW <= N
  float acc[M][RW];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < RW; ++r) acc[m][r] = 0.f;
  const uint8_t* wr[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r) wr[r] = wq + (long)(row0 + r) * K;
  const uint8_t* sr = s + (long)(row0 >> 7) * (K >> 7);  // this wave's row of block scales
  auto consume = [&](const int k, const u32x4* wv, const uint8_t sb) {
    const float sc = e8m0_scale(sb);
    bf16x8 xv[M][2];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      xv[m][0] = *reinterpret_cast<const bf16x8*>(x + m * ldx + k);
      xv[m][1] = *reinterpret_cast<const bf16x8*>(x + m * ldx + k + 8);
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      bf16x2 w2[8];
      cvt16(wv[r], sc, w2);
#pragma unroll
      for (int m = 0; m < M; ++m) acc[m][r] = dot16(xv[m][0], xv[m][1], w2, acc[m][r]);
    }
  };
  int k = 16 * lane;
  for (; k + (U - 1) * 1024 < K; k += U * 1024) {
    u32x4 wv[U][RW];
    uint8_t sb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int r = 0; r < RW; ++r) wv[u][r] = ld_stream_q(wr[r] + k + u * 1024);
      sb[u] = sr[(k >> 7) + u * 8];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) consume(k + u * 1024, wv[u], sb[u]);
  }
  for (; k < K; k += 1024) {
    u32x4 wv[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) wv[r] = ld_stream_q(wr[r] + k);
    consume(k, wv, sr[k >> 7]);
  }
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const float v = wave_sum(acc[m][r]);
      if (lane == m * RW + r) y[(long)m * N + row0 + r] = (bf16)v;
    }
}

template <int M>
static void launch_gemv_w8(const bf16* x, const uint8_t* wq, const uint8_t* s, bf16* y, int N, int K, long ldx,
                           hipStream_t st) {
  if (N >= 8192) gemv_w8_kernel<M, 4, 4><<<cdiv(N / 4, 4), 256, 0, st>>>(x, wq, s, y, N, K, ldx);
  else gemv_w8_kernel<M, 2, 4><<<cdiv(N / 2, 4), 256, 0, st>>>(x, wq, s, y, N, K, ldx);
}

static void check_w8_image(const char* op, const at::Tensor& wq, const at::Tensor& s, int64_t lead) {
  TORCH_CHECK(wq.is_cuda() && s.is_cuda() && wq.scalar_type() == at::kFloat8_e4m3fn && s.scalar_type() == at::kByte,
              op, ": wq float8_e4m3fn, s uint8 (E8M0) HIP tensors");
  TORCH_CHECK(wq.dim() == lead + 2 && wq.is_contiguous() && s.is_contiguous(), op, ": wq, s contiguous");
  const int64_t N = wq.size(lead), K = wq.size(lead + 1);
  TORCH_CHECK(N % 128 == 0 && K % 128 == 0, op, ": N % 128 == 0 and K % 128 == 0 (got N = ", N, ", K = ", K, ")");
  TORCH_CHECK(s.dim() == lead + 2 && s.size(lead) == N / 128 && s.size(lead + 1) == K / 128 &&
                  (lead == 0 || s.size(0) == wq.size(0)),
              op, ": s must be [", (lead ? "E, " : ""), "N/128, K/128]");
  TORCH_CHECK(N < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && ((uintptr_t)wq.data_ptr() % 16) == 0, op,
              ": wq must be 16-byte aligned");
}

// x [M, K] bf16 (row stride ldx), wq [N, K] e4m3, s [N/128, K/128] E8M0 -> y [M, N] bf16; M <= 4
at::Tensor gemv_w8(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& s) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16, "gemv_w8: x must be a bf16 HIP tensor");
  check_w8_image("gemv_w8", wq, s, 0);
  TORCH_CHECK(x.dim() == 2 && x.size(1) == wq.size(1), "gemv_w8: x [M, K], wq [N, K]");
  TORCH_CHECK(x.device() == wq.device() && x.device() == s.device(), "gemv_w8: one device");
  const int M = x.size(0), K = x.size(1), N = wq.size(0);
  TORCH_CHECK(M >= 1 && M <= 4, "gemv_w8: M must be 1..4");
  TORCH_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0 && x.stride(0) >= K && ((uintptr_t)x.data_ptr() % 16) == 0,
              "gemv_w8: x rows must be 16-byte aligned");
  DeviceGuard g(x.device());
  auto y = at::empty({M, N}, x.options());
  if (N == 0 || K == 0) return K == 0 ? y.zero_() : y;
  auto st = stream();
  const bf16* xp = (const bf16*)x.data_ptr();
  const uint8_t* wp = (const uint8_t*)wq.data_ptr();
  const uint8_t* sp = (const uint8_t*)s.data_ptr();
  bf16* yp = (bf16*)y.data_ptr();
  switch (M) {
    case 1: launch_gemv_w8<1>(xp, wp, sp, yp, N, K, x.stride(0), st); break;
    case 2: launch_gemv_w8<2>(xp, wp, sp, yp, N, K, x.stride(0), st); break;
    case 3: launch_gemv_w8<3>(xp, wp, sp, yp, N, K, x.stride(0), st); break;
    default: launch_gemv_w8<4>(xp, wp, sp, yp, N, K, x.stride(0), st); break;
  }
  SPA_LAUNCH_CHECK();
  return y;
}


// ---------------------------------------------------------------------------------------
// Grouped (MoE) fp8 weight-only GEMV: grouped_gemv_kernel (gemv.hip) on the e4m3 image of the
// expert weights. Grid: experts x column chunks; a wave owns RW weight rows and walks the
// expert's token rows in groups of 4; experts with no rows exit at once (device row counts).
template <int RW, int U>
__global__ __launch_bounds__(256) void grouped_gemv_w8_kernel(const bf16* __restrict__ x,
                                                              const uint8_t* __restrict__ wq,
                                                              const uint8_t* __restrict__ s, bf16* __restrict__ y,
                                                              const int* __restrict__ offsets, int N, int K) {
  static_assert(128 % RW == 0, "a wave's rows must share one 128-row scale block");
  constexpr int MB = 4;
  const int lane = threadIdx.x & 63;
  const int nwb = cdiv(N / RW, 4);  // blocks per expert
  const int e = blockIdx.x / nwb;
  const int wave = __builtin_amdgcn_readfirstlane((blockIdx.x % nwb) * 4 + (threadIdx.x >> 6));
  const int r_begin = offsets[e], r_end = offsets[e + 1];
  const int row0 = wave * RW;
  if (r_begin >= r_end || row0 >= N) return;  // wave-uniform
  const uint8_t* we = wq + (long)e * N * K;
  const uint8_t* wr[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r) wr[r] = we + (long)(row0 + r) * K;
  const uint8_t* sr = s + ((long)e * (N >> 7) + (row0 >> 7)) * (K >> 7);
  for (int m0 = r_begin; m0 < r_end; m0 += MB) {
    const int mn = min(MB, r_end - m0);
    float acc[MB][RW];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int r = 0; r < RW; ++r) acc[m][r] = 0.f;
    auto consume = [&](const int k, const u32x4* wv, const uint8_t sb) {
      const float sc = e8m0_scale(sb);
      bf16x2 w2[RW][8];
#pragma unroll
      for (int r = 0; r < RW; ++r) cvt16(wv[r], sc, w2[r]);
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        if (m < mn) {
          const bf16* xr = x + (long)(m0 + m) * K + k;
          const bf16x8 xa = *reinterpret_cast<const bf16x8*>(xr);
          const bf16x8 xb = *reinterpret_cast<const bf16x8*>(xr + 8);
#pragma unroll
          for (int r = 0; r < RW; ++r) acc[m][r] = dot16(xa, xb, w2[r], acc[m][r]);
        }
      }
    };
    int k = 16 * lane;
    for (; k + (U - 1) * 1024 < K; k += U * 1024) {
      u32x4 wv[U][RW];
      uint8_t sb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int r = 0; r < RW; ++r) wv[u][r] = *reinterpret_cast<const u32x4*>(wr[r] + k + u * 1024);
        sb[u] = sr[(k >> 7) + u * 8];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) consume(k + u * 1024, wv[u], sb[u]);
    }
    for (; k < K; k += 1024) {
      u32x4 wv[RW];
#pragma unroll
      for (int r = 0; r < RW; ++r) wv[r] = *reinterpret_cast<const u32x4*>(wr[r] + k);
      consume(k, wv, sr[k >> 7]);
    }
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const float v = wave_sum(acc[m][r]);
        if (lane == m * RW + r && m < mn) y[(long)(m0 + m) * N + row0 + r] = (bf16)v;
      }
  }
}

// x [A, K] expert-sorted rows, wq [E, N, K] e4m3, s [E, N/128, K/128], offsets [E+1] (device) -> y [A, N]
at::Tensor grouped_gemv_w8(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& s,
                           const at::Tensor& offsets) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16, "grouped_gemv_w8: x must be a bf16 HIP tensor");
  check_w8_image("grouped_gemv_w8", wq, s, 1);
  TORCH_CHECK(x.dim() == 2 && x.size(1) == wq.size(2) && x.is_contiguous(),
              "grouped_gemv_w8: x [A, K] contiguous, wq [E, N, K]");
  TORCH_CHECK(offsets.is_cuda() && offsets.scalar_type() == at::kInt && offsets.is_contiguous() &&
                  offsets.numel() == wq.size(0) + 1,
              "grouped_gemv_w8: offsets int32 [E+1] on the device");
  TORCH_CHECK(x.device() == wq.device() && x.device() == s.device() && x.device() == offsets.device(),
              "grouped_gemv_w8: one device");
  const int A = x.size(0), K = x.size(1), E = wq.size(0), N = wq.size(1);
  TORCH_CHECK(((uintptr_t)x.data_ptr() % 16) == 0, "grouped_gemv_w8: x 16-byte aligned");
  DeviceGuard g(x.device());
  auto y = at::empty({A, N}, x.options());
  if (A == 0 || N == 0 || E == 0) return y;
  if (K == 0) return y.zero_();
  const int nwb = cdiv(N / 2, 4);
  TORCH_CHECK((int64_t)E * nwb < (int64_t)1 << 31, "grouped_gemv_w8: grid too large");
  grouped_gemv_w8_kernel<2, 4><<<E * nwb, 256, 0, stream()>>>(
      (const bf16*)x.data_ptr(), (const uint8_t*)wq.data_ptr(), (const uint8_t*)s.data_ptr(), (bf16*)y.data_ptr(),
      offsets.data_ptr<int>(), N, K);
  SPA_LAUNCH_CHECK();
  return y;
}

}  // namespace spa

TORCH_LIBRARY_FRAGMENT(spa, m) {
  m.def("gemv_w8(Tensor x, Tensor wq, Tensor s) -> Tensor");
  m.def("grouped_gemv_w8(Tensor x, Tensor wq, Tensor s, Tensor offsets) -> Tensor");
}
TORCH_LIBRARY_IMPL(spa, CUDA, m) {
  m.impl("gemv_w8", &spa::gemv_w8);
  m.impl("grouped_gemv_w8", &spa::grouped_gemv_w8);
}
