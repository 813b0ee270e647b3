// Weight-streaming GEMV for decode: y[M, N] = x[M, K] @ W[N, K]^T, x / y bf16, fp32 accumulation,
// M <= 4 (the decode batch), dense and grouped (MoE), for three weight formats:
//   bf16   W as stored (gemv, grouped_gemv);
//   e4m3   the fp8 weight-only image: Wq OCP e4m3 [N, K], S uint8 E8M0 [N/128, K/128] (DeepSeek-V3's
//          128 x 128 block scales, as quant_weight_fp8_blk writes them), w = q * 2^(S - 127); half the
//          bytes (gemv_w8, grouped_gemv_w8). N % 128 == 0 and K % 128 == 0.
//   mxfp4  the OCP MXFP4 weight-only image: Wq uint8 [N, K/2], two e2m1 codes per byte (k = 2j in bits
//          3:0, k = 2j + 1 in bits 7:4; code = sign << 3 | mag, mag 0..7 = 0, .5, 1, 1.5, 2, 3, 4, 6),
//          S uint8 E8M0 [N, K/32], one scale per 32 consecutive k of one row, as quant_weight_mxfp4
//          (quant_mxfp4.hip) writes them; 4.25 bits per weight (gemv_w4, grouped_gemv_w4).
//          K % 32 == 0 and N % 4 == 0.
//
// A decode step multiplies a handful of token rows by every projection matrix: pure weight
// streaming (LLaMA3-8B: 16 GB per token), so the kernel is built for HBM, not for MFMA:
//  * each wave owns RW consecutive rows of W; its lanes split K in 16-byte chunks (lane l reads
//    chunk l + 64 i), so one wave-instruction reads 1 KB contiguous of a row;
//  * U chunks x RW rows of weight loads are issued before any is consumed (U * RW * 16 B in
//    flight per lane), non-temporal in the dense kernel (read once, kept out of L2): latency is
//    hidden by memory-level parallelism, no LDS round trip (cdna_hip_programming.md, 'GEMV / M <= 16');
//  * RW = 2 for narrow outputs (N < 8192: o-proj, down-proj) so the grid still holds >= 2
//    waves per SIMD; RW = 4 otherwise;
//  * x (M x K, a few KB) is re-read per chunk from L1/L2, where it stays;
//  * products with v_dot2_f32_bf16 (2 bf16 MACs per instruction), one 64-lane xor
//    reduction per output at the end.
// torch.mm at M = 1 goes to hipBLASLt 16x16 macro tiles at 2.5-5 TB/s on streamed weights
// (decode profile: wo 2.5, wqkv 3.3, w13 3.9, w2 5.0 TB/s); this is the op the decode path uses.
//
// The loop structure exists once (accumulate_rows); a weight format is a policy struct that says
// what a 16-byte load holds, how it becomes bf16x8 operands of the dot, and in which of two
// statement orders the dense kernel consumes a chunk. For e4m3:
//  * a 16-byte load is 16 weights, so eight consecutive lanes share one K block's scale, and RW
//    (2 or 4) divides 128, so a wave's rows sit in ONE 128-row block: one scale byte per lane per
//    1 KB pass, whatever RW is;
//  * v_cvt_scalef32_pk_bf16_fp8 turns two e4m3 bytes times a float scale into a bf16 pair; with
//    2^(S - 127) as that scale the block scale is free, and e4m3 times a power of two is exact in
//    bf16, so the products feed v_dot2_f32_bf16 exactly as bf16 weights do. The conversion is done
//    once per weight row and reused by all token rows;
//  * the block exponents are 1..254 (quant_weight_fp8_blk clamps to +-126), so S << 23 is the
//    scale's fp32 bit pattern.
// For mxfp4:
//  * a 16-byte load is 32 weights = exactly one MX block, so every (lane, row, load) has its own scale
//    byte: one byte load per weight row and pass, 64 consecutive bytes per wave and row;
//  * v_cvt_scalef32_pk_bf16_fp4 turns one byte (two codes) times a float scale into a bf16 pair, low
//    nibble first; e2m1 times a power of two is exact in bf16. Scale bytes are 1..254 as above
//    (quant_weight_mxfp4 clamps the exponent to [-126, 125]);
//  * a pass is 2048 weights of a row, and U = 8 is chosen by measurement alone
//    (profiles/mxfp4_decode_gemv.txt, section 2): up to K = 14336 no row enters the 8-pass loop, all of
//    LLaMA3-8B runs through the single-pass loop behind it, and that loop, compiled behind the 8-pass
//    one, timed faster than U = 2 and U = 4 and than the same loop standing alone. Why is not known, so
//    rerun that section after a toolchain update. (8192 x 28672, where the 8-pass loop runs, is timed too.)
//    The grouped kernel keeps one pass in flight (UG = 1): with 8 it needs 256 VGPRs, one wave per SIMD,
//    and dsv3_style decode was 17 % slower than on fp8 images.
#include "spa_common.h"
#include "weight_formats.h"

namespace spa {

// The weight-format policies WBf16, WE4m3 and WMxfp4 (what a 16-byte load holds, how it becomes bf16x8 operands of
// the dot, the statement order of the dense kernel) live in weight_formats.h, shared with skinny_gemm.hip.

__device__ __forceinline__ float dot8(const bf16x8& a, const bf16x8& b, float c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bf16x2 a2 = {a[2 * j], a[2 * j + 1]};
    const bf16x2 b2 = {b[2 * j], b[2 * j + 1]};
    c = __builtin_amdgcn_fdot2_f32_bf16(a2, b2, c, false);
  }
  return c;
}

// acc[m][r] += this lane's share of x[m0 + m, :] . wr[r][:] for the first mn <= MB of those rows of x
// (row stride ldx): k ascending, every dot2 chain in element order. NT: non-temporal weight loads.
// ROWWISE (all MB rows live): the x rows of a chunk are loaded first, then each weight row is
// converted and used; else all weight rows are converted, then each live x row is loaded and used.
template <class F, int MB, int RW, int U, bool NT, bool ROWWISE>
__device__ __forceinline__ void accumulate_rows(float (&acc)[MB][RW], const bf16* __restrict__ x, const int m0,
                                                const long ldx, const int mn,
                                                const typename F::elem* const (&wr)[RW],
                                                const uint8_t* __restrict__ sr, const int K, const int lane) {
  static_assert(F::ROW_SCALES || 128 % RW == 0, "a wave's rows must share one 128-row scale block");
  using raw = typename F::raw;
  constexpr int CH = 8 * F::H, PASS = 64 * CH;  // weights per lane / per wave and pass
  constexpr int SH = F::SH, SR = F::ROW_SCALES ? RW : 1;  // SR: scale bytes per chunk
  auto load = [](const typename F::elem* p) {
    return NT ? __builtin_nontemporal_load(reinterpret_cast<const raw*>(p)) : *reinterpret_cast<const raw*>(p);
  };
  auto consume = [&](const int k, const raw* wv, const uint8_t (&sc)[SR]) {
    bf16x8 xv[MB][F::H], wp[RW][F::H];
    auto load_x = [&](const int m) {
#pragma unroll
      for (int h = 0; h < F::H; ++h)
        xv[m][h] = *reinterpret_cast<const bf16x8*>(x + (long)(m0 + m) * ldx + k + 8 * h);
    };
    if (ROWWISE) {
#pragma unroll
      for (int m = 0; m < MB; ++m) load_x(m);
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        F::prepare(wv[r], sc[F::ROW_SCALES ? r : 0], wp[r]);
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
          for (int h = 0; h < F::H; ++h) acc[m][r] = dot8(xv[m][h], wp[r][h], acc[m][r]);
      }
      return;
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) F::prepare(wv[r], sc[F::ROW_SCALES ? r : 0], wp[r]);
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      if (m < mn) {
        load_x(m);
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
          for (int h = 0; h < F::H; ++h) acc[m][r] = dot8(xv[m][h], wp[r][h], acc[m][r]);
      }
    }
  };
  int k = CH * lane;
  for (; k + (U - 1) * PASS < K; k += U * PASS) {
    raw wv[U][RW];
    uint8_t sc[U][SR];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int r = 0; r < RW; ++r) wv[u][r] = load(wr[r] + (k >> SH) + ((u * PASS) >> SH));
#pragma unroll
      for (int r = 0; r < SR; ++r) sc[u][r] = F::scale(sr, r, K, k, u * PASS);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) consume(k + u * PASS, wv[u], sc[u]);
  }
  for (; k < K; k += PASS) {
    raw wv[RW];
    uint8_t sc[SR];
#pragma unroll
    for (int r = 0; r < RW; ++r) wv[r] = load(wr[r] + (k >> SH));
#pragma unroll
    for (int r = 0; r < SR; ++r) sc[r] = F::scale(sr, r, K, k, 0);
    consume(k, wv, sc);
  }
}

// Dense: x [M, K] (row stride ldx), w [N, K] (row stride ldw), s: w's block scales -> y [M, N].
template <class F, int M, int RW, int U>
__global__ __launch_bounds__(256) void gemv_kernel(const bf16* __restrict__ x, const typename F::elem* __restrict__ w,
                                                   const uint8_t* __restrict__ s, bf16* __restrict__ y, int N, int K,
                                                   long ldx, long ldw) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const int row0 = wave * RW;
  if (row0 >= N) return;  // wave-uniform
  const typename F::elem* wr[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r)  // tail rows: duplicate, not stored
    wr[r] = w + (long)(F::BLOCKED ? row0 + r : min(row0 + r, N - 1)) * (F::BLOCKED ? (long)(K >> F::SH) : ldw);
  float acc[M][RW] = {};
  const uint8_t* sr = F::scale_row(s, 0, N, row0, K);
  accumulate_rows<F, M, RW, U, true, F::template ROW_AT_A_TIME<M, RW>>(acc, x, 0, ldx, M, wr, sr, K, lane);
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const float v = wave_sum(acc[m][r]);
      if (lane == m * RW + r && (F::BLOCKED || row0 + r < N)) y[(long)m * N + row0 + r] = (bf16)v;
    }
}

// Grouped (MoE): y[a, :] = x[a, :] @ W_e^T for the rows a in [off[e], off[e+1]) of every expert e
// (the expert-sorted assignments of a few tokens: 6 rows over 64 experts at batch 1). The MFMA
// grouped GEMM pays a 256-row tile per active expert for one or two real rows; this streams each
// ACTIVE expert's weights once instead. Grid: experts x column chunks; a wave owns RW weight rows
// (output columns) and walks the expert's token rows in groups of 4 (re-reading its weight rows
// from L2 past 4 rows, hence plain loads). Experts with no rows exit at once (the row counts live
// on the device: no host sync). x [A, K], w [E, N, K] (or its image), s, all contiguous.
template <class F, int RW, int U>
__global__ __launch_bounds__(256) void grouped_gemv_kernel(const bf16* __restrict__ x,
                                                           const typename F::elem* __restrict__ w,
                                                           const uint8_t* __restrict__ s, bf16* __restrict__ y,
                                                           const int* __restrict__ offsets, int N, int K) {
  constexpr int MB = 4;
  const int lane = threadIdx.x & 63;
  const int nwb = (N + 4 * RW - 1) / (4 * RW);  // blocks per expert; 32-bit: most blocks only get to the exit below
  const int e = blockIdx.x / nwb;
  const int wave = __builtin_amdgcn_readfirstlane((blockIdx.x % nwb) * 4 + (threadIdx.x >> 6));
  const int r_begin = offsets[e], r_end = offsets[e + 1];
  const int row0 = wave * RW;
  if (r_begin >= r_end || row0 >= N) return;  // wave-uniform
  const typename F::elem* wr[RW];
#pragma unroll
  for (int r = 0; r < RW; ++r)
    wr[r] = w + ((long)e * N + (F::BLOCKED ? row0 + r : min(row0 + r, N - 1))) * (K >> F::SH);
  const uint8_t* sr = F::scale_row(s, e, N, row0, K);
  for (int m0 = r_begin; m0 < r_end; m0 += MB) {
    const int mn = min(MB, r_end - m0);
    float acc[MB][RW] = {};
    accumulate_rows<F, MB, RW, U, false, false>(acc, x, m0, K, mn, wr, sr, K, lane);
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const float v = wave_sum(acc[m][r]);
        if (lane == m * RW + r && m < mn && (F::BLOCKED || row0 + r < N))
          y[(long)(m0 + m) * N + row0 + r] = (bf16)v;
      }
  }
}

// Host-side argument checks, shared by the six ops. `lead`: 0 dense, 1 grouped (a leading expert dim).
// The weight operand: bf16 w [.., N, K]; or with `s` an image of it: e4m3 wq [.., N, K] + s [.., N/128,
// K/128], or mxfp4 wq uint8 [.., N, K/2] + s [.., N, K/32]. Returns K, the weights per row.
template <class F>
static int64_t check_weight(const char* op, const at::Tensor& w, const at::Tensor* s, int64_t lead) {
  TORCH_CHECK(w.is_cuda() && w.dim() == lead + 2, op, ": w must be a ", lead + 2, "-D HIP tensor");
  const int64_t N = w.size(lead), K = w.size(lead + 1) << F::SH;
  TORCH_CHECK(N < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && ((uintptr_t)w.data_ptr() % 16) == 0, op,
              ": w must be 16-byte aligned");
  if (!s) {
    TORCH_CHECK(w.scalar_type() == at::kBFloat16, op, ": bf16 HIP tensors");
    // a dense weight may be a row-strided view (a slice of a wider buffer)
    TORCH_CHECK(K % 8 == 0 && (lead ? w.is_contiguous() : w.stride(1) == 1 && w.stride(0) % 8 == 0), op,
                ": rows must be 16-byte aligned with K % 8 == 0", lead ? ", w contiguous" : "");
    return K;
  }
  constexpr bool W4 = F::ROW_SCALES;
  TORCH_CHECK(s->is_cuda() && s->device() == w.device() &&
                  w.scalar_type() == (W4 ? at::kByte : at::kFloat8_e4m3fn) && s->scalar_type() == at::kByte,
              op, ": wq ", W4 ? "uint8 (two e2m1 codes per byte)" : "float8_e4m3fn",
              ", s uint8 (E8M0) HIP tensors on one device");
  TORCH_CHECK(w.is_contiguous() && s->is_contiguous(), op, ": wq, s contiguous");
  if (W4) {
    TORCH_CHECK(N % 4 == 0 && K % 32 == 0, op, ": N % 4 == 0 and K % 32 == 0 (got N = ", N, ", K = ", K, ")");
  } else {
    TORCH_CHECK(N % 128 == 0 && K % 128 == 0, op, ": N % 128 == 0 and K % 128 == 0 (got N = ", N, ", K = ", K, ")");
  }
  const int64_t sn = W4 ? N : N / 128, sk = W4 ? K / 32 : K / 128;
  TORCH_CHECK(s->dim() == lead + 2 && s->size(lead) == sn && s->size(lead + 1) == sk &&
                  (lead == 0 || s->size(0) == w.size(0)),
              op, ": s must be [", (lead ? "E, " : ""), W4 ? "N, K/32]" : "N/128, K/128]");
  return K;
}

// x: bf16 [rows, K] on w's device, rows 16-byte aligned (K % 8 == 0 is the weight's check); grouped: contiguous
static void check_x(const char* op, const at::Tensor& x, const at::Tensor& w, int64_t K, int64_t lead) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.device() == w.device(), op,
              ": x must be a bf16 HIP tensor on w's device");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == K, op, ": x [rows, K], w [.., N, K]");
  TORCH_CHECK((lead ? x.is_contiguous() : x.stride(1) == 1 && x.stride(0) % 8 == 0) &&
                  ((uintptr_t)x.data_ptr() % 16) == 0,
              op, ": x rows must be 16-byte aligned", lead ? ", x contiguous" : "");
}

template <class F, int M>
static void launch_gemv(const at::Tensor& x, const at::Tensor& w, const at::Tensor* s, at::Tensor& y) {
  const int N = w.size(0), K = x.size(1);
  const auto xp = (const bf16*)x.data_ptr();
  const auto wp = (const typename F::elem*)w.data_ptr();
  const auto sp = s ? (const uint8_t*)s->data_ptr() : nullptr;
  const auto yp = (bf16*)y.data_ptr();
  if (N >= 8192)
    gemv_kernel<F, M, 4, F::U><<<cdiv(cdiv(N, 4), 4), 256, 0, stream()>>>(xp, wp, sp, yp, N, K, x.stride(0), w.stride(0));
  else
    gemv_kernel<F, M, 2, F::U><<<cdiv(cdiv(N, 2), 4), 256, 0, stream()>>>(xp, wp, sp, yp, N, K, x.stride(0), w.stride(0));
}

// x [M, K] bf16 (row stride ldx), w [N, K] (or its image wq + s) -> y [M, N] bf16; M <= 4
template <class F>
static at::Tensor gemv_op(const char* op, const at::Tensor& x, const at::Tensor& w, const at::Tensor* s) {
  const int K = check_weight<F>(op, w, s, 0);
  check_x(op, x, w, K, 0);
  const int M = x.size(0), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= 4, op, ": M must be 1..4");
  DeviceGuard g(x.device());
  auto y = at::empty({M, N}, x.options());
  if (N == 0 || K == 0) return K == 0 ? y.zero_() : y;
  switch (M) {
    case 1: launch_gemv<F, 1>(x, w, s, y); break;
    case 2: launch_gemv<F, 2>(x, w, s, y); break;
    case 3: launch_gemv<F, 3>(x, w, s, y); break;
    default: launch_gemv<F, 4>(x, w, s, y); break;
  }
  SPA_LAUNCH_CHECK();
  return y;
}

// x [A, K] expert-sorted rows, w [E, N, K] (or its image wq + s), offsets [E+1] (device) -> y [A, N]
template <class F>
static at::Tensor grouped_gemv_op(const char* op, const at::Tensor& x, const at::Tensor& w, const at::Tensor* s,
                                  const at::Tensor& offsets) {
  check_x(op, x, w, check_weight<F>(op, w, s, 1), 1);
  TORCH_CHECK(offsets.is_cuda() && offsets.device() == x.device() && offsets.scalar_type() == at::kInt &&
                  offsets.is_contiguous() && offsets.numel() == w.size(0) + 1,
              op, ": offsets int32 [E+1] on the device");
  const int A = x.size(0), K = x.size(1), E = w.size(0), N = w.size(1);
  DeviceGuard g(x.device());
  auto y = at::empty({A, N}, x.options());
  if (A == 0 || N == 0 || E == 0) return y;
  if (K == 0) return y.zero_();
  const int nwb = cdiv(cdiv(N, 2), 4);
  TORCH_CHECK((int64_t)E * nwb < (int64_t)1 << 31, op, ": grid too large");
  grouped_gemv_kernel<F, 2, F::UG><<<E * nwb, 256, 0, stream()>>>(
      (const bf16*)x.data_ptr(), (const typename F::elem*)w.data_ptr(), s ? (const uint8_t*)s->data_ptr() : nullptr,
      (bf16*)y.data_ptr(), offsets.data_ptr<int>(), N, K);
  SPA_LAUNCH_CHECK();
  return y;
}

at::Tensor gemv(const at::Tensor& x, const at::Tensor& w) { return gemv_op<WBf16>("gemv", x, w, nullptr); }
at::Tensor gemv_w8(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& s) {
  return gemv_op<WE4m3>("gemv_w8", x, wq, &s);
}
at::Tensor grouped_gemv(const at::Tensor& x, const at::Tensor& w, const at::Tensor& offsets) {
  return grouped_gemv_op<WBf16>("grouped_gemv", x, w, nullptr, offsets);
}
at::Tensor grouped_gemv_w8(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& s,
                           const at::Tensor& offsets) {
  return grouped_gemv_op<WE4m3>("grouped_gemv_w8", x, wq, &s, offsets);
}

at::Tensor gemv_w4(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& s) {
  return gemv_op<WMxfp4>("gemv_w4", x, wq, &s);
}
at::Tensor grouped_gemv_w4(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& s,
                           const at::Tensor& offsets) {
  return grouped_gemv_op<WMxfp4>("grouped_gemv_w4", x, wq, &s, offsets);
}

}  // namespace spa

TORCH_LIBRARY_FRAGMENT(spa, m) {
  m.def("gemv(Tensor x, Tensor w) -> Tensor");
  m.def("grouped_gemv(Tensor x, Tensor w, Tensor offsets) -> Tensor");
  m.def("gemv_w8(Tensor x, Tensor wq, Tensor s) -> Tensor");
  m.def("grouped_gemv_w8(Tensor x, Tensor wq, Tensor s, Tensor offsets) -> Tensor");
  m.def("gemv_w4(Tensor x, Tensor wq, Tensor s) -> Tensor");
  m.def("grouped_gemv_w4(Tensor x, Tensor wq, Tensor s, Tensor offsets) -> Tensor");
}
TORCH_LIBRARY_IMPL(spa, CUDA, m) {
  m.impl("gemv", &spa::gemv);
  m.impl("grouped_gemv", &spa::grouped_gemv);
  m.impl("gemv_w8", &spa::gemv_w8);
  m.impl("grouped_gemv_w8", &spa::grouped_gemv_w8);
  m.impl("gemv_w4", &spa::gemv_w4);
  m.impl("grouped_gemv_w4", &spa::grouped_gemv_w4);
}
