// Weight-only decode for one MFMA row tile: y[M, N] = bf16(x[M, K] @ dequant(W)[N, K]^T), 1 <= M <= 16,
// x / y bf16, fp32 accumulation, W the fp8 or MXFP4 decode image that gemv_w8 / gemv_w4 read (gemv.hip;
// no other copy of the weights). skinny_gemm_w8 and skinny_gemm_w4 are the two instantiations of ONE
// kernel over the weight-format policies of weight_formats.h. N % 128 == 0 and K % 128 == 0.
//
// Like the GEMV it is built for the weight stream, but the products run on v_mfma_f32_16x16x32_bf16:
//  * x is the A operand (lane l: token row l & 15, k-group l >> 4), W the B operand (lane l: weight row
//    l & 15, k-group l >> 4), so D holds y[4 (l >> 4) + i][n0 + (l & 15)] in register i;
//  * the k order inside a reduction is free as long as a lane's x fragment matches its W fragment, so a
//    lane takes ONE contiguous 16-byte piece of its weight row per step: 16 weights (e4m3) or 32 (MXFP4,
//    exactly one scale block), k = k0 + CH * (l >> 4) .. + CH - 1. A step is STEP = 4 CH k (64 / 128) of 16
//    rows; the conversion (WE4m3 / WMxfp4 ::prepare, exact in bf16, the block scale applied by the
//    conversion instruction) yields H = 2 / 4 MFMA operands, and the lane's x fragment is the same
//    CH consecutive k of its token row: 32 / 64 contiguous bytes;
//  * weights go straight to VGPRs, non-temporal, U steps x NT n-tiles of loads in flight before any is
//    consumed (cdna_hip_programming.md, 'GEMV / M <= 16'); no LDS round trip for W;
//  * a wave owns NT n-tiles (16 NT weight rows) and reuses each x fragment NT times from registers: x
//    comes from L2 at 1 KB per MFMA against 512 / 256 B of weights, so without reuse it would be 2-4 x the
//    HBM stream; with NT = 4 it is 0.5-1 x, with NT = 2 1-2 x;
//  * token rows >= M are never read (their lanes read row M - 1 again: rows of D are independent, so what
//    they hold reaches no stored value) and never stored.
//
// Decomposition (skinny_plan, a function of N and K ONLY, so that y[:m] of a 16-row call is bitwise the
// m-row call, and a row never depends on its neighbours):
//  * a block is 4 waves that share 16 NT weight rows and split the block's K range four ways; NT = 2 for
//    N < 8192 (o-proj, down-proj, qkv), else 4, as the GEMV's RW;
//  * narrow outputs also split K over gridDim.y = S blocks: S = ceil(512 / (N / 16 NT)), so that the grid
//    holds >= 512 blocks = 2 waves per SIMD on 256 CUs, capped so that every wave keeps >= 2 of the K / 128
//    scale blocks (S <= K / 1024). LLaMA3-8B: qkv (6144 x 4096) 192 x 3, o (4096 x 4096) 128 x 4, gate/up
//    (28672 x 4096) 448 x 2, down (4096 x 14336) 128 x 4, LM head (128256 x 4096) 2004 x 1;
//  * the 4 S slices are runs of whole 128-k scale blocks: slice i is blocks [i nb / 4S, (i + 1) nb / 4S);
//  * sums are deterministic: a wave adds its MFMAs in ascending k; wave 0 adds the four waves' fp32 tiles
//    in wave order through LDS; with S > 1 the block tiles go to an fp32 workspace [S, M, N] (from the
//    caching allocator: capturable) and skinny_merge_kernel adds them in ascending s. No atomics.
#include "spa_common.h"
#include "weight_formats.h"

SPA_DEBUG_TU("skinny_gemm.hip")

namespace spa {

constexpr int SKINNY_MAX_ROWS = 16;
constexpr int SKINNY_WAVES = 4;         // waves of a block = K slices of a block
constexpr int SKINNY_MIN_BLOCKS = 512;  // blocks wanted in the grid: 2 per CU
constexpr int SKINNY_MIN_KB = 2;        // 128-k scale blocks a wave keeps at least when K is split over blocks

// steps in flight per wave: 4 x 64 k (e4m3) or 2 x 128 k (MXFP4) = 256 k = SKINNY_MIN_KB scale blocks
template <class F> constexpr int skinny_u() { return F::ROW_SCALES ? 2 : 4; }

template <class F, int NT, int U>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(const bf16* __restrict__ x,
                                                          const typename F::elem* __restrict__ w,
                                                          const uint8_t* __restrict__ s, bf16* __restrict__ y,
                                                          float* __restrict__ part, int M, int N, int K, long ldx) {
  using raw = typename F::raw;
  constexpr int CH = 8 * F::H, STEP = 4 * CH, SH = F::SH;  // weights per lane and load / per 16 rows and step
  constexpr int SR = F::ROW_SCALES ? NT : 1;               // scale bytes per lane and step
  __shared__ f32x4 red[SKINNY_WAVES - 1][NT][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * NT);
  const int nb = K >> 7, slices = gridDim.y * SKINNY_WAVES, sl = blockIdx.y * SKINNY_WAVES + wave;
  const int kb = (int)((long)sl * nb / slices) << 7, ke = (int)((long)(sl + 1) * nb / slices) << 7;
  const int m = min(col, M - 1);  // rows past M: row M - 1 again, never stored
  SPA_DBG_CHECK(m, M);
  const bf16* xr = x + (long)m * ldx + CH * g;
  const typename F::elem* wr[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    SPA_DBG_CHECK(n0 + 16 * t + col, N);
    wr[t] = w + (long)(n0 + 16 * t + col) * (K >> SH) + ((CH * g) >> SH);
  }
  const uint8_t* sr = F::scale_row(s, 0, N, F::ROW_SCALES ? n0 + col : n0, K);
  auto load = [&](const int t, const int k) {
    SPA_DBG_CHECK(k + CH * g + CH - 1, K);
    return __builtin_nontemporal_load(reinterpret_cast<const raw*>(wr[t] + (k >> SH)));
  };
  // the scale byte of n-tile t's chunk at step k (+ ahead): per lane for MXFP4, one per wave for e4m3
  auto scale = [&](const int t, const int k, const int ahead) {
    SPA_DBG_CHECK(F::ROW_SCALES ? (long)(n0 + 16 * t + col) * (K >> 5) + ((k + ahead) >> 5) + g
                                : (long)(n0 >> 7) * (K >> 7) + ((k + ahead) >> 7),
                  F::ROW_SCALES ? (long)N * (K >> 5) : (long)(N >> 7) * (K >> 7));
    return F::scale(sr, 16 * t, K, F::ROW_SCALES ? k + CH * g : k, ahead);
  };
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto consume = [&](const int k, const raw* wv, const uint8_t* sc) {
    bf16x8 xv[F::H];
#pragma unroll
    for (int h = 0; h < F::H; ++h) xv[h] = *reinterpret_cast<const bf16x8*>(xr + k + 8 * h);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      bf16x8 wp[F::H];
      F::prepare(wv[t], sc[F::ROW_SCALES ? t : 0], wp);
#pragma unroll
      for (int h = 0; h < F::H; ++h) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xv[h], wp[h], acc[t], 0, 0, 0);
    }
  };
  int k = kb;
  for (; k + U * STEP <= ke; k += U * STEP) {
    raw wv[U][NT];
    uint8_t sc[U][SR];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int t = 0; t < NT; ++t) wv[u][t] = load(t, k + u * STEP);
#pragma unroll
      for (int t = 0; t < SR; ++t) sc[u][t] = scale(t, k, u * STEP);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) consume(k + u * STEP, wv[u], sc[u]);
  }
  for (; k < ke; k += STEP) {
    raw wv[NT];
    uint8_t sc[SR];
#pragma unroll
    for (int t = 0; t < NT; ++t) wv[t] = load(t, k);
#pragma unroll
    for (int t = 0; t < SR; ++t) sc[t] = scale(t, k, 0);
    consume(k, wv, sc);
  }
  // the block's tile: wave 0 + wave 1 + wave 2 + wave 3, in that order
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) red[wave - 1][t][lane] = acc[t];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4 v = acc[t];
#pragma unroll
    for (int q = 0; q < SKINNY_WAVES - 1; ++q) v += red[q][t][lane];
    const int n = n0 + 16 * t + col;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int mm = 4 * g + i;
      if (mm < M && SPA_DBG_OK((long)mm * N + n, (long)M * N)) {
        if (part)
          part[((long)blockIdx.y * M + mm) * N + n] = v[i];
        else
          y[(long)mm * N + n] = (bf16)v[i];
      }
    }
  }
}

// y = bf16(part[0] + part[1] + .. + part[S - 1]), ascending; part fp32 [S, MN], MN % 4 == 0
__global__ __launch_bounds__(256) void skinny_merge_kernel(const float* __restrict__ part, bf16* __restrict__ y, int S,
                                                           long MN) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  SPA_DBG_CHECK(i + 3, MN);
  f32x4 v = *reinterpret_cast<const f32x4*>(part + i);
  for (int q = 1; q < S; ++q) v += *reinterpret_cast<const f32x4*>(part + q * MN + i);
  bf16x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (bf16)v[j];
  *reinterpret_cast<bf16x4*>(y + i) = o;
}

// The decomposition of an [N, K] product (head of this file): n-tiles per wave and K splits over blocks.
// It may depend on N and K only, never on M: rows must not see how many neighbours they have.
static void skinny_plan(int64_t N, int64_t K, int& NT, int& S) {
  NT = N < 8192 ? 2 : 4;
  const int64_t blocks = N / (16 * NT), nb = K >> 7;
  S = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(SKINNY_MIN_BLOCKS, blocks), nb / (SKINNY_WAVES * SKINNY_MIN_KB)));
}

template <class F>
static at::Tensor skinny_gemm_op(const char* op, const at::Tensor& x, const at::Tensor& wq, const at::Tensor& s) {
  constexpr bool W4 = F::ROW_SCALES;
  TORCH_CHECK(x.is_cuda() && wq.is_cuda() && s.is_cuda() && x.device() == wq.device() && s.device() == wq.device(), op,
              ": x, wq, s must be HIP tensors on one device");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && wq.scalar_type() == (W4 ? at::kByte : at::kFloat8_e4m3fn) &&
                  s.scalar_type() == at::kByte,
              op, ": x bf16, wq ", W4 ? "uint8 (two e2m1 codes per byte)" : "float8_e4m3fn", ", s uint8 (E8M0)");
  TORCH_CHECK(x.dim() == 2 && wq.dim() == 2 && s.dim() == 2, op, ": x [M, K], wq [N, K", W4 ? " / 2" : "", "], s 2-D");
  TORCH_CHECK(wq.is_contiguous() && s.is_contiguous() && ((uintptr_t)wq.data_ptr() % 16) == 0, op,
              ": wq, s contiguous, wq 16-byte aligned");
  const int64_t M = x.size(0), N = wq.size(0), K = wq.size(1) << F::SH;
  TORCH_CHECK(M >= 1 && M <= SKINNY_MAX_ROWS, op, ": M must be 1..16 (got ", M, ")");
  TORCH_CHECK(N < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && N % 128 == 0 && K % 128 == 0, op,
              ": N % 128 == 0 and K % 128 == 0 (got N = ", N, ", K = ", K, ")");
  TORCH_CHECK(x.size(1) == K, op, ": x [M, K] and the image disagree on K (", x.size(1), " vs ", K, ")");
  TORCH_CHECK(s.size(0) == (W4 ? N : N / 128) && s.size(1) == (W4 ? K / 32 : K / 128), op, ": s must be [",
              W4 ? "N, K/32]" : "N/128, K/128]");
  TORCH_CHECK(x.stride(1) == 1 && x.stride(0) % 8 == 0 && ((uintptr_t)x.data_ptr() % 16) == 0, op,
              ": x rows must be contiguous and 16-byte aligned");
  DeviceGuard guard(x.device());
  auto y = at::empty({M, N}, x.options());
  if (N == 0 || K == 0) return K == 0 ? y.zero_() : y;
  int NT, S;
  skinny_plan(N, K, NT, S);
  at::Tensor part;
  if (S > 1) part = at::empty({S, M, N}, x.options().dtype(at::kFloat));
  const dim3 grid((unsigned)(N / (16 * NT)), (unsigned)S);
  const auto xp = (const bf16*)x.data_ptr();
  const auto wp = (const typename F::elem*)wq.data_ptr();
  const auto sp = (const uint8_t*)s.data_ptr();
  const auto yp = (bf16*)y.data_ptr();
  float* pp = S > 1 ? part.data_ptr<float>() : nullptr;
  constexpr int U = skinny_u<F>();
  if (NT == 2)
    skinny_gemm_kernel<F, 2, U><<<grid, 256, 0, stream()>>>(xp, wp, sp, yp, pp, (int)M, (int)N, (int)K, x.stride(0));
  else
    skinny_gemm_kernel<F, 4, U><<<grid, 256, 0, stream()>>>(xp, wp, sp, yp, pp, (int)M, (int)N, (int)K, x.stride(0));
  SPA_LAUNCH_CHECK();
  if (S > 1) {
    const long MN = M * N;
    skinny_merge_kernel<<<cdiv(MN, 1024), 256, 0, stream()>>>(pp, yp, S, MN);
    SPA_LAUNCH_CHECK();
  }
  return y;
}

at::Tensor skinny_gemm_w8(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& s) {
  return skinny_gemm_op<WE4m3>("skinny_gemm_w8", x, wq, s);
}
at::Tensor skinny_gemm_w4(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& s) {
  return skinny_gemm_op<WMxfp4>("skinny_gemm_w4", x, wq, s);
}

}  // namespace spa

TORCH_LIBRARY_FRAGMENT(spa, m) {
  m.def("skinny_gemm_w8(Tensor x, Tensor wq, Tensor s) -> Tensor");
  m.def("skinny_gemm_w4(Tensor x, Tensor wq, Tensor s) -> Tensor");
}
TORCH_LIBRARY_IMPL(spa, CUDA, m) {
  m.impl("skinny_gemm_w8", &spa::skinny_gemm_w8);
  m.impl("skinny_gemm_w4", &spa::skinny_gemm_w4);
}
