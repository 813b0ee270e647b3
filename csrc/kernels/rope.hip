// Rotary position embedding, applied in place on the q/k heads of a fused
// [B, T, NH, hd] projection buffer (NH = H + 2*Hkv for a packed qkv), so no
// split/transpose copy is ever made. Backward = the same kernel with the
// inverse rotation (sin negated) on the incoming gradient.
//
// Reference: llama3/LLaMA-jax.ipynb:563-601 (precompute_freqs_cis / apply_rotary_emb:
// interleaved pairs (x[2i], x[2i+1]) rotated by t*theta^(-2i/hd)). A non-interleaved
// "rotate_half" layout is also provided (pairs (x[i], x[i+hd/2])).
//
// Layout: each thread owns 8 contiguous bf16 of one head row (16-byte load/store);
// cos/sin come from an fp32 table [Tmax, hd/2] (L2/LLC resident).
#include "spa_common.h"
#include "fp8_quant.h"
#include "paged_kv.h"
#include <type_traits>

SPA_DEBUG_TU("rope.hip")

namespace spa {

// MODE 0: interleaved pairs (x[2i], x[2i+1]) rotated (LLaMA-jax);
// MODE 1: rotate_half pairs (x[i], x[i+hd/2]);
// MODE 2: Gemma-ref quirk (gemma/gemma.ipynb:182-200: per-position dense matrix with
//         2x2 blocks [[cos, cos], [-sin, sin]], NOT a rotation) applied elementwise:
//         y_e = c (x_e + x_o), y_o = s (x_o - x_e); "inverse" applies the transpose
//         (the exact backward of the forward map).
template <typename DT, int MODE>
__global__ __launch_bounds__(256) void rope_kernel(DT* __restrict__ x, const float* __restrict__ cosT,
                                                   const float* __restrict__ sinT, const int* __restrict__ pos,
                                                   long sb, long st, long sh, int B, int T, int nrot, int hd,
                                                   int pos_off, float sign) {
  const int vpr = hd / 8;                 // vectors per head row
  const long total = (long)B * T * nrot * vpr;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int v = i % vpr;
    long r = i / vpr;
    const int hh = r % nrot;
    r /= nrot;
    const int t = r % T;
    const int b = r / T;
    const int ps = pos ? pos[b * T + t] : t + pos_off;
    DT* p = x + b * sb + t * st + hh * sh;
    const float* c = cosT + (long)ps * (hd / 2);
    const float* s = sinT + (long)ps * (hd / 2);
    if constexpr (MODE == 0 || MODE == 2) {
      float a[8];
      load8(p + v * 8, a);
      const f32x4 cv = *reinterpret_cast<const f32x4*>(c + v * 4);
      const f32x4 sv = *reinterpret_cast<const f32x4*>(s + v * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float x0 = a[2 * k], x1 = a[2 * k + 1];
        const float cs = cv[k];
        if constexpr (MODE == 0) {
          const float sn = sign * sv[k];
          a[2 * k] = x0 * cs - x1 * sn;
          a[2 * k + 1] = x0 * sn + x1 * cs;
        } else if (sign > 0.f) {   // forward: [[c, c], [-s, s]] x
          a[2 * k] = cs * (x0 + x1);
          a[2 * k + 1] = sv[k] * (x1 - x0);
        } else {                   // transpose: [[c, -s], [c, s]] dy
          a[2 * k] = cs * x0 - sv[k] * x1;
          a[2 * k + 1] = cs * x0 + sv[k] * x1;
        }
      }
      store8(p + v * 8, a);
    } else {
      // rotate_half: thread v < vpr/2 handles elements [8v, 8v+8) and their partners at +hd/2
      if (v >= vpr / 2) continue;
      float a[8], bq[8];
      load8(p + v * 8, a);
      load8(p + hd / 2 + v * 8, bq);
      float cv[8], sv[8];
      load8(c + v * 8, cv);
      load8(s + v * 8, sv);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float x0 = a[k], x1 = bq[k], sn = sign * sv[k];
        a[k] = x0 * cv[k] - x1 * sn;
        bq[k] = x0 * sn + x1 * cv[k];
      }
      store8(p + v * 8, a);
      store8(p + hd / 2 + v * 8, bq);
    }
  }
}

// x: [B, T, NH, hd] view (hd contiguous), rotates heads [0, nrot). In place.
void rope_(const at::Tensor& x, const at::Tensor& cos, const at::Tensor& sin, const c10::optional<at::Tensor>& pos,
           int64_t nrot, int64_t pos_off, int64_t mode, bool inverse) {
  SPA_CHECK_CUDA(x);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat, "rope: bf16/fp32");
  TORCH_CHECK(x.dim() == 4 && x.stride(3) == 1, "rope: x must be [B,T,NH,hd] with contiguous hd");
  const int B = x.size(0), T = x.size(1), hd = x.size(3);
  TORCH_CHECK(hd % 16 == 0, "rope: hd must be a multiple of 16");
  TORCH_CHECK(nrot <= x.size(2));
  TORCH_CHECK(cos.scalar_type() == at::kFloat && cos.is_contiguous() && sin.is_contiguous() && cos.size(1) == hd / 2);
  TORCH_CHECK(x.stride(1) % 8 == 0 && x.stride(2) % 8 == 0 && x.stride(0) % 8 == 0 && (uintptr_t)x.data_ptr() % 16 == 0);
  if (pos) { TORCH_CHECK(pos->scalar_type() == at::kInt && pos->is_contiguous() && pos->numel() == (int64_t)B * T); }
  else { TORCH_CHECK(pos_off + T <= cos.size(0), "rope: table too short"); }
  DeviceGuard g(x.device());
  const long total = (long)B * T * nrot * (hd / 8);
  if (total == 0) return;
  const int grid = (int)std::min<long>((total + 255) / 256, 4096);
  auto st = stream();
  const float sign = inverse ? -1.f : 1.f;
  auto launch = [&](auto modec) {
    constexpr int M = decltype(modec)::value;
    if (x.scalar_type() == at::kBFloat16)
      rope_kernel<bf16, M><<<grid, 256, 0, st>>>((bf16*)x.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(),
                                                 pos ? pos->data_ptr<int>() : nullptr, x.stride(0), x.stride(1),
                                                 x.stride(2), B, T, (int)nrot, hd, (int)pos_off, sign);
    else
      rope_kernel<float, M><<<grid, 256, 0, st>>>(x.data_ptr<float>(), cos.data_ptr<float>(), sin.data_ptr<float>(),
                                                  pos ? pos->data_ptr<int>() : nullptr, x.stride(0), x.stride(1),
                                                  x.stride(2), B, T, (int)nrot, hd, (int)pos_off, sign);
  };
  if (mode == 0) launch(std::integral_constant<int, 0>{});
  else if (mode == 1) launch(std::integral_constant<int, 1>{});
  else if (mode == 2) launch(std::integral_constant<int, 2>{});
  else TORCH_CHECK(false, "rope: mode must be 0, 1 or 2");
  SPA_LAUNCH_CHECK();
}

// Decode-step prologue in one launch: for a packed qkv buffer [B, T, H + 2 Hkv, hd], rotate
// the q heads in place, rotate the k heads into the KV cache and copy the v heads into it, at
// cache row *index + t. MODE 0: interleaved pairs (LLaMA), MODE 1: rotate_half (Gemma). The
// row and the RoPE positions are read from device memory, so a captured hipGraph replays it
// at every position (replaces rope_ + two index_copy_ launches per layer). Rows past the
// cache end are dropped.
//
// Paged cache (rope_kv_write_paged_, infer/cache.py PagedKVCache): kc / vc are page pools [num_pages,
// page_size, Hkv, hd], Tmax is the table's NP * page_size logical rows, and logical row r of sequence b
// goes to pool row bt[b, r >> lg] * page_size + (r & (page_size - 1)). A row outside [0, Tmax) is dropped
// before the table is read; an unreserved row's entry is 0, the null page, which nothing valid reads
// (paged_kv.h).
struct NoTable {};

// PAGED: the k / v destination row comes through the block table (tb; kct / vct are the pool-row stride,
// kcb / vcb unused); the q-head rotation and all arithmetic are the same source, and PAGED = false
// compiles to what it was before the flag.
template <int MODE, bool PAGED = false>
__global__ __launch_bounds__(256) void rope_kv_write_kernel(bf16* __restrict__ x, const float* __restrict__ cosT,
                                                            const float* __restrict__ sinT,
                                                            const int* __restrict__ pos,
                                                            const long* __restrict__ index, bf16* __restrict__ kc,
                                                            bf16* __restrict__ vc, long sb, long st, long sh,
                                                            long kcb, long kct, long kch, long vcb, long vct,
                                                            long vch, int B, int T, int H, int Hkv, int hd,
                                                            int Tmax, bool per_row,
                                                            std::conditional_t<PAGED, PagedTable, NoTable> tb) {
  const int vpr = hd / 8;
  const int NH = H + 2 * Hkv;
  const long total = (long)B * T * NH * vpr;
  const long row0 = *index;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int v = i % vpr;
    long r = i / vpr;
    const int hh = r % NH;
    r /= NH;
    const int t = r % T;
    const int b = r / T;
    SPA_DBG_CHECK(b, B);  // the per-row index read (debug build)
    const long row = (per_row ? index[b] : row0) + t;  // ragged batch: each sequence's own cache row
    if (hh >= H && (row >= Tmax || row < 0)) continue;
    if (hh >= H && !SPA_DBG_OK(row, Tmax)) continue;
    long cb = b, crow = row;  // cache batch and row of a k / v head
    if constexpr (PAGED) {
      cb = 0;
      if (hh >= H) {  // row is inside [0, NP * page_size): the table index is inside the table
        crow = paged_pool_row(tb, paged_page(tb, b, row), row);
      }
    }
    const bf16* src = x + b * sb + t * st + hh * sh;
    bf16* dst = hh < H ? x + b * sb + t * st + hh * sh
                       : (hh < H + Hkv ? kc + cb * kcb + crow * kct + (hh - H) * kch
                                       : vc + cb * vcb + crow * vct + (hh - H - Hkv) * vch);
    float a[8];
    if (hh >= H + Hkv) {  // v: plain copy into the cache
      load8(src + v * 8, a);
      store8(dst + v * 8, a);
      continue;
    }
    const int ps = pos[b * T + t];
    const float* c = cosT + (long)ps * (hd / 2);
    const float* s = sinT + (long)ps * (hd / 2);
    if constexpr (MODE == 0) {
      load8(src + v * 8, a);
      const f32x4 cv = *reinterpret_cast<const f32x4*>(c + v * 4);
      const f32x4 sv = *reinterpret_cast<const f32x4*>(s + v * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float x0 = a[2 * k], x1 = a[2 * k + 1];
        a[2 * k] = x0 * cv[k] - x1 * sv[k];
        a[2 * k + 1] = x0 * sv[k] + x1 * cv[k];
      }
      store8(dst + v * 8, a);
    } else {  // rotate_half: thread v < vpr/2 owns elements [8v, 8v+8) and their partners at +hd/2
      if (v >= vpr / 2) continue;
      float bq[8], cv[8], sv[8];
      load8(src + v * 8, a);
      load8(src + hd / 2 + v * 8, bq);
      load8(c + v * 8, cv);
      load8(s + v * 8, sv);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float x0 = a[k], x1 = bq[k];
        a[k] = x0 * cv[k] - x1 * sv[k];
        bq[k] = x0 * sv[k] + x1 * cv[k];
      }
      store8(dst + v * 8, a);
      store8(dst + hd / 2 + v * 8, bq);
    }
  }
}

void rope_kv_write_(const at::Tensor& x, const at::Tensor& cos, const at::Tensor& sin, const at::Tensor& pos,
                    const at::Tensor& index, const at::Tensor& kc, const at::Tensor& vc, int64_t H, int64_t Hkv,
                    int64_t mode, bool per_row) {
  for (auto* t : {&x, &kc, &vc}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 && t->dim() == 4 && t->stride(3) == 1,
                "rope_kv_write: bf16 [B, T, heads, hd] tensors with contiguous hd");
    TORCH_CHECK(t->stride(0) % 8 == 0 && t->stride(1) % 8 == 0 && t->stride(2) % 8 == 0 &&
                    (uintptr_t)t->data_ptr() % 16 == 0,
                "rope_kv_write: 16-byte aligned rows");
  }
  const int B = x.size(0), T = x.size(1), hd = x.size(3);
  TORCH_CHECK(x.size(2) == H + 2 * Hkv && hd % 16 == 0, "rope_kv_write: x must be packed [B, T, H + 2 Hkv, hd]");
  TORCH_CHECK(kc.size(0) == B && vc.size(0) == B && kc.size(2) == Hkv && vc.size(2) == Hkv && kc.size(3) == hd &&
                  vc.size(3) == hd && vc.size(1) == kc.size(1),
              "rope_kv_write: cache shape mismatch");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && cos.is_contiguous() && sin.is_contiguous() && cos.size(1) == hd / 2,
              "rope_kv_write: fp32 [Tmax, hd/2] tables");
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kInt && pos.is_contiguous() && pos.numel() == (int64_t)B * T,
              "rope_kv_write: pos must be device int32 [B, T]");
  TORCH_CHECK(index.is_cuda() && index.scalar_type() == at::kLong && index.numel() >= 1,
              "rope_kv_write: index must be a device int64 tensor");
  TORCH_CHECK(!per_row || (index.numel() == B && index.is_contiguous()),
              "rope_kv_write: per_row needs one index per sequence (", B, "), got ", index.numel());
  TORCH_CHECK(mode == 0 || mode == 1, "rope_kv_write: mode 0 (interleaved) or 1 (rotate_half)");
  DeviceGuard g(x.device());
  const long total = (long)B * T * (H + 2 * Hkv) * (hd / 8);
  if (total == 0) return;
  const int grid = (int)std::min<long>((total + 255) / 256, 4096);
  auto launch = [&](auto modec) {
    constexpr int M = decltype(modec)::value;
    rope_kv_write_kernel<M><<<grid, 256, 0, stream()>>>(
        (bf16*)x.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), pos.data_ptr<int>(),
        index.data_ptr<int64_t>(), (bf16*)kc.data_ptr(), (bf16*)vc.data_ptr(), x.stride(0), x.stride(1),
        x.stride(2), kc.stride(0), kc.stride(1), kc.stride(2), vc.stride(0), vc.stride(1), vc.stride(2), B, T,
        (int)H, (int)Hkv, hd, (int)kc.size(1), per_row, NoTable{});
  };
  if (mode == 0) launch(std::integral_constant<int, 0>{});
  else launch(std::integral_constant<int, 1>{});
  SPA_LAUNCH_CHECK();
}

// rope_kv_write_ into a paged cache: kpool / vpool bf16 [num_pages, page_size, Hkv, hd], block_table
// int32 [B, NP]. Logical rows outside [0, NP * page_size) are dropped; rows a sequence has not reserved
// land in the null page.
void rope_kv_write_paged_(const at::Tensor& x, const at::Tensor& cos, const at::Tensor& sin, const at::Tensor& pos,
                          const at::Tensor& index, const at::Tensor& kpool, const at::Tensor& vpool,
                          const at::Tensor& block_table, int64_t H, int64_t Hkv, int64_t mode, bool per_row) {
  for (auto* t : {&x, &kpool, &vpool}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 && t->dim() == 4 && t->stride(3) == 1,
                "rope_kv_write_paged: bf16 x [B, T, heads, hd] and pools [num_pages, page_size, Hkv, hd], contiguous hd");
    TORCH_CHECK(t->stride(0) % 8 == 0 && t->stride(1) % 8 == 0 && t->stride(2) % 8 == 0 &&
                    (uintptr_t)t->data_ptr() % 16 == 0,
                "rope_kv_write_paged: 16-byte aligned rows");
  }
  const int B = x.size(0), T = x.size(1), hd = x.size(3);
  TORCH_CHECK(x.size(2) == H + 2 * Hkv && hd % 16 == 0, "rope_kv_write_paged: x must be packed [B, T, H + 2 Hkv, hd]");
  const int64_t num_pages = kpool.size(0), page = kpool.size(1);
  TORCH_CHECK(page >= 16 && page <= 256 && (page & (page - 1)) == 0,
              "rope_kv_write_paged: page_size must be a power of two in [16, 256], got ", page);
  TORCH_CHECK(vpool.sizes() == kpool.sizes() && kpool.size(2) == Hkv && kpool.size(3) == hd && num_pages >= 1,
              "rope_kv_write_paged: pool shape mismatch");
  TORCH_CHECK(kpool.stride(0) == page * kpool.stride(1) && vpool.stride(0) == page * vpool.stride(1),
              "rope_kv_write_paged: a pool's pages must be back to back (stride(0) == page_size * stride(1))");
  TORCH_CHECK(block_table.is_cuda() && block_table.device() == x.device() && kpool.device() == x.device() &&
                  vpool.device() == x.device() && block_table.scalar_type() == at::kInt && block_table.dim() == 2 &&
                  block_table.size(0) == B && block_table.is_contiguous(),
              "rope_kv_write_paged: block_table must be a contiguous int32 [B, NP] tensor on x's device");
  const int64_t NP = block_table.size(1);
  TORCH_CHECK(NP * page < (1L << 31) && num_pages * page < (1L << 31), "rope_kv_write_paged: rows must fit an int32");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && cos.is_contiguous() && sin.is_contiguous() && cos.size(1) == hd / 2,
              "rope_kv_write_paged: fp32 [Tmax, hd/2] tables");
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kInt && pos.is_contiguous() && pos.numel() == (int64_t)B * T,
              "rope_kv_write_paged: pos must be device int32 [B, T]");
  TORCH_CHECK(index.is_cuda() && index.scalar_type() == at::kLong && index.numel() >= 1,
              "rope_kv_write_paged: index must be a device int64 tensor");
  TORCH_CHECK(!per_row || (index.numel() == B && index.is_contiguous()),
              "rope_kv_write_paged: per_row needs one index per sequence (", B, "), got ", index.numel());
  TORCH_CHECK(mode == 0 || mode == 1, "rope_kv_write_paged: mode 0 (interleaved) or 1 (rotate_half)");
  DeviceGuard g(x.device());
  const long total = (long)B * T * (H + 2 * Hkv) * (hd / 8);
  if (total == 0) return;
  const int grid = (int)std::min<long>((total + 255) / 256, 4096);
  int lg = 0;
  while ((1 << lg) < page) ++lg;
  const PagedTable tb{block_table.data_ptr<int>(), (int)NP, lg, (int)num_pages};
  auto launch = [&](auto modec) {
    constexpr int M = decltype(modec)::value;
    rope_kv_write_kernel<M, true><<<grid, 256, 0, stream()>>>(
        (bf16*)x.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), pos.data_ptr<int>(),
        index.data_ptr<int64_t>(), (bf16*)kpool.data_ptr(), (bf16*)vpool.data_ptr(), x.stride(0), x.stride(1),
        x.stride(2), 0L, kpool.stride(1), kpool.stride(2), 0L, vpool.stride(1), vpool.stride(2), B, T, (int)H,
        (int)Hkv, hd, (int)(NP * page), per_row, tb);
  };
  if (mode == 0) launch(std::integral_constant<int, 0>{});
  else launch(std::integral_constant<int, 1>{});
  SPA_LAUNCH_CHECK();
}

// ------------------------------------------------------------------ fp8 KV cache writers
// Cache format (infer/cache.py, quant="fp8"): K and V rows as OCP e4m3 bytes [B, Tmax, Hkv, hd] (the
// bf16 cache's layout) plus one E8M0 scale byte per (batch, kv head, token) in [B, Hkv, Tmax]; a row
// is x ~= q * 2^(s - 127) with the fp8_quant.h scale choice over the row's hd values. What is quantised
// is the bf16 value the bf16 cache would hold, so "fp8 cache == torch-quantise(bf16 cache)" bitwise.
struct KV8Dst {
  uint8_t* q; uint8_t* s;
  long qb, qt, qh;  // byte strides of the e4m3 rows (hd contiguous)
  long sb, sh;      // scale strides (token contiguous)
};

// Eager write: bf16 k / v [B, T, Hkv, hd] (strided views of the packed qkv buffer) into cache rows
// [pos, pos + T). hd / 8 adjacent lanes own one (k|v, b, t, head) row: 8 values each, amax by
// shuffles inside the lane group, then the scale, the bytes and the scale byte; the row is read once.
__global__ __launch_bounds__(256) void kv_quant_write_kernel(const bf16* __restrict__ k, const bf16* __restrict__ v,
                                                             KV8Dst kd, KV8Dst vd, long skb, long skt, long skh,
                                                             long svb, long svt, long svh, int B, int T, int Hkv,
                                                             int hd, int pos, int Tmax) {
  const int vpr = hd / 8;  // lanes per row: a power of two <= 64, so a lane group never straddles a wave
  const long total = 2L * B * T * Hkv * vpr;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int l = i % vpr;
    long r = i / vpr;
    const int h = r % Hkv;
    r /= Hkv;
    const int t = r % T;
    r /= T;
    const int b = r % B;
    const bool isv = r / B != 0;
    const bf16* src = isv ? v + b * svb + t * svt + h * svh : k + b * skb + t * skt + h * skh;
    const KV8Dst& d = isv ? vd : kd;
    float a[8];
    load8(src + l * 8, a);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(a[j]));
    for (int o = 1; o < vpr; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const int e = e8m0_exp(amax);
    const long row = (long)pos + t;
    if (SPA_DBG_OK(row, Tmax)) {
      *reinterpret_cast<int2*>(d.q + b * d.qb + row * d.qt + h * d.qh + l * 8) = q8(a, e8m0_inv(e));
      if (l == 0 && SPA_DBG_OK(h * (long)Tmax + row, (long)Hkv * Tmax)) d.s[b * d.sb + h * d.sh + row] = (uint8_t)(e + 127);
    }
  }
}

// e4m3 data [B, Tmax, Hkv, hd] + E8M0 scales [B, Hkv, Tmax] of one cache side, checked
static KV8Dst kv8_dst(const at::Tensor& q, const at::Tensor& s, int64_t B, int64_t Hkv, int64_t hd, const char* op) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kFloat8_e4m3fn && q.dim() == 4 && q.stride(3) == 1,
              op, ": cache data must be float8_e4m3fn [B, Tmax, Hkv, hd] with contiguous hd");
  TORCH_CHECK(q.size(0) == B && q.size(2) == Hkv && q.size(3) == hd, op, ": cache shape mismatch");
  TORCH_CHECK(q.stride(0) % 8 == 0 && q.stride(1) % 8 == 0 && q.stride(2) % 8 == 0 && (uintptr_t)q.data_ptr() % 8 == 0,
              op, ": 8-byte aligned cache rows");
  TORCH_CHECK(s.is_cuda() && s.scalar_type() == at::kByte && s.dim() == 3 && s.size(0) == B && s.size(1) == Hkv &&
                  s.size(2) == q.size(1) && s.stride(2) == 1,
              op, ": scales must be uint8 [B, Hkv, Tmax], token-contiguous");
  return KV8Dst{(uint8_t*)q.data_ptr(), (uint8_t*)s.data_ptr(), q.stride(0), q.stride(1), q.stride(2), s.stride(0),
                s.stride(1)};
}

void kv_quant_write_(const at::Tensor& k, const at::Tensor& v, const at::Tensor& kq, const at::Tensor& ks,
                     const at::Tensor& vq, const at::Tensor& vs, int64_t pos) {
  for (auto* t : {&k, &v}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 && t->dim() == 4 && t->stride(3) == 1,
                "kv_quant_write: bf16 [B, T, Hkv, hd] k / v with contiguous hd");
    TORCH_CHECK(t->stride(0) % 8 == 0 && t->stride(1) % 8 == 0 && t->stride(2) % 8 == 0 &&
                    (uintptr_t)t->data_ptr() % 16 == 0,
                "kv_quant_write: 16-byte aligned rows");
  }
  const int B = k.size(0), T = k.size(1), Hkv = k.size(2), hd = k.size(3);
  TORCH_CHECK(v.sizes() == k.sizes(), "kv_quant_write: k / v shape mismatch");
  TORCH_CHECK(hd >= 8 && hd <= 512 && (hd & (hd - 1)) == 0, "kv_quant_write: hd must be a power of two in [8, 512]");
  const KV8Dst kd = kv8_dst(kq, ks, B, Hkv, hd, "kv_quant_write"), vd = kv8_dst(vq, vs, B, Hkv, hd, "kv_quant_write");
  const int Tmax = kq.size(1);
  TORCH_CHECK(vq.size(1) == Tmax, "kv_quant_write: cache shape mismatch");
  TORCH_CHECK(pos >= 0 && pos + T <= Tmax, "kv_quant_write: rows [", pos, ", ", pos + T, ") outside a ", Tmax, "-row cache");
  DeviceGuard g(k.device());
  const long total = 2L * B * T * Hkv * (hd / 8);
  if (total == 0) return;
  const int grid = (int)std::min<long>((total + 255) / 256, 4096);
  kv_quant_write_kernel<<<grid, 256, 0, stream()>>>((const bf16*)k.data_ptr(), (const bf16*)v.data_ptr(), kd, vd,
                                                    k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1),
                                                    v.stride(2), B, T, Hkv, hd, (int)pos, Tmax);
  SPA_LAUNCH_CHECK();
}

// rope_kv_write_ for the fp8 cache (graph decode prologue): the q heads are rotated in place exactly
// as there; a k head is rotated, rounded to bf16 (the value the bf16 cache would hold) and quantised, a
// v head is quantised, both into row *index + t. The hd / 8 threads of a head row are adjacent lanes
// in this index mapping, so the row's amax is a shuffle reduction among them (rotate_half: the upper
// half of the lanes holds no data and contributes 0).
template <int MODE>
__global__ __launch_bounds__(256) void rope_kv_write_q8_kernel(bf16* __restrict__ x, const float* __restrict__ cosT,
                                                               const float* __restrict__ sinT,
                                                               const int* __restrict__ pos,
                                                               const long* __restrict__ index, KV8Dst kd, KV8Dst vd,
                                                               long sb, long st, long sh, int B, int T, int H, int Hkv,
                                                               int hd, int Tmax, bool per_row) {
  const int vpr = hd / 8;
  const int NH = H + 2 * Hkv;
  const long total = (long)B * T * NH * vpr;
  const long row0 = *index;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int v = i % vpr;
    long r = i / vpr;
    const int hh = r % NH;
    r /= NH;
    const int t = r % T;
    const int b = r / T;
    SPA_DBG_CHECK(b, B);  // the per-row index read (debug build)
    const long row = (per_row ? index[b] : row0) + t;  // ragged batch: each sequence's own cache row
    if (hh >= H && (row >= Tmax || row < 0)) continue;  // whole lane groups: hh and row are uniform in a row
    bf16* src = x + b * sb + t * st + hh * sh;
    float a[8], bq[8];
    bool lo = true, hi = false;  // this lane holds elements [8v, 8v+8) / also their partners at +hd/2
    if (hh >= H + Hkv) {         // v: as is
      load8(src + v * 8, a);
    } else {
      const int ps = pos[b * T + t];
      const float* c = cosT + (long)ps * (hd / 2);
      const float* s = sinT + (long)ps * (hd / 2);
      if constexpr (MODE == 0) {
        load8(src + v * 8, a);
        const f32x4 cv = *reinterpret_cast<const f32x4*>(c + v * 4);
        const f32x4 sv = *reinterpret_cast<const f32x4*>(s + v * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float x0 = a[2 * k], x1 = a[2 * k + 1];
          a[2 * k] = fmaf(x0, cv[k], -(x1 * sv[k]));
          a[2 * k + 1] = fmaf(x0, sv[k], x1 * cv[k]);
        }
      } else {  // rotate_half: thread v < vpr/2 owns elements [8v, 8v+8) and their partners at +hd/2
        lo = hi = v < vpr / 2;
        if (lo) {
          float cv[8], sv[8];
          load8(src + v * 8, a);
          load8(src + hd / 2 + v * 8, bq);
          load8(c + v * 8, cv);
          load8(s + v * 8, sv);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float x0 = a[k], x1 = bq[k];
            a[k] = fmaf(x0, cv[k], -(x1 * sv[k]));
            bq[k] = fmaf(x0, sv[k], x1 * cv[k]);
          }
        }
      }
      if (hh < H) {  // q: in place
        if (lo) store8(src + v * 8, a);
        if (hi) store8(src + hd / 2 + v * 8, bq);
        continue;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {  // k: the bf16 the bf16 cache would hold
        a[k] = (float)(bf16)a[k];
        bq[k] = (float)(bf16)bq[k];
      }
    }
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (lo) amax = fmaxf(amax, fabsf(a[k]));
      if (hi) amax = fmaxf(amax, fabsf(bq[k]));
    }
    for (int o = 1; o < vpr; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const int e = e8m0_exp(amax);
    const float inv = e8m0_inv(e);
    const bool isv = hh >= H + Hkv;
    const int h = hh - H - (isv ? Hkv : 0);
    const KV8Dst& d = isv ? vd : kd;
    if (!SPA_DBG_OK(row, Tmax)) continue;
    uint8_t* dst = d.q + b * d.qb + row * d.qt + h * d.qh;
    if (lo) *reinterpret_cast<int2*>(dst + v * 8) = q8(a, inv);
    if (hi) *reinterpret_cast<int2*>(dst + hd / 2 + v * 8) = q8(bq, inv);
    if (v == 0 && SPA_DBG_OK(h * (long)Tmax + row, (long)Hkv * Tmax)) d.s[b * d.sb + h * d.sh + row] = (uint8_t)(e + 127);
  }
}

void rope_kv_write_q8_(const at::Tensor& x, const at::Tensor& cos, const at::Tensor& sin, const at::Tensor& pos,
                       const at::Tensor& index, const at::Tensor& kq, const at::Tensor& ks, const at::Tensor& vq,
                       const at::Tensor& vs, int64_t H, int64_t Hkv, int64_t mode, bool per_row) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 4 && x.stride(3) == 1,
              "rope_kv_write_q8: bf16 [B, T, heads, hd] qkv with contiguous hd");
  TORCH_CHECK(x.stride(0) % 8 == 0 && x.stride(1) % 8 == 0 && x.stride(2) % 8 == 0 && (uintptr_t)x.data_ptr() % 16 == 0,
              "rope_kv_write_q8: 16-byte aligned rows");
  const int B = x.size(0), T = x.size(1), hd = x.size(3);
  TORCH_CHECK(x.size(2) == H + 2 * Hkv && hd >= 16 && hd <= 512 && (hd & (hd - 1)) == 0,
              "rope_kv_write_q8: x must be packed [B, T, H + 2 Hkv, hd], hd a power of two in [16, 512]");
  const KV8Dst kd = kv8_dst(kq, ks, B, Hkv, hd, "rope_kv_write_q8"), vd = kv8_dst(vq, vs, B, Hkv, hd, "rope_kv_write_q8");
  TORCH_CHECK(vq.size(1) == kq.size(1), "rope_kv_write_q8: cache shape mismatch");
  TORCH_CHECK(cos.scalar_type() == at::kFloat && cos.is_contiguous() && sin.is_contiguous() && cos.size(1) == hd / 2,
              "rope_kv_write_q8: fp32 [Tmax, hd/2] tables");
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kInt && pos.is_contiguous() && pos.numel() == (int64_t)B * T,
              "rope_kv_write_q8: pos must be device int32 [B, T]");
  TORCH_CHECK(index.is_cuda() && index.scalar_type() == at::kLong && index.numel() >= 1,
              "rope_kv_write_q8: index must be a device int64 tensor");
  TORCH_CHECK(!per_row || (index.numel() == B && index.is_contiguous()),
              "rope_kv_write_q8: per_row needs one index per sequence (", B, "), got ", index.numel());
  TORCH_CHECK(mode == 0 || mode == 1, "rope_kv_write_q8: mode 0 (interleaved) or 1 (rotate_half)");
  DeviceGuard g(x.device());
  const long total = (long)B * T * (H + 2 * Hkv) * (hd / 8);
  if (total == 0) return;
  const int grid = (int)std::min<long>((total + 255) / 256, 4096);
  auto launch = [&](auto modec) {
    constexpr int M = decltype(modec)::value;
    rope_kv_write_q8_kernel<M><<<grid, 256, 0, stream()>>>(
        (bf16*)x.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(), pos.data_ptr<int>(),
        index.data_ptr<int64_t>(), kd, vd, x.stride(0), x.stride(1), x.stride(2), B, T, (int)H, (int)Hkv, hd,
        (int)kq.size(1), per_row);
  };
  if (mode == 0) launch(std::integral_constant<int, 0>{});
  else launch(std::integral_constant<int, 1>{});
  SPA_LAUNCH_CHECK();
}

}  // namespace spa

TORCH_LIBRARY_FRAGMENT(spa, m) {
  m.def("rope_(Tensor(a!) x, Tensor cos, Tensor sin, Tensor? pos, int nrot, int pos_off, int mode, "
        "bool inverse) -> ()");
  m.def("rope_kv_write_(Tensor(a!) x, Tensor cos, Tensor sin, Tensor pos, Tensor index, Tensor(b!) kc, "
        "Tensor(c!) vc, int n_heads, int n_kv_heads, int mode=0, bool per_row=False) -> ()");
  m.def("rope_kv_write_paged_(Tensor(a!) x, Tensor cos, Tensor sin, Tensor pos, Tensor index, Tensor(b!) kpool, "
        "Tensor(c!) vpool, Tensor block_table, int n_heads, int n_kv_heads, int mode=0, bool per_row=False) -> ()");
  m.def("kv_quant_write_(Tensor k, Tensor v, Tensor(a!) kq, Tensor(b!) ks, Tensor(c!) vq, Tensor(d!) vs, int pos) -> ()");
  m.def("rope_kv_write_q8_(Tensor(a!) x, Tensor cos, Tensor sin, Tensor pos, Tensor index, Tensor(b!) kq, "
        "Tensor(c!) ks, Tensor(d!) vq, Tensor(e!) vs, int n_heads, int n_kv_heads, int mode=0, "
        "bool per_row=False) -> ()");
}
TORCH_LIBRARY_IMPL(spa, CUDA, m) {
  m.impl("rope_", &spa::rope_);
  m.impl("rope_kv_write_", &spa::rope_kv_write_);
  m.impl("rope_kv_write_paged_", &spa::rope_kv_write_paged_);
  m.impl("kv_quant_write_", &spa::kv_quant_write_);
  m.impl("rope_kv_write_q8_", &spa::rope_kv_write_q8_);
}
