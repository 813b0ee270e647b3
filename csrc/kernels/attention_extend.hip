// Extend attention: many query rows per sequence against a long KV cache whose valid length lives on
// the device, one length per sequence -- the multi-token step of a ragged or paged cache (a new chat
// turn behind a live slot, a chunk of a chunked prefill, a verify step). attn_decode takes at most 16
// rows per kv head and the flash forward needs a host length common to the batch; this kernel takes
// any Tq with the decode kernels' contract:
//   q bf16 [B, Tq, H, hd] (strided: the q heads of a packed qkv buffer), k / v the whole cache buffers
//   [B, Tk, Hkv, hd] or page pools [num_pages, page_size, Hkv, hd] behind a block table, kv_len int32
//   on the device (one entry, or B with per_row). Always causal: sequence b attends over its rows
//   [0, n_b), n_b = min(kv_len[b], Tk); query token t sits at row n_b - Tq + t and sees the keys at or
//   before it. A row that sees no key (n_b < Tq) writes zeros and lse = +inf.
//
// The loop is attn_fwd_kernel<HD, HD, 4, CAUSAL, false> of attention.hip (same products S^T = K Q^T and
// O^T = V^T P^T on v_mfma_f32_32x32x16_bf16, 32 query rows per wave, double-buffered K/V tiles with
// one barrier per tile, masks on diagonal / tail tiles only) and KEEPS its deferred rescale
// (kRescaleThr = 2^8: the tests' yardstick is emulate_bf16(defer_log2 = 8.0)). Two things differ:
//  * n_b is one scalar load per block; it gives the block's causal offset n_b - Tq and replaces Tk as
//    the valid-row bound everywhere. The grid is cdiv(Tq, 128) * B * H (x key splits), a function of
//    host shapes only, so a launch can be captured in a graph and replayed at any lengths.
//  * Tiles are loaded in 16-row pieces, one scalar buffer descriptor each. A wave's lanes cover at
//    most 16 aligned tile rows of a row pass, so the piece is wave-uniform; tiles start at multiples
//    of 32 and pages hold 16..256 rows, so a piece never straddles a page. PAGED: the piece's page is
//    one scalar table load (paged_kv.h), the loads of a tile's pieces issued together in front of
//    its K/V loads. The descriptor's range ends at the sequence's last valid row inside the piece,
//    so rows at or past n_b read zeros from the hardware range check, no table entry past
//    (n_b - 1) >> lg is read and no pool row the sequence does not own. PAGED is a flag on one
//    kernel body: the floating-point code is the same source, and the paged result is bitwise the
//    contiguous one on the gathered rows.
//  * Key split, as the forward's p.ksplit: a grid under 512 blocks is split along the keys (gridDim.y,
//    each split at least 256 cache rows, fp32 partials merged by attn_extend_merge_kernel). Measured
//    without it (profiles/extend_attention.txt): at B = 1 a 512-token chunk is 128 blocks and a
//    64-token turn 32 on 256 CUs, and the unsplit build takes 1.30x - 5.63x the time of this one
//    under 512 blocks. The split count depends on host shapes only.
// No K/V sharing across a GQA group's q-heads: not measured to win.
#include <algorithm>
#include "attn_common.h"
#include "attn_params.h"
#include "paged_kv.h"

SPA_DEBUG_TU("attention_extend.hip")

namespace spa {

struct ExtendParams {
  const bf16* q; const bf16* k; const bf16* v;
  bf16* out; float* lse;
  const int* kv_len;  // device cache length(s)
  bool per_row;       // kv_len holds B lengths; else one for all
  int B, H, Hkv, Tq, Tk;
  long sqb, sqt, sqh, skb, skt, skh, svb, svt, svh, sob, sot, soh;
  float scale_log2;
  PagedTable tb;      // PAGED only: k / v are the pools, skb / svb unused
  // key split (small grids): gridDim.y = ksplit blocks per (query block, b, h), each over a contiguous
  // share of the block's key tiles, writing fp32 partials -- unnormalised O rows at part
  // [ksplit, B, H, Tq, hd] and (m, l) pairs at mlpart [ksplit, B, H, Tq, 2] -- merged by
  // attn_extend_merge_kernel. ksplit is a function of host shapes only.
  int ksplit;
  float* part;
  float* mlpart;
};

// A/B switches (tools/build_variant.sh NAME -DSPA_EXTEND_KSPLIT=0 | -DSPA_EXTEND_LOOKAHEAD=1), rows of
// both variants in profiles/extend_attention.txt. KSPLIT 0 launches every grid unsplit (1.30x - 5.63x
// the time under 512 blocks). LOOKAHEAD 1 looks a tile's page ids up one tile load ahead of their use, as
// attn_decode_paged does: measured no faster at hd 128 with 512-token chunks and 1.11x - 1.25x the
// time at hd 256 and for 64-token steps, so the default looks them up in front of the tile's own loads.
#ifndef SPA_EXTEND_KSPLIT
#define SPA_EXTEND_KSPLIT 1
#endif
#ifndef SPA_EXTEND_LOOKAHEAD
#define SPA_EXTEND_LOOKAHEAD 0
#endif

constexpr int kExtWaves = 4;
template <int HD> constexpr int ext_bn() { return HD >= 256 ? 32 : 64; }

// PAGED: the page ids of the wave's pieces of the tile at row0, one scalar table load per row pass, all
// issued before the first is used (one scalar-load latency per tile, not one per row pass). A piece at
// or past n reads no table entry.
template <class L>
__device__ __forceinline__ void ext_pages(int (&pg)[L::NP], const ExtendParams& p, int b, int row0, int n, int piece) {
#pragma unroll
  for (int ps = 0; ps < L::NP; ++ps) {
    const int r0 = row0 + ps * L::R + piece;
    pg[ps] = r0 < n ? paged_page(p.tb, b, r0) : 0;
  }
}

// One K and one V tile (rows row0 .. row0 + BN of sequence b) into the loaders' registers, in 16-row
// pieces: `piece` is the wave's 16-aligned row offset inside a row pass, the loaders' voff is relative
// to it. n = valid rows of the sequence, pg (PAGED) = ext_pages of this tile.
template <bool PAGED, class L>
__device__ __forceinline__ void ext_load(L& lk, L& lv, const ExtendParams& p, const bf16* kbase, const bf16* vbase,
                                         int row0, int n, int piece, const int (&pg)[L::NP]) {
#pragma unroll
  for (int ps = 0; ps < L::NP; ++ps) {
    const int r0 = row0 + ps * L::R + piece;
    const int left = min(n - r0, 16);
    long prow = r0;
    if constexpr (PAGED) {
      prow = left > 0 ? paged_pool_row(p.tb, pg[ps], r0) : 0;
      SPA_DBG_CHECK(prow + (left > 0 ? left - 1 : 0), (long)p.tb.num_pages << p.tb.lg);
    }
    const int kbytes = left > 0 ? (int)(((long)(left - 1) * p.skt + L::IW) * 2) : 0;
    const int vbytes = left > 0 ? (int)(((long)(left - 1) * p.svt + L::IW) * 2) : 0;
    const __amdgpu_buffer_rsrc_t rk =
        __builtin_amdgcn_make_buffer_rsrc((void*)(kbase + prow * p.skt), 0, kbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv =
        __builtin_amdgcn_make_buffer_rsrc((void*)(vbase + prow * p.svt), 0, vbytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < L::NC; ++j) {
      lk.r[ps * L::NC + j] =
          __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rk, lk.voff + 256 * j, 0, 0));
      lv.r[ps * L::NC + j] =
          __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv, lv.voff + 256 * j, 0, 0));
    }
  }
}

template <int HD, bool PAGED>
__global__ __launch_bounds__(kExtWaves * 64, HD <= 128 ? 2 : 1) void attn_extend_kernel(ExtendParams p) {
  constexpr int NW = kExtWaves, BN = ext_bn<HD>(), NSUB = BN / 32, BM = 32 * NW, KS = HD / 16, DT = HD / 32;
  constexpr int NT = NW * 64, TK = BN * HD, TB = 2 * TK;
  static_assert(img_w<HD>() == HD, "square head dims only");
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * TB];  // [buf][K|V]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 31, hh = lane >> 5;
  const int nqb = cdiv(p.Tq, BM);
  // block -> (q-block, batch, q-head): q-block major over (b, h), heaviest q-blocks first
  const int nbh = p.H * p.B;
  const int bh = blockIdx.x % nbh;
  const int qb = nqb - 1 - blockIdx.x / nbh;
  const int h = bh % p.H, b = bh / p.H;
  const int hk = h / (p.H / p.Hkv);
  SPA_DBG_CHECK(qb, nqb);
  SPA_DBG_CHECK(hk, p.Hkv);
  (void)SPA_DBG_BRH(b, 0, 1, h, p.H);
  // valid cache rows of this block's sequence: one scalar load per block (b is block-uniform)
  const int n = min(p.kv_len[p.per_row ? b : 0], p.Tk);
  const int causal_off = n - p.Tq;  // key j visible to query token i iff j <= i + causal_off
  const int q0 = __builtin_amdgcn_readfirstlane(qb * BM + wave * 32);
  const int q = q0 + lq;
  const float c = p.scale_log2;

  bf16x8 qf[KS];
  {
    const bf16* qp = p.q + b * p.sqb + (long)q * p.sqt + h * p.sqh + 8 * hh;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = q < p.Tq ? *reinterpret_cast<const bf16x8*>(qp + 16 * s) : zero8();
  }
  f32x16 o[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) o[i] = splat16(0.f);
  float m = -1e30f, l = 0.f;

  const int kend = min(n, qb * BM + BM + causal_off);
  // a wave past the last query row skips all MFMA work but keeps staging tiles and meeting the barriers
  const int wave_kend = q0 >= p.Tq ? 0 : min(n, q0 + 32 + causal_off);
  const int ntiles_all = kend > 0 ? cdiv(kend, BN) : 0;
  // key split: this block's share [jbeg, jbeg + ntiles) of the key tiles (none: the empty partial)
  const int si = blockIdx.y;
  const int kper = cdiv(ntiles_all, p.ksplit);
  const int jbeg = min(ntiles_all, si * kper);
  const int ntiles = min(ntiles_all, jbeg + kper) - jbeg;
  const int kb0 = jbeg * BN;

  const bf16* kbase = p.k + (PAGED ? 0 : b * p.skb) + hk * p.skh;
  const bf16* vbase = p.v + (PAGED ? 0 : b * p.svb) + hk * p.svh;
  using Loader = TileLoader<HD, BN, NT>;
  Loader lk, lv;
  lk.init(p.skt, tid);
  lv.init(p.svt, tid);
  // 16-row pieces: the global offsets are relative to the wave's piece of a row pass
  const int rr = tid / Loader::W;
  const int piece = __builtin_amdgcn_readfirstlane(rr & ~15);
  lk.voff = (int)(((long)(rr & 15) * p.skt + lk.ch * 8) * 2);
  lv.voff = (int)(((long)(rr & 15) * p.svt + lv.ch * 8) * 2);
  [[maybe_unused]] int pg[Loader::NP] = {};
  // tile `row0` into the loaders' registers, PAGED: behind its page ids (SPA_EXTEND_LOOKAHEAD: the ids
  // were looked up one load earlier, and the next tile's are looked up behind this tile's loads)
  auto load = [&](const int row0) {
    if constexpr (PAGED && !SPA_EXTEND_LOOKAHEAD) ext_pages<Loader>(pg, p, b, row0, n, piece);
    ext_load<PAGED>(lk, lv, p, kbase, vbase, row0, n, piece, pg);
    if constexpr (PAGED && SPA_EXTEND_LOOKAHEAD) ext_pages<Loader>(pg, p, b, row0 + BN, n, piece);
  };
  if (ntiles > 0) {
    if constexpr (PAGED && SPA_EXTEND_LOOKAHEAD) ext_pages<Loader>(pg, p, b, kb0, n, piece);
    load(kb0);
    lk.store(smem);
    lv.store(smem + TK);
    if (ntiles > 1) load(kb0 + BN);
  }
  __syncthreads();
  LdsOff<HD> offk;
  offk.init(lane);
  // causal / tail mask of one 32-key sub-tile: only on diagonal / tail tiles
  auto mask = [&](f32x16& s, const int k0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      if (key >= n || key > q + causal_off) s[r] = -INFINITY;
    }
  };
  // scores -> probabilities for one 32-key sub-tile: each sub-tile is its own online-softmax step
  auto softmax = [&](f32x16& s) {
    float mx = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
    const float mxs = halfmax(mx) * c;
    // per-lane (exec-masked) deferred rescale: both lane halves of a row take the same decision
    if (mxs > m + kRescaleThr) {
      const float alpha = fexp2(m - mxs);
      l *= alpha;
#pragma unroll
      for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
      m = mxs;
    }
    const float nm = -m;
    float ls = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = fexp2(fmaf(s[r], c, nm));
      s[r] = e;
      ls += e;
    }
    l += ls;
  };
  // body(j, buffer) with the buffer a compile-time constant (loop unrolled x2) so every LDS address
  // is a precomputed lane offset + an immediate
  auto body = [&](const int j, auto bufc) {
    constexpr int BUF = decltype(bufc)::value;
    const int k0 = kb0 + j * BN;
    const bf16* Ks = smem + BUF * TB;
    const bf16* Vs = Ks + TK;
    if (j + 1 < ntiles) {
      bf16* Kn = smem + (1 - BUF) * TB;
      lk.store(Kn);
      lv.store(Kn + TK);
      if (j + 2 < ntiles) load(k0 + 2 * BN);
    }
#pragma unroll
    for (int t = 0; t < NSUB; ++t) {
      const int ks0 = k0 + 32 * t;
      if (ks0 < wave_kend) {
        bf16x8 kr[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kr[ks] = ld_row(Ks + 32 * t * HD, offk.row[ks]);
        f32x16 s = mfma32(kr[0], qf[0], splat16(0.f));
#pragma unroll
        for (int ks = 1; ks < KS; ++ks) s = mfma32(kr[ks], qf[ks], s);
        __builtin_amdgcn_sched_group_barrier(0x100, KS, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, KS, 0);
        const bool need_mask = (ks0 + 32 > n) || (ks0 + 31 > q0 + causal_off);
        if (need_mask) mask(s, ks0);
        softmax(s);
        const bf16x8 pa = pack_acc(s, 0), pb = pack_acc(s, 1);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          o[dt] = mfma32(ld_tr(Vs + 32 * t * HD, offk.tra[dt], offk.trb[dt]), pa, o[dt]);
          o[dt] = mfma32(ld_tr(Vs + (32 * t + 16) * HD, offk.tra[dt], offk.trb[dt]), pb, o[dt]);
        }
        chain_sched<2 * DT, 2, 3>();
      }
    }
    __syncthreads();
  };
  // make the q-fragment loads retire here, once, not at every tile's first MFMA (see attn_fwd_kernel)
#pragma unroll
  for (int s = 0; s < KS; ++s) asm volatile("" ::"v"(qf[s]));
  for (int j = 0; j < ntiles; j += 2) {
    body(j, IC<0>{});
    if (j + 1 < ntiles) body(j + 1, IC<1>{});
  }
  l = halfsum(l);
  if (p.ksplit > 1) {      // fp32 partial: unnormalised O and the (m, l) softmax state
    if (q < p.Tq && SPA_DBG_BRH(b, q, p.Tq, h, p.H) && SPA_DBG_OK(si, p.ksplit)) {
      const long row = (((long)si * p.B + b) * p.H + h) * p.Tq + q;
      float* dst = p.part + row * HD;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 w;
#pragma unroll
          for (int i = 0; i < 4; ++i) w[i] = o[dt][4 * g + i];
          *reinterpret_cast<f32x4*>(dst + 32 * dt + 8 * g + 4 * hh) = w;
        }
      if (hh == 0) {
        float2 ml;
        ml.x = m;
        ml.y = l;
        reinterpret_cast<float2*>(p.mlpart)[row] = ml;
      }
    }
    return;
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
  if (q < p.Tq && SPA_DBG_BRH(b, q, p.Tq, h, p.H)) {
    bf16* op = p.out + b * p.sob + (long)q * p.sot + h * p.soh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4 w;
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = (bf16)(o[dt][4 * g + i] * inv);
        *reinterpret_cast<bf16x4*>(op + 32 * dt + 8 * g + 4 * hh) = w;
      }
    if (hh == 0)
      p.lse[((long)b * p.H + h) * p.Tq + q] = (l > 0.f) ? (m + __log2f(l)) * 0.69314718055994531f : INFINITY;
  }
}

// Merge of the key splits: one wave per query row (b, h, q), a lane takes the columns lane, lane + 64, ...
// O = sum_s O_s 2^(m_s - M) / sum_s l_s 2^(m_s - M), M = max_s m_s; an empty split holds (m, l) = (-1e30, 0)
// and O_s = 0. A row no split saw a key for writes zeros and lse = +inf.
template <int HD>
__global__ __launch_bounds__(256) void attn_extend_merge_kernel(ExtendParams p) {
  const int lane = threadIdx.x & 63;
  const long nrows = (long)p.B * p.H * p.Tq;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const int q = (int)(row % p.Tq);
  const long bh = row / p.Tq;
  const int h = (int)(bh % p.H), b = (int)(bh / p.H);
  const float2* ml = reinterpret_cast<const float2*>(p.mlpart);
  float M = -1e30f;
  for (int s = 0; s < p.ksplit; ++s) M = fmaxf(M, ml[s * nrows + row].x);
  float L = 0.f, acc[HD / 64];
#pragma unroll
  for (int c = 0; c < HD / 64; ++c) acc[c] = 0.f;
  for (int s = 0; s < p.ksplit; ++s) {
    const float2 x = ml[s * nrows + row];
    const float w = fexp2(x.x - M);
    L += x.y * w;
    const float* src = p.part + (s * nrows + row) * HD + lane;
#pragma unroll
    for (int c = 0; c < HD / 64; ++c) acc[c] += src[64 * c] * w;
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  if (!SPA_DBG_BRH(b, q, p.Tq, h, p.H)) return;
  bf16* op = p.out + b * p.sob + (long)q * p.sot + h * p.soh + lane;
#pragma unroll
  for (int c = 0; c < HD / 64; ++c) op[64 * c] = (bf16)(acc[c] * inv);
  if (lane == 0) p.lse[row] = (L > 0.f) ? (M + __log2f(L)) * 0.69314718055994531f : INFINITY;
}

namespace {

// Key splits of a launch: grids under 512 blocks (two per CU) are split until they reach it, each
// split keeping at least 256 cache rows. A function of host shapes only (Tk is the buffers' row bound,
// not a length), so the launch stays graph-capturable.
int extend_splits(long blocks, int Tk) {
  if (!SPA_EXTEND_KSPLIT || blocks >= 512) return 1;
  const long want = (512 + blocks - 1) / blocks, cap = Tk / 256;
  return (int)std::max(1L, std::min({want, cap, 32L}));
}

void check_kv_len(const char* op, const at::Tensor& q, const at::Tensor& kv_len, bool per_row, int B) {
  TORCH_CHECK(kv_len.is_cuda() && kv_len.device() == q.device() && kv_len.scalar_type() == at::kInt &&
                  kv_len.numel() >= 1,
              op, ": kv_len must be a device int32 tensor");
  TORCH_CHECK(!per_row || (kv_len.numel() == B && kv_len.is_contiguous()), op,
              ": per_row needs one kv_len per sequence (", B, "), got ", kv_len.numel());
}

void check_rows(const char* op, const at::Tensor& t) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.dim() == 4, op, ": bf16 4-d tensors");
  TORCH_CHECK(t.stride(3) == 1 && t.stride(2) % 8 == 0 && t.stride(1) % 8 == 0 && t.stride(0) % 8 == 0 &&
                  ((uintptr_t)t.data_ptr() % 16) == 0,
              op, ": rows must be 16-byte aligned and contiguous in hd");
}

template <bool PAGED>
std::vector<at::Tensor> launch_extend(ExtendParams& p, const at::Tensor& q, int HD) {
  DeviceGuard g(q.device());
  auto out = at::empty({p.B, p.Tq, p.H, HD}, q.options());
  auto lse = at::empty({p.B, p.H, p.Tq}, q.options().dtype(at::kFloat));
  if ((long)p.B * p.Tq * p.H == 0) return {out, lse};
  p.q = (const bf16*)q.data_ptr();
  p.out = (bf16*)out.data_ptr();
  p.lse = lse.data_ptr<float>();
  p.sqb = q.stride(0); p.sqt = q.stride(1); p.sqh = q.stride(2);
  p.sob = out.stride(0); p.sot = out.stride(1); p.soh = out.stride(2);
  const long blocks = (long)cdiv(p.Tq, 32 * kExtWaves) * p.B * p.H;
  TORCH_CHECK(blocks < (1L << 31), "attn_extend: grid too large");
  auto st = stream();
  p.ksplit = extend_splits(blocks, p.Tk);
  at::Tensor part;
  const long nrows = (long)p.B * p.H * p.Tq;
  if (p.ksplit > 1) {
    part = at::empty({(long)p.ksplit * nrows * (HD + 2)}, q.options().dtype(at::kFloat));
    p.part = part.data_ptr<float>();
    p.mlpart = p.part + (long)p.ksplit * nrows * HD;   // 8-byte aligned: ksplit * nrows * HD is even
  }
  const dim3 grid((unsigned)blocks, (unsigned)p.ksplit);
  const unsigned mgrid = (unsigned)((nrows + 3) / 4);
#define SPA_EXTEND_LAUNCH(HDV)                                                          \
  {                                                                                     \
    attn_extend_kernel<HDV, PAGED><<<grid, kExtWaves * 64, 0, st>>>(p);                  \
    if (p.ksplit > 1) attn_extend_merge_kernel<HDV><<<mgrid, 256, 0, st>>>(p);           \
  }
  if (HD == 64) SPA_EXTEND_LAUNCH(64)
  else if (HD == 128) SPA_EXTEND_LAUNCH(128)
  else SPA_EXTEND_LAUNCH(256)
#undef SPA_EXTEND_LAUNCH
  SPA_LAUNCH_CHECK();
  return {out, lse};
}

}  // namespace

// q bf16 [B, Tq, H, hd]; k / v the whole cache buffers [B, Tk, Hkv, hd]; kv_len device int32, one
// entry or [B] with per_row. Returns [out bf16 [B, Tq, H, hd], lse fp32 [B, H, Tq]].
std::vector<at::Tensor> attn_extend(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                    const at::Tensor& kv_len, bool per_row) {
  for (auto* t : {&q, &k, &v}) check_rows("attn_extend", *t);
  const int B = q.size(0), Tq = q.size(1), H = q.size(2), HD = q.size(3);
  const int Tk = k.size(1), Hkv = k.size(2);
  TORCH_CHECK(HD == 64 || HD == 128 || HD == 256, "attn_extend: head dim must be 64, 128 or 256");
  TORCH_CHECK(k.size(0) == B && v.size(0) == B && v.size(1) == Tk && v.size(2) == Hkv && k.size(3) == HD &&
                  v.size(3) == HD && Hkv > 0 && H % Hkv == 0 && k.device() == q.device() && v.device() == q.device(),
              "attn_extend: shape mismatch");
  TORCH_CHECK(Tq <= Tk, "attn_extend: the cache must hold the query tokens");
  check_kv_len("attn_extend", q, kv_len, per_row, B);
  ExtendParams p{};
  p.k = (const bf16*)k.data_ptr(); p.v = (const bf16*)v.data_ptr();
  p.kv_len = kv_len.data_ptr<int>(); p.per_row = per_row;
  p.B = B; p.H = H; p.Hkv = Hkv; p.Tq = Tq; p.Tk = Tk;
  p.skb = k.stride(0); p.skt = k.stride(1); p.skh = k.stride(2);
  p.svb = v.stride(0); p.svt = v.stride(1); p.svh = v.stride(2);
  p.scale_log2 = (float)(scale * 1.4426950408889634);
  return launch_extend<false>(p, q, HD);
}

// attn_extend over a paged cache: kpool / vpool bf16 [num_pages, page_size, Hkv, hd], block_table int32
// [B, NP], Tk the logical row bound (<= NP * page_size). Rows at or past a sequence's valid length are
// never read, nor are their table entries.
std::vector<at::Tensor> attn_extend_paged(const at::Tensor& q, const at::Tensor& kpool, const at::Tensor& vpool,
                                          const at::Tensor& block_table, double scale, int64_t Tk64,
                                          const at::Tensor& kv_len, bool per_row) {
  for (auto* t : {&q, &kpool, &vpool}) check_rows("attn_extend_paged", *t);
  const int B = q.size(0), Tq = q.size(1), H = q.size(2), HD = q.size(3);
  const int64_t num_pages = kpool.size(0), page = kpool.size(1);
  const int Hkv = kpool.size(2);
  TORCH_CHECK(HD == 64 || HD == 128 || HD == 256, "attn_extend_paged: head dim must be 64, 128 or 256");
  TORCH_CHECK(page >= 16 && page <= 256 && (page & (page - 1)) == 0,
              "attn_extend_paged: page_size must be a power of two in [16, 256], got ", page);
  TORCH_CHECK(vpool.sizes() == kpool.sizes() && kpool.size(3) == HD && Hkv > 0 && H % Hkv == 0 && num_pages >= 1,
              "attn_extend_paged: shape mismatch");
  TORCH_CHECK(kpool.stride(0) == page * kpool.stride(1) && vpool.stride(0) == page * vpool.stride(1),
              "attn_extend_paged: a pool's pages must be back to back (stride(0) == page_size * stride(1))");
  TORCH_CHECK(num_pages * page < (1L << 31), "attn_extend_paged: pool rows must fit an int32");
  TORCH_CHECK(block_table.is_cuda() && block_table.device() == q.device() && kpool.device() == q.device() &&
                  vpool.device() == q.device() && block_table.scalar_type() == at::kInt && block_table.dim() == 2 &&
                  block_table.size(0) == B && block_table.is_contiguous(),
              "attn_extend_paged: block_table must be a contiguous int32 [B, NP] tensor on q's device");
  const int64_t NP = block_table.size(1);
  TORCH_CHECK(Tk64 >= 0 && Tk64 <= NP * page, "attn_extend_paged: Tk = ", Tk64, " outside the table's ", NP * page,
              " rows");
  const int Tk = (int)Tk64;
  TORCH_CHECK(Tq <= Tk, "attn_extend_paged: the cache must hold the query tokens");
  check_kv_len("attn_extend_paged", q, kv_len, per_row, B);
  ExtendParams p{};
  p.k = (const bf16*)kpool.data_ptr(); p.v = (const bf16*)vpool.data_ptr();
  p.kv_len = kv_len.data_ptr<int>(); p.per_row = per_row;
  p.B = B; p.H = H; p.Hkv = Hkv; p.Tq = Tq; p.Tk = Tk;
  p.skt = kpool.stride(1); p.skh = kpool.stride(2);  // skb / svb unused: rows come through the table
  p.svt = vpool.stride(1); p.svh = vpool.stride(2);
  p.scale_log2 = (float)(scale * 1.4426950408889634);
  int lg = 0;
  while ((1 << lg) < page) ++lg;
  p.tb = PagedTable{block_table.data_ptr<int>(), (int)NP, lg, (int)num_pages};
  return launch_extend<true>(p, q, HD);
}

}  // namespace spa

TORCH_LIBRARY_FRAGMENT(spa, m) {
  m.def("attn_extend(Tensor q, Tensor k, Tensor v, float scale, Tensor kv_len, bool per_row=False) -> Tensor[]");
  m.def("attn_extend_paged(Tensor q, Tensor kpool, Tensor vpool, Tensor block_table, float scale, int Tk, "
        "Tensor kv_len, bool per_row=False) -> Tensor[]");
}
TORCH_LIBRARY_IMPL(spa, CUDA, m) {
  m.impl("attn_extend", &spa::attn_extend);
  m.impl("attn_extend_paged", &spa::attn_extend_paged);
}
