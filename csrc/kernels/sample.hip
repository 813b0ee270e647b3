// Fused token sampler: one launch turns a row of logits into a token id (temperature, top-k,
// top-p, counter RNG), so a captured decode step can end in it (infer/graph.py).
//
// Contract (the fp64 oracle is ops/reference.py::sample_logits), per row, T = max(temperature, 1e-6):
//   order   raw logit descending, ties by ascending token index;
//   top-k   the first k tokens of that order (1 <= k < V, else off);
//   top-p   over softmax(logit / T) renormalised on the top-k set: a token stays iff the mass
//           strictly before it in the order is <= top_p (top_p >= 1: off);
//   draw    P = the kept tokens' softmax in VOCABULARY order, C its inclusive prefix sum,
//           Z = C[V-1]: the result is the smallest i with C[i] >= u * Z, u in (0, 1] either
//           supplied per row or u01(seed, offset * B + b) (spa_rng.h).
// -inf has weight 0; rows with NaN or nothing finite are unspecified (the id stays in [0, V)).
// u has 24 bits, so a token under 2^-24 of the kept mass may never be drawn.
//
// The kept set is always "every key above a threshold key, plus the first n ties AT the
// threshold in index order", so nothing is sorted: the threshold is found by radix passes over
// the order-preserving integer key of the logit (12 + 10 + 10 bits; count histograms for top-k,
// exp-weighted mass histograms for top-p, both in LDS), the number of admitted ties follows
// from the histogram of the last digit, and one prefix pass in vocabulary order draws. The
// third digit is skipped when every key under the selected 22-bit prefix shares its low bits
// (always, for bf16 or bf16-rounded logits).
//
// One 1024-thread workgroup per row, one launch, no workspace, no global atomics: every pass
// re-reads the row (0.25-0.5 MB at V = 128K: L2 resident after the first), wave w owning the
// contiguous tiles [w * tpw, (w + 1) * tpw) with 8 tiles (8 x 16 B per lane) in flight.
// Passes: plain 2 (max, draw), top-k 3, top-p 4, both 4 (top_k <= 1024: the top-k set is gathered
// in LDS and top-p settled there; 5 beyond) (+1 per filter for fp32 logits with live low bits),
// plus the draw's rescan of one wave's segment. fp32 sums (the top-p histogram: fixed
// point). Measured at V = 128256 fp32, one HIP-graph replay with the offset increment: 60 us
// plain, 86 us top-k 50, 137 us top-p 0.9, 109 us both at B = 1, +10 us at B = 16
// (profiles/fused_sampling.txt): a pass is one CU's read of the row, 20-25 us each when the
// kernel runs alone (about half of that inside the LLaMA3-8B decode graph). Splitting a row
// over several workgroups (partials in a workspace, merged by the last to arrive or by a second
// launch) is the next step if the sampler ever shows in a decode profile.
#include "spa_common.h"
#include "spa_rng.h"

namespace spa {
namespace {

constexpr int kNT = 1024, kNW = kNT / 64, kVec = 4, kTile = 64 * kVec, kUnroll = 6;
constexpr int kBits1 = 12, kBits2 = 10, kBits3 = 10;
constexpr int kBins = 1 << kBits1;
constexpr int kListCap = kNT;   // largest top_k whose set is gathered in LDS for top-p (one candidate per thread)

// float -> uint32 with the same order (-0 folded into +0, so equal logits have equal keys).
// 0 is no finite or infinite float's key: it marks "no element".
__device__ __forceinline__ uint32_t to_key(float f) {
  uint32_t b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// A weight (<= 1: the row maximum's is 1) in fixed point. Integer LDS atomics add the mass histogram:
// the sums do not depend on arrival order (the same call gives the same id, bit for bit), and a
// ds_add_f32 histogram measured twice the whole call's time (top-p 0.9, B = 1, V = 128256: 266 us
// against 134 us; a count-only pass costs ~12 us). The sum of 2^23 weights of 1 still fits 64 bits.
constexpr float kFixed = 1099511627776.f;   // 2^40
__device__ __forceinline__ unsigned long long to_fixed(float w) { return (unsigned long long)(w * kFixed + 0.5f); }
__device__ __forceinline__ float from_key(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <typename T>
struct Row {
  const T* __restrict__ p;   // first element of the row
  int V;
  int mis;      // elements between the previous kVec-element boundary and p (vector loads stay aligned)
  int tiles;    // kTile-element tiles covering [-mis, V)
  int tpw;      // tiles per wave
};

template <typename T> struct VecOf;
template <> struct VecOf<float> { typedef f32x4 type; };
template <> struct VecOf<bf16> { typedef bf16x4 type; };

// kUnroll consecutive tiles from tile t (tiles >= t1: none): lane l of tile t holds elements
// [(t * 64 + l) * kVec - mis, +kVec) of the row; what falls outside [0, V) is unspecified (callers
// test the index). Every whole group is one aligned vector load and all of them are issued before
// the first is used (one round trip per batch: the passes are latency-bound at 4 waves per SIMD);
// the row's first and last group, when partial, are re-read element by element afterwards.
template <typename T>
__device__ __forceinline__ void load_batch(const T* __restrict__ p, int V, int mis, int t, int t1, int lane,
                                           typename VecOf<T>::type (&raw)[kUnroll]) {
  typedef typename VecOf<T>::type vec_t;
  // logits live in global memory: say so (through the Row the compiler emitted flat loads)
  typedef const __attribute__((address_space(1))) vec_t* gvec_p;
  typedef const __attribute__((address_space(1))) T* gelem_p;
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int i0 = ((t + u) * 64 + lane) * kVec - mis;
    raw[u] = vec_t{};
    if (t + u < t1 && i0 >= 0 && i0 + kVec <= V) raw[u] = *(gvec_p)(p + i0);
  }
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int i0 = ((t + u) * 64 + lane) * kVec - mis;
    if (t + u < t1 && !(i0 >= 0 && i0 + kVec <= V) && i0 + kVec > 0 && i0 < V) {   // partial: an end of the row
#pragma unroll
      for (int j = 0; j < kVec; ++j) {
        const int i = i0 + j;
        if (i >= 0 && i < V) raw[u][j] = *(gelem_p)(p + i);
      }
    }
  }
}

// f(key, index) for every element of the row; a wave walks its own contiguous tiles in order
template <typename T, typename F>
__device__ __forceinline__ void for_each(const Row<T>& r, F&& f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t0 = wave * r.tpw, t1 = min(t0 + r.tpw, r.tiles);
  for (int t = t0; t < t1; t += kUnroll) {
    typename VecOf<T>::type raw[kUnroll];
    load_batch<T>(r.p, r.V, r.mis, t, t1, lane, raw);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
      for (int j = 0; j < kVec; ++j) {
        const int i = (t + u) * kTile + lane * kVec + j - r.mis;
        if (t + u < t1 && (unsigned)i < (unsigned)r.V) f(to_key((float)raw[u][j]), i);
      }
    }
  }
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_incl_i(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ float wave_incl_f(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

struct Shared {
  int hc[kBins];        // digit counts
  unsigned long long hm[kBins];   // digit masses (top-p passes), fixed point: weight * 2^40
  int sc[kNW];
  float sm[kNW];
  unsigned kmax, kand, kor;
  int digit, cbefore, cin;
  float mbefore;
  int ctot;
  float mtot;
  float wabove[kNW];
  int wties[kNW];
  int nlist;                  // top-k + top-p with a small k: keys above the top-k threshold, listed
  unsigned long long zfx;     // and their fixed-point mass
};

// Histogram of digit (key >> shift) & (2^nbits - 1) over the keys whose higher bits equal `prefix`
// and that lie above `floor_key` (the top-k threshold during the top-p passes: its admitted ties
// are added by the caller). Also: the largest matching key, and AND / OR of the matching keys
// >= floor_key (do they share their bits below `shift`?).
template <typename T, bool MASS>
__device__ __forceinline__ void hist_pass(const Row<T>& r, Shared& s, int shift, int nbits, uint32_t prefix, uint32_t floor_key,
                          float mval, float invT) {
  const int tid = threadIdx.x, nbins = 1 << nbits, hs = shift + nbits;
  __syncthreads();
  for (int i = tid; i < nbins; i += kNT) {
    s.hc[i] = 0;
    if (MASS) s.hm[i] = 0ull;
  }
  if (tid == 0) { s.kmax = 0u; s.kand = ~0u; s.kor = 0u; }
  __syncthreads();
  uint32_t mx = 0u, la = ~0u, lo = 0u;
  for_each(r, [&](uint32_t k, int) {
    if (hs < 32 && (k >> hs) != prefix) return;
    mx = max(mx, k);
    if (k < floor_key) return;
    la &= k; lo |= k;
    if (k == floor_key) return;
    const int d = (int)((k >> shift) & (uint32_t)(nbins - 1));
    atomicAdd(&s.hc[d], 1);
    if (MASS) atomicAdd(&s.hm[d], to_fixed(__expf((from_key(k) - mval) * invT)));
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    la &= (uint32_t)__shfl_xor((int)la, o, 64);
    lo |= (uint32_t)__shfl_xor((int)lo, o, 64);
  }
  if ((tid & 63) == 0) {
    atomicMax(&s.kmax, mx);
    atomicAnd(&s.kand, la);
    atomicOr(&s.kor, lo);
  }
  __syncthreads();
}

// Walk the histogram from the highest digit down. Count mode: the digit that holds the
// `need`-th key (1-based). Mass mode: the lowest non-empty digit whose mass-before is <= limit
// (the highest non-empty digit always qualifies: its mass-before is 0). Results in s.digit,
// s.cbefore / s.mbefore (count / mass in the digits above), s.cin, s.ctot, s.mtot.
template <bool MASS>
__device__ __forceinline__ void select_digit(Shared& s, int nbits, int need, float limit) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nbins = 1 << nbits;
  const int per = nbins / kNT;   // 4 (12 bits) or 1 (10 bits)
  int c[4];
  float m[4];
  int tc = 0;
  float tm = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = 0; m[j] = 0.f;
    if (j < per) {
      const int bin = nbins - 1 - (tid * per + j);
      c[j] = s.hc[bin];
      if (MASS) m[j] = (float)s.hm[bin] * (1.f / kFixed);
    }
    tc += c[j]; tm += m[j];
  }
  const int ic = wave_incl_i(tc, lane);
  const float im = wave_incl_f(tm, lane);
  if (lane == 63) { s.sc[wave] = ic; s.sm[wave] = im; }
  if (tid == 0) s.digit = -1;
  __syncthreads();
  int bc = 0, totc = 0;
  float bm = 0.f, totm = 0.f;
#pragma unroll
  for (int w = 0; w < kNW; ++w) {
    if (w < wave) { bc += s.sc[w]; bm += s.sm[w]; }
    totc += s.sc[w]; totm += s.sm[w];
  }
  const float pm = __shfl_up(im, 1, 64);
  bc += ic - tc;
  bm += lane ? pm : 0.f;
  if (tid == 0) { s.ctot = totc; s.mtot = totm; }
  int mine = -1, mybc = 0, mycin = 0;
  float mybm = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < per && c[j] > 0) {
      const bool hit = MASS ? (bm <= limit) : (bc < need && need <= bc + c[j]);
      if (hit) { mine = tid * per + j; mybc = bc; mybm = bm; mycin = c[j]; }
    }
    bc += c[j]; bm += m[j];
  }
  if (mine >= 0) atomicMax(&s.digit, mine);   // descending position: the largest is the lowest digit
  __syncthreads();
  if (mine >= 0 && mine == s.digit) { s.cbefore = mybc; s.mbefore = mybm; s.cin = mycin; }
  __syncthreads();
  if (tid == 0) {
    if (s.digit < 0) { s.digit = nbins - 1; s.cbefore = 0; s.mbefore = 0.f; s.cin = 0; }  // NaN rows
    s.digit = nbins - 1 - s.digit;
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kNT) void sample_kernel(const T* __restrict__ logits, int V, float invT, int top_k,
                                                     float top_p, const float* __restrict__ u,
                                                     const int64_t* __restrict__ seed,
                                                     const int64_t* __restrict__ offset, int64_t* __restrict__ out) {
  __shared__ Shared s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, B = gridDim.x;
  Row<T> r;
  r.p = logits + (long)b * V;
  r.V = V;
  r.mis = (int)(((uintptr_t)r.p / sizeof(T)) % kVec);
  r.tiles = (V + r.mis + kTile - 1) / kTile;
  r.tpw = (r.tiles + kNW - 1) / kNW;
  const int shifts[3] = {kBits2 + kBits3, kBits3, 0}, widths[3] = {kBits1, kBits2, kBits3};
  const bool use_k = top_k >= 1 && top_k < V, use_p = top_p < 1.f;

  // ---- top-k: threshold key and the number of its ties that are admitted; the row maximum
  uint32_t thr = 0u;   // kept: key > thr, plus the first nt keys == thr in index order
  int nt = 0;
  uint32_t kmax;
  if (use_k) {
    int need = top_k;
    uint32_t prefix = 0u;
    for (int d = 0; d < 3; ++d) {
      hist_pass<T, false>(r, s, shifts[d], widths[d], prefix, 0u, 0.f, 0.f);
      if (d == 0) kmax = s.kmax;
      const uint32_t low = (1u << shifts[d]) - 1u, kand = s.kand, shared_low = ((s.kand ^ s.kor) & low) == 0u;
      select_digit<false>(s, widths[d], need, 0.f);
      need -= s.cbefore;
      prefix = (prefix << widths[d]) | (uint32_t)s.digit;
      if (d > 0 && shared_low) { prefix = (prefix << shifts[d]) | (kand & low); break; }
    }
    thr = prefix;
    nt = max(need, 1);
  } else {
    __syncthreads();
    if (tid == 0) s.kmax = 0u;
    __syncthreads();
    uint32_t mx = 0u;
    for_each(r, [&](uint32_t k, int) { mx = max(mx, k); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    if (lane == 0) atomicMax(&s.kmax, mx);
    __syncthreads();
    kmax = s.kmax;
  }
  const float mval = from_key(kmax);
  auto weight = [&](uint32_t k) { return __expf((from_key(k) - mval) * invT); };

  // ---- top-p over the top-k set: the last key whose mass-before is <= top_p * Z_k
  if (use_p && use_k && top_k <= kListCap) {
    // A small top-k set is gathered instead (one pass, no mass histogram): every key above thr_k
    // goes to an LDS list with its fixed-point weight (the nt_k admitted ties of thr_k are known),
    // and each thread tries one candidate threshold: its mass-before is the integer sum of the
    // heavier entries, so neither the list's arrival order nor the summation order shows.
    uint32_t* list = reinterpret_cast<uint32_t*>(s.hc);
    unsigned long long* wl = s.hm;
    const uint32_t thr_k = thr;
    const int nt_k = nt;
    __syncthreads();
    if (tid == 0) { s.nlist = 0; s.zfx = 0ull; s.kand = ~0u; s.cin = 0; }
    __syncthreads();
    for_each(r, [&](uint32_t k, int) {
      if (k > thr_k) {
        const int pos = atomicAdd(&s.nlist, 1);   // fewer than top_k keys lie above thr_k
        if (pos < kListCap) { list[pos] = k; wl[pos] = to_fixed(weight(k)); }
      }
    });
    __syncthreads();
    const int n = min(s.nlist, kListCap);
    if (tid < n) atomicAdd(&s.zfx, wl[tid]);
    __syncthreads();
    const unsigned long long zfx = s.zfx + (unsigned long long)nt_k * to_fixed(weight(thr_k));
    const float pz = top_p * ((float)zfx * (1.f / kFixed));
    float before = 0.f;
    uint32_t x = 0u;
    if (tid <= n) {   // candidates: every listed key, and thr_k itself
      x = tid < n ? list[tid] : thr_k;
      unsigned long long bf = 0ull;
      for (int j = 0; j < n; ++j) bf += list[j] > x ? wl[j] : 0ull;
      before = (float)bf * (1.f / kFixed);
      if (before <= pz) atomicMin(&s.kand, x);   // the heaviest key always qualifies (0 <= pz)
    }
    __syncthreads();
    thr = s.kand;
    if (tid <= n && x == thr) {
      s.mbefore = before;   // equal keys computed the same integer sum
      if (tid < n) atomicAdd(&s.cin, 1);
    }
    __syncthreads();
    const int cin = thr == thr_k ? nt_k : s.cin;
    const float w = weight(thr);
    const float q = w > 0.f ? (pz - s.mbefore) / w : (float)cin;
    nt = q >= (float)cin ? cin : max((int)q + 1, 1);
    nt = max(nt, 1);
  } else if (use_p) {
    const uint32_t thr_k = thr;
    const int nt_k = nt;
    const float w_k = nt_k > 0 ? weight(thr_k) : 0.f;
    float acc = 0.f, pz = 0.f;
    int cin = 0;
    uint32_t prefix = 0u;
    for (int d = 0; d < 3; ++d) {
      const int hs = shifts[d] + widths[d];
      hist_pass<T, true>(r, s, shifts[d], widths[d], prefix, thr_k, mval, invT);
      if (tid == 0 && nt_k > 0 && (hs >= 32 || (thr_k >> hs) == prefix)) {   // the admitted top-k ties
        const int dg = (int)((thr_k >> shifts[d]) & ((1u << widths[d]) - 1u));
        s.hc[dg] += nt_k;
        s.hm[dg] += (unsigned long long)nt_k * to_fixed(w_k);
      }
      __syncthreads();
      const uint32_t low = (1u << shifts[d]) - 1u, kand = s.kand, shared_low = ((s.kand ^ s.kor) & low) == 0u;
      select_digit<true>(s, widths[d], 0, d == 0 ? 0.f : pz - acc);
      if (d == 0) {
        // the first walk only totals the kept mass (its limit 0 selects the top digit); walk again
        pz = top_p * s.mtot;
        select_digit<true>(s, widths[d], 0, pz);
      }
      acc += s.mbefore;
      cin = s.cin;
      prefix = (prefix << widths[d]) | (uint32_t)s.digit;
      if (d > 0 && shared_low) { prefix = (prefix << shifts[d]) | (kand & low); break; }
    }
    thr = prefix;
    const float w = weight(thr);
    const float q = w > 0.f ? (pz - acc) / w : (float)cin;
    nt = q >= (float)cin ? cin : max((int)q + 1, 1);
    nt = max(nt, 1);
  }

  // ---- draw: per-wave kept mass in vocabulary order, then the owning wave rescans its segment
  {
    float ab = 0.f;
    int ti = 0;
    for_each(r, [&](uint32_t k, int) {
      if (k > thr) ab += weight(k);
      else if (k == thr) ++ti;
    });
    ab = wave_sum(ab);
    ti = wave_sum_i(ti);
    __syncthreads();
    if (lane == 0) { s.wabove[wave] = ab; s.wties[wave] = ti; }
    __syncthreads();
  }
  const float wthr = nt > 0 ? weight(thr) : 0.f;
  float km[kNW];
  float Z = 0.f;
  {
    int tb = 0;
#pragma unroll
    for (int w = 0; w < kNW; ++w) {
      const int adm = min(max(nt - tb, 0), s.wties[w]);
      km[w] = s.wabove[w] + (float)adm * wthr;
      Z += km[w];
      tb += s.wties[w];
    }
  }
  const float uu = u ? u[b] : u01((uint64_t)seed[0], (uint64_t)offset[0] * (uint64_t)B + (uint64_t)b);
  const float target = uu * Z;
  int selw = -1, lastw = -1, sel_tb = 0;
  float sel_cum = 0.f;
  {
    float cum = 0.f;
    int tb = 0;
#pragma unroll
    for (int w = 0; w < kNW; ++w) {
      if (km[w] > 0.f) lastw = w;
      if (selw < 0 && km[w] > 0.f && cum + km[w] >= target) { selw = w; sel_cum = cum; sel_tb = tb; }
      cum += km[w];
      tb += s.wties[w];
    }
    if (selw < 0 && lastw >= 0) {   // rounding left the last sum a hair under u * Z
      selw = lastw; sel_cum = 0.f; sel_tb = 0;
      for (int w = 0; w < lastw; ++w) { sel_cum += km[w]; sel_tb += s.wties[w]; }
    }
  }
  if (selw < 0) {   // nothing with weight: unspecified row, keep the id in range
    if (tid == 0) out[b] = 0;
    return;
  }
  if (wave != selw) return;
  // Per batch the tiles' totals come first (kUnroll independent butterflies, their shuffle latencies
  // overlapped) and whole tiles before the target are stepped over; the two dependent wave scans
  // run only on the tile that holds it (scanning every tile cost 5-10 us more per call).
  // Totals and scans add in different orders: should stepping over lose the target by a rounding,
  // the second attempt scans every tile.
  int result = -1, lastkept = -1;
  const int t0 = wave * r.tpw, t1 = min(t0 + r.tpw, r.tiles);
  for (int attempt = 0; attempt < 2 && result < 0; ++attempt) {
  float run = sel_cum;
  int trun = sel_tb;
  for (int t = t0; t < t1 && result < 0; t += kUnroll) {
    typename VecOf<T>::type raw[kUnroll];
    load_batch<T>(r.p, r.V, r.mis, t, t1, lane, raw);
    float tsum[kUnroll];
    int tcnt[kUnroll];
#pragma unroll
    for (int x = 0; x < kUnroll; ++x) {
      tsum[x] = 0.f; tcnt[x] = 0;
#pragma unroll
      for (int j = 0; j < kVec; ++j) {
        const int i = (t + x) * kTile + lane * kVec + j - r.mis;
        const uint32_t kk = (t + x < t1 && (unsigned)i < (unsigned)V) ? to_key((float)raw[x][j]) : 0u;
        if (kk > thr) tsum[x] += weight(kk);
        else if (kk != 0u && kk == thr) ++tcnt[x];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int x = 0; x < kUnroll; ++x) {
        tsum[x] += __shfl_xor(tsum[x], o, 64);
        tcnt[x] += __shfl_xor(tcnt[x], o, 64);
      }
    }
#pragma unroll
    for (int x = 0; x < kUnroll; ++x) {
      if (t + x >= t1 || result >= 0) continue;   // wave-uniform
      if (attempt == 0) {
        const float mass = tsum[x] + (float)min(max(nt - trun, 0), tcnt[x]) * wthr;
        if (run + mass < target) { run += mass; trun += tcnt[x]; continue; }
      }
      const int i0 = (t + x) * kTile + lane * kVec - r.mis;
      uint32_t kx[kVec];   // 0: outside the row
      int tc = 0;
#pragma unroll
      for (int j = 0; j < kVec; ++j) {
        kx[j] = (unsigned)(i0 + j) < (unsigned)V ? to_key((float)raw[x][j]) : 0u;
        tc += (kx[j] != 0u && kx[j] == thr) ? 1 : 0;
      }
      const int tinc = wave_incl_i(tc, lane);
      int rank = trun + tinc - tc;   // ties before this lane's first element
      float p[kVec], sum = 0.f;
#pragma unroll
      for (int j = 0; j < kVec; ++j) {
        const uint32_t kk = kx[j];
        p[j] = 0.f;
        if (kk != 0u) {
          if (kk > thr) p[j] = weight(kk);
          else if (kk == thr) { p[j] = rank < nt ? wthr : 0.f; ++rank; }
        }
        sum += p[j];
        if (p[j] > 0.f) lastkept = i0 + j;
      }
      const float inc = wave_incl_f(sum, lane);
      const unsigned long long hit = __ballot(sum > 0.f && run + inc >= target);
      if (hit) {
        const int src = __ffsll((long long)hit) - 1;
        int pick = -1, lastp = -1;
        float c = run + inc - sum;
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
          c += p[j];
          if (p[j] > 0.f) {
            lastp = i0 + j;
            if (pick < 0 && c >= target) pick = i0 + j;
          }
        }
        if (pick < 0) pick = lastp;   // the lane's own sum order fell a hair short: its last kept token
        result = __shfl(pick, src, 64);
      } else {
        run += __shfl(inc, 63, 64);
        trun += __shfl(tinc, 63, 64);
      }
    }
  }
  }
  if (result < 0) {   // the rescan's sums fell a hair short of the target: the segment's last kept token
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lastkept = max(lastkept, __shfl_xor(lastkept, o, 64));
    result = lastkept;
  }
  if (lane == 0) out[b] = (int64_t)min(max(result, 0), V - 1);
}

}  // namespace

at::Tensor sample_logits(const at::Tensor& logits, double temperature, int64_t top_k, double top_p,
                         const c10::optional<at::Tensor>& u, const c10::optional<at::Tensor>& seed,
                         const c10::optional<at::Tensor>& offset, const c10::optional<at::Tensor>& out) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "sample_logits: logits must be a [B, V] HIP tensor");
  TORCH_CHECK(logits.scalar_type() == at::kFloat || logits.scalar_type() == at::kBFloat16,
              "sample_logits: logits must be fp32 or bf16");
  TORCH_CHECK(logits.is_contiguous(), "sample_logits: logits must be contiguous");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(B >= 1 && V >= 1 && V < (1LL << 30) && B < (1LL << 31), "sample_logits: need B >= 1 and 1 <= V < 2^30");
  TORCH_CHECK(top_p > 0.0, "sample_logits: top_p must be > 0");
  TORCH_CHECK(u.has_value() != (seed.has_value() && offset.has_value()) && seed.has_value() == offset.has_value(),
              "sample_logits: pass exactly one of u or (seed and offset)");
  const float* up = nullptr;
  const int64_t *sp = nullptr, *op = nullptr;
  if (u) {
    TORCH_CHECK(u->is_cuda() && u->get_device() == logits.get_device() && u->scalar_type() == at::kFloat &&
                    u->is_contiguous() && u->numel() == B,
                "sample_logits: u must be a contiguous fp32 [B] tensor on the logits' device");
    up = u->data_ptr<float>();
  } else {
    for (const auto* t : {&*seed, &*offset})
      TORCH_CHECK(t->is_cuda() && t->get_device() == logits.get_device() && t->scalar_type() == at::kLong &&
                      t->numel() == 1,
                  "sample_logits: seed and offset must be int64 [1] tensors on the logits' device");
    sp = seed->data_ptr<int64_t>();
    op = offset->data_ptr<int64_t>();
  }
  at::Tensor o;
  if (out) {
    TORCH_CHECK(out->is_cuda() && out->get_device() == logits.get_device() && out->scalar_type() == at::kLong &&
                    out->is_contiguous() && out->numel() == B,
                "sample_logits: out must be a contiguous int64 tensor of B elements on the logits' device");
    o = *out;
  } else {
    o = at::empty({B, 1}, logits.options().dtype(at::kLong));
  }
  DeviceGuard g(logits.device());
  const float invT = 1.f / std::max((float)temperature, 1e-6f);
  const int k = (int)std::min<int64_t>(std::max<int64_t>(top_k, 0), V);   // 0 or V: off
  const float tp = (float)std::min(top_p, 1.0);
  if (logits.scalar_type() == at::kFloat)
    sample_kernel<float><<<(int)B, kNT, 0, stream()>>>(logits.data_ptr<float>(), (int)V, invT, k, tp, up, sp, op,
                                                      o.data_ptr<int64_t>());
  else
    sample_kernel<bf16><<<(int)B, kNT, 0, stream()>>>((const bf16*)logits.data_ptr(), (int)V, invT, k, tp, up, sp, op,
                                                     o.data_ptr<int64_t>());
  SPA_LAUNCH_CHECK();
  return o;
}

}  // namespace spa

TORCH_LIBRARY_FRAGMENT(spa, m) {
  m.def("sample_logits(Tensor logits, float temperature, int top_k, float top_p, Tensor? u=None, Tensor? seed=None, "
        "Tensor? offset=None, Tensor(a!)? out=None) -> Tensor");
}
TORCH_LIBRARY_IMPL(spa, CUDA, m) { m.impl("sample_logits", &spa::sample_logits); }
