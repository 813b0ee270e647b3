"""Per-tile error bounds for the MFMA GEMM family against an fp64 oracle (pure torch, any device).

Operations: the grouped GEMMs of csrc/kernels/gemm4a.hip (ring, gemm4r, gemm4d), gemm8.hip (``grouped_gemm8``,
``wgrad8`` and its reduce), moe.hip ``grouped_gemm``, and the fp8 products of moe_fp8.hip / gemm8_fp8.hip. For all
of them there is ``ref64`` (the fp64 product, inputs taken at the values the kernel receives: for the fp8 ops the
e4m3 operands dequantised in fp64, ``deq_rows`` / ``deq_act_blk`` / ``deq_w_blk``), ``emulate`` (the same product
with only the roundings such a kernel must make: exact products, fp32 accumulation, one rounding to the output
dtype) and the measures below. A kernel's error per unit is bounded by a small multiple of the emulation's error
on the same inputs: a self-calibrating bound with no fixed constants, in the shape of tests/rowop_oracle.py.

Modes (the contract of ops.moe.grouped_gemm): 0: out[rows_e] = a[rows_e] @ w[e]^T; 1: out[rows_e] = a[rows_e] @ w[e];
2: out[e] = a[rows_e]^T @ w[rows_e] (the reduction runs over the expert's tokens). The dense weight gradient is
mode 2 with offsets [0, T]. ``c``: the old value of ``out`` that ``accumulate`` adds onto.

Units. The 16 x 16 output block, one MFMA tile, aligned to each expert's first row in modes 0 / 1 and to each
expert's [N, K] in mode 2. Blocks are walked row of blocks by row of blocks; a clipped block under 64 elements is
merged with the blocks that follow it (first along the row of blocks, then into the next row of blocks) until the
unit holds 64, and what is left at an expert's end joins the unit before it. No element is left out of a bound.
Each unit gets an RMS and a max-abs error (``unit_errors``).

Emulation orders. "seq": fp32 accumulation over blocks of 8 consecutive k (one lane group's k of an MFMA), each
block's 8 products summed exactly. "kernel": the order the source shows: ``depth``-deep MFMA slices ascending
from the expert's first k (32 for the 16x16x32 bf16 MFMA of gemm4a.hip / gemm8.hip, 16 for moe.hip's 32x32x16,
128 for the fp8 kernels: one scaled product per 128-k block), each slice summed exactly and added to the fp32
accumulator; for wgrad8 fp32 partials per token slice (``wgrad8_slices``, gemm8.hip:797-802), summed s = 0, 1, ..,
then the old ``out`` (wgrad_reduce_kernel, gemm8.hip:746-759).

Margins in force (kernel unit error <= margin x yardstick unit error on the same inputs):

    bf16 out:  RMS 1.5 x the worst bf16 RMS spread of SPREADS, max-abs 4.0   yardstick: ONE emulation, "kernel"
    fp32 out:  RMS 4.0, max-abs 4.0                          yardstick: per unit, the larger of the two orders

Observed spread between the two orders (tests/test_gemm_oracle_cpu.py measures it over every case and input kind
of tests/test_gemm_tiles_gpu.py, prints it and holds it to ``SPREADS``; worst per-unit ratio, either order as the
yardstick of the other):

    family   bf16 RMS   bf16 max-abs   fp32 RMS   fp32 max-abs
    gemm4a   1.0311     1.021          --         --        (600 products: modes 0 / 1 / 2, every shape and kind)
    gemm8    1.0430     1.013          --         --
    moe      1.0000     1.000          --         --
    wgrad8   1.0000     1.000          4.97       10.9
    fp8      1.0239     1.000          1.000      1.005     (fp32: both orders with mfma_f8_dot8)

    -> bf16 RMS margin 1.5 x 1.044 = 1.566 (the project's rule in attn_oracle.py: 1.5 x the worst spread), below the
       2.0 the CPU file asserts; bf16 truncation fails it on every unit. The spread is not the 1.0000 of three
       probed shapes: over thousands of units a few hold an element whose fp32 sum lies next to a bf16 rounding
       boundary and goes to the other neighbour in the other order, which moves a 64-element unit's RMS by a few
       percent.
    -> fp32: the orders differ by the count of roundings (one per 8 k against one per 32 k, and per token slice
       for wgrad8). The yardstick is per unit the larger of the two. On the fp8 products both orders carry the
       instruction's own summation (below), which is all of their error: without it the e4m3 sums are exact in
       fp32 on many units and the orders 53 x apart on the rest.

A unit whose yardstick error is exactly zero (an empty expert's dW, the "integer" input kind, accumulate onto
zeros of an exact product) must match exactly.

Kernel-specific steps (off unless asked for; never part of a margin):
    round_acc_first   gemm4a.hip g4_epilogue (:283 rounds acc to bf16 into the LDS image, :298 adds the old C in
                      fp32 and rounds again) and gemm8.hip's full-tile epilogue (:706, :723): bf16 accumulate is
                      bf16(float(bf16(acc)) + C). gemm8's 64-row tail tile (modes 0 / 1, ``g8_full_rows``) and
                      moe.hip (:405-413), moe_fp8.hip (:452-463) round acc + C once. gemm8_fp8.hip's bf16 epilogue
                      (:466, :482; wgrad8_fp8_blk) rounds acc first as gemm8.hip does. ``round_acc_first`` is True,
                      or a bool mask over the output rows.
Not modelled, because below the resolution of a bf16 output: moe_fp8.hip:494 applies the fp32 row scales
as (acc * sx) * sw after accumulating the raw e4m3 products; the emulation accumulates the dequantised products.

    mfma_f8_dot8      moe_fp8.hip:431 (v_mfma_scale_f32_32x32x64_f8f6f4) and gemm8_fp8.hip:236 (16x16x128): the
                      block-scaled e4m3 MFMA does not add exact products. tools/probe_fp8_mfma.py (hand-made e4m3
                      images with unit scales through both fp8 wgrad kernels, which give the same figures) shows:
                      in each group of 8 consecutive k every product is cut towards zero to a multiple of
                      2^(E - 13), E the largest sum of the two operands' exponents in the group (beside 256 x 256 a
                      product of 8 arrives, one of 4 is lost, 14 arrives as 8, 28 as 24; the same beside 448 x 448,
                      so E is the exponent sum, not the product's exponent); the groups then add up as exactly as
                      fp32 holds them. On randn operands that is about 2^-15 of a tile's largest value, 2e4 x the
                      error of exact products in fp32, and invisible in a bf16 output. ``emulate(dot8=13)`` cuts
                      the products so, in both orders ("kernel": 16 k per fp32 addition, "seq": 8); it is asked for
                      where the output is fp32 (fp8_wgrad_case). With it the kernels measure 1.000 x the yardstick.
"""
import functools
import math

import torch

MAX_MARGIN = 4.0
F32_RMS_MARGIN, F32_MAX_MARGIN = 4.0, 4.0
UNIT, MIN_UNIT = 16, 64
MFMA_F8_BITS = 13      # mfma_f8_dot8 (module docstring)

# worst spread between the two emulation orders per kernel family: (bf16 RMS, bf16 max-abs, fp32 RMS, fp32 max-abs),
# measured by tests/test_gemm_oracle_cpu.py test_spreads, which fails when a measurement exceeds its entry
SPREADS = {
    "gemm4a": (1.032, 1.03, 0.0, 0.0),
    "gemm8": (1.044, 1.02, 0.0, 0.0),
    "moe": (1.001, 1.001, 0.0, 0.0),
    "wgrad8": (1.001, 1.001, 5.0, 11.0),
    "fp8": (1.024, 1.001, 1.001, 1.006),
}
RMS_MARGIN = 1.5 * max(v[0] for v in SPREADS.values())   # the project's rule (attn_oracle.py): 1.5 x the worst spread


def margins(dtype):
    return (RMS_MARGIN, MAX_MARGIN) if dtype == torch.bfloat16 else (F32_RMS_MARGIN, F32_MAX_MARGIN)


def rel(a, b):
    """The whole-tensor measure of the older tests (tests/test_gemm4a_gpu.py, tests/test_moe_gpu.py)."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _cdiv(a, b):
    return (a + b - 1) // b


def offsets_of(counts):
    o = [0]
    for c in counts:
        o.append(o[-1] + int(c))
    return o


def _olist(offsets):
    return [int(v) for v in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]


# ------------------------------------------------------------------ dequantisation (fp64, exact)
def deq_rows(q, s):
    """e4m3 rows with one fp32 scale per row (quant_rows_fp8)."""
    return q.double() * s.double().reshape(-1, 1)


def deq_act_blk(q, s):
    """q [R, K] e4m3, s [R, >= K/128] E8M0: 1 x 128 tiles (quant_act_fp8_blk; the images of quant_t_fp8_seg)."""
    R, K = q.shape
    sc = torch.exp2(s[:, :K // 128].double() - 127)
    return (q.double().view(R, K // 128, 128) * sc[..., None]).view(R, K)


def deq_w_blk(wq, sw):
    """wq [E, N, K] e4m3 (N need not be a multiple of 128), sw [E, ceil(N/128), K/128] E8M0: 128 x 128 blocks."""
    E, N, K = wq.shape
    sc = torch.exp2(sw.double() - 127).repeat_interleave(128, 1)[:, :N]          # [E, N, K/128]
    return (wq.double().view(E, N, K // 128, 128) * sc[..., None]).view(E, N, K)


# ------------------------------------------------------------------ the product, per expert
def _problems(a, w, offsets, mode):
    """(e, lo, hi, A [m, k], B [k, n]) per expert: out_e = A @ B."""
    o = _olist(offsets)
    for e in range(len(o) - 1):
        lo, hi = o[e], o[e + 1]
        if mode == 2:
            yield e, lo, hi, a[lo:hi].t(), w[lo:hi]
        elif mode == 0:
            yield e, lo, hi, a[lo:hi], w[e].t()
        else:
            yield e, lo, hi, a[lo:hi], w[e]


def out_shape(a, w, offsets, mode):
    E = len(_olist(offsets)) - 1
    if mode == 2:
        return (E, a.shape[1], w.shape[1])
    return (a.shape[0], w.shape[1] if mode == 0 else w.shape[2])


def ref64(a, w, offsets, mode, c=None):
    """fp64 product of the operands as given (+ the old ``out`` value ``c``)."""
    out = torch.zeros(out_shape(a, w, offsets, mode), dtype=torch.float64, device=a.device)
    for e, lo, hi, A, B in _problems(a, w, offsets, mode):
        if hi > lo:
            r = A.double() @ B.double()
            if mode == 2:
                out[e] = r
            else:
                out[lo:hi] = r
    if c is not None:
        out = out + c.double().view_as(out)
    return out


def _dot8(A, B, k, ke, bits):
    """sum_k A[:, k] B[k] over [k, ke) as the block-scaled e4m3 MFMA forms it (module docstring, mfma_f8_dot8): in
    each group of 8 consecutive k every product is cut (towards zero) to a multiple of 2^(E - bits), E the largest
    sum of the two operands' exponents in the group; the cut products add exactly."""
    m, n = A.shape[0], B.shape[1]
    pad = (-(ke - k)) % 8
    a = torch.nn.functional.pad(A[:, k:ke], (0, pad)).view(m, -1, 8, 1)
    b = torch.nn.functional.pad(B[k:ke], (0, 0, 0, pad)).view(1, -1, 8, n)
    ea = torch.where(a != 0, torch.frexp(a)[1] - 1, torch.full_like(a, -4096, dtype=torch.int32))
    eb = torch.where(b != 0, torch.frexp(b)[1] - 1, torch.full_like(b, -4096, dtype=torch.int32))
    E = (ea + eb).amax(2, keepdim=True).clamp_min(-900)                       # [m, G, 1, n]
    grid = torch.ldexp(torch.ones((), dtype=A.dtype, device=A.device), E - bits)
    return (torch.trunc(a * b / grid) * grid).sum((1, 2))


def _accum(A, B, depth, k0=0, k1=None, dot8=None):
    """fp32 accumulator of A[:, k0:k1] @ B[k0:k1]: slices of ``depth`` k summed exactly (fp64), one fp32 rounding
    per slice. ``dot8``: the slices are formed by ``_dot8`` with that many bits."""
    A, B = A.double(), B.double()
    k1 = A.shape[1] if k1 is None else k1
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32, device=A.device)
    for k in range(k0, k1, depth):
        ke = min(k + depth, k1)
        part = A[:, k:ke] @ B[k:ke] if dot8 is None else _dot8(A, B, k, ke, dot8)
        acc = (acc.double() + part).float()
    return acc


def wgrad8_slices(T, N, K, splits=0):
    """Token-slice offsets of ops.wgrad8 (gemm8.hip:797-802, :818)."""
    tiles = _cdiv(N, 256) * _cdiv(K, 256)
    S = splits if splits > 0 else max(1, 256 // tiles)
    S = max(1, min(S, T // 512))
    chunk = _cdiv(_cdiv(T, S), 64) * 64
    S = _cdiv(T, chunk) if chunk else 0
    return [min(T, i * chunk) for i in range(S + 1)]


def _round(v, dtype, rounding):
    if rounding == "trunc":       # a deliberate fault for tests/test_gemm_oracle_cpu.py
        assert dtype == torch.bfloat16
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(dtype)
    return v.to(dtype)


def emulate(a, w, offsets, mode, order="kernel", out_dtype=torch.bfloat16, c=None, depth=32, slices=None,
            round_acc_first=False, rounding="nearest", dot8=None):
    """The product with fp32 accumulation in one of the two orders and one rounding to ``out_dtype``.
    ``slices``: wgrad8's token-slice offsets (mode 2, one expert). ``round_acc_first``, ``rounding``: module
    docstring."""
    d = depth if order == "kernel" else 8
    acc = torch.zeros(out_shape(a, w, offsets, mode), dtype=torch.float32, device=a.device)
    for e, lo, hi, A, B in _problems(a, w, offsets, mode):
        if hi <= lo:
            continue
        if slices is not None and order == "kernel":
            r = None
            for s in range(len(slices) - 1):
                p = _accum(A, B, d, slices[s], slices[s + 1], dot8)
                r = p if r is None else r + p
        else:
            r = _accum(A, B, d, dot8=dot8)
        if mode == 2:
            acc[e] = r
        else:
            acc[lo:hi] = r
    if c is None:
        return _round(acc, out_dtype, rounding)
    cf = c.float().view_as(acc)
    once = acc + cf
    if round_acc_first is False:
        return _round(once, out_dtype, rounding)
    twice = acc.to(out_dtype).float() + cf
    if round_acc_first is True:
        return _round(twice, out_dtype, rounding)
    m = round_acc_first.to(acc.device).view(-1, *([1] * (acc.dim() - 1)))
    return _round(torch.where(m, twice, once), out_dtype, rounding)


def g8_full_rows(counts, tail=64):
    """Mask over the rows of a mode 0 / 1 output: True where gemm8 runs the full 256-row tile, False on the 64-row
    tail tile (an expert's last rows past a multiple of 256 when at most ``tail`` of them, gemm8.hip:181-184)."""
    m = torch.ones(sum(counts), dtype=torch.bool)
    o = offsets_of(counts)
    for e, cnt in enumerate(counts):
        rem = cnt % 256
        if 0 < rem <= tail:
            m[o[e + 1] - rem:o[e + 1]] = False
    return m


# ------------------------------------------------------------------ units
@functools.lru_cache(maxsize=None)
def _unit_map(m, n):
    """ids [m, n] of the units of one expert's m x n output, and per unit its first (row block, column block)."""
    nrb, ncb = _cdiv(m, UNIT), _cdiv(n, UNIT)
    hr, wc = m - UNIT * (nrb - 1), n - UNIT * (ncb - 1)
    bid = torch.empty(nrb, ncb, dtype=torch.long)
    first = []
    if min(hr, UNIT) * wc >= MIN_UNIT and hr * UNIT >= MIN_UNIT:       # no clipped block under 64: one unit each
        bid.copy_(torch.arange(nrb * ncb).view(nrb, ncb))
        first = [(i // ncb, i % ncb) for i in range(nrb * ncb)]
    else:
        cur, held = -1, MIN_UNIT
        for rb in range(nrb):
            h = hr if rb == nrb - 1 else UNIT
            for cb in range(ncb):
                if held >= MIN_UNIT:
                    cur, held = cur + 1, 0
                    first.append((rb, cb))
                bid[rb, cb] = cur
                held += h * (wc if cb == ncb - 1 else UNIT)
        if held < MIN_UNIT and cur > 0:                                 # the remainder joins the unit before it
            bid[bid == cur] = cur - 1
            first.pop()
    ids = bid.repeat_interleave(UNIT, 0)[:m].repeat_interleave(UNIT, 1)[:, :n].contiguous()
    return ids, len(first), first


class Layout:
    """Unit ids of a whole output, with each unit's (expert, row block, column block)."""

    def __init__(self, offsets, mode, shape):
        o = _olist(offsets)
        E = len(o) - 1
        self.where = []
        if mode == 2:
            ids, n, first = _unit_map(shape[1], shape[2])
            self.ids = (ids[None] + n * torch.arange(E).view(E, 1, 1)).reshape(-1)
            for e in range(E):
                self.where += [(e, rb, cb) for rb, cb in first]
            self.n = n * E
        else:
            parts, base = [], 0
            for e in range(E):
                if o[e + 1] > o[e]:
                    ids, n, first = _unit_map(o[e + 1] - o[e], shape[1])
                    parts.append(ids + base)
                    base += n
                    self.where += [(e, rb, cb) for rb, cb in first]
            self.ids = torch.cat(parts).reshape(-1) if parts else torch.zeros(0, dtype=torch.long)
            self.n = base
        assert self.ids.numel() == math.prod(shape), "every element belongs to a unit"
        self._dev = {}

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.ids.to(device)
        return self._dev[key]


def unit_errors(x, ref, lay):
    """(RMS, max-abs) error per unit, fp64 [n] each."""
    ids = lay.on(x.device)
    d = (x.double() - ref).reshape(-1)
    z = torch.zeros(lay.n, dtype=torch.float64, device=x.device)
    cnt = torch.bincount(ids, minlength=lay.n).clamp_min(1)
    rms = torch.sqrt(z.index_add(0, ids, d * d) / cnt)
    mx = z.scatter_reduce(0, ids, d.abs(), "amax", include_self=True)
    return rms, mx


def unit_ratios(x, ref, yard, lay, yard2=None):
    """Per-unit kernel / yardstick ratios (RMS, max-abs) and the mask of units whose yardstick error is zero."""
    kr, km = unit_errors(x, ref, lay)
    yr, ym = unit_errors(yard, ref, lay)
    if yard2 is not None:
        yr2, ym2 = unit_errors(yard2, ref, lay)
        yr, ym = torch.maximum(yr, yr2), torch.maximum(ym, ym2)
    zero = ym == 0
    one = torch.ones_like(yr)
    return kr / torch.where(zero, one, yr), km / torch.where(zero, one, ym), zero, km


def assert_blocks(x, ref, yard, name, lay, yard2=None, rms_margin=None, max_margin=None):
    """Every unit of ``x`` within the margins of the yardstick's error on the same unit; a unit the yardstick gets
    exactly right must be exactly right. Returns the worst (RMS, max-abs) ratios."""
    assert x.shape == ref.shape == yard.shape, (name, x.shape, ref.shape, yard.shape)
    if lay.n == 0:
        return 0.0, 0.0
    rm, mm = margins(x.dtype)
    rm, mm = rms_margin or rm, max_margin or mm
    bad = ~torch.isfinite(x.double()).reshape(-1)
    if bad.any():
        i = int(bad.nonzero()[0])
        e, rb, cb = lay.where[int(lay.on(x.device)[i])]
        raise AssertionError(f"{name}: {int(bad.sum())} non-finite outputs, the first in the unit of expert {e}, "
                             f"row block {rb}, column block {cb} (flat index {i})")
    r_rms, r_max, zero, km = unit_ratios(x, ref, yard, lay, yard2)
    wrong = zero & (km > 0)
    if wrong.any():
        u = int(wrong.nonzero()[0])
        e, rb, cb = lay.where[u]
        raise AssertionError(f"{name}: {int(wrong.sum())} units must be exact (yardstick error 0) and are not; first: "
                             f"expert {e}, row block {rb}, column block {cb}, max-abs error {km[u].item():.4g}")
    r_rms, r_max = torch.where(zero, torch.zeros_like(r_rms), r_rms), torch.where(zero, torch.zeros_like(r_max), r_max)
    w_rms, w_max = r_rms.max().item(), r_max.max().item()
    if w_rms > rm or w_max > mm:
        u = int(torch.argmax(torch.maximum(r_rms / rm, r_max / mm)))
        e, rb, cb = lay.where[u]
        raise AssertionError(f"{name}: worst unit expert {e}, row block {rb}, column block {cb}: RMS error "
                             f"{r_rms[u].item():.3f} x yardstick (margin {rm:.3f}), max-abs {r_max[u].item():.3f} x "
                             f"(margin {mm:.1f}); {int(((r_rms > rm) | (r_max > mm)).sum())} of {lay.n} units over")
    return w_rms, w_max


def spread(e1, e2, ref, lay):
    """Worst per-unit (RMS, max-abs) ratio between two emulations, either as the yardstick of the other, and the
    count of units that one of them gets exactly right and the other does not."""
    a_r, a_m = unit_errors(e1, ref, lay)
    b_r, b_m = unit_errors(e2, ref, lay)

    def worst(p, q):
        ok = (p > 0) & (q > 0)
        if not ok.any():
            return 0.0
        return max((p[ok] / q[ok]).max().item(), (q[ok] / p[ok]).max().item())
    return worst(a_r, b_r), worst(a_m, b_m), int(((a_m > 0) != (b_m > 0)).sum())


# ------------------------------------------------------------------ inputs
KINDS = ("randn", "ramped", "integer")
INT_LIVE = 192        # live reduction indices of the integer kind; with |c| <= 64 every output is within 256


def _bf(t):
    return t.to(torch.bfloat16)


def _ints(shape, g):
    return torch.randint(-1, 2, shape, generator=g).float()


def _live(n, g):
    """Mask over n reduction indices with at most INT_LIVE set, always the first and last 32 among them."""
    m = torch.zeros(n, dtype=torch.bool)
    if n <= INT_LIVE:
        return ~m
    m[:32] = True
    m[-32:] = True
    mid = torch.randperm(n - 64, generator=g)[:INT_LIVE - 64] + 32
    m[mid] = True
    return m


def make_inputs(kind, counts, N, K, mode, seed, acc_dtype=None):
    """bf16 operands (a, w) of one grouped product on the CPU, and the old ``out`` value c (None unless
    ``acc_dtype``). Mode 0: a [M, K], w [E, N, K]; mode 1: a [M, K], w [E, K, N] (reduction K, output columns N);
    mode 2: a [T, N], w [T, K] (reduction: the expert's tokens).
    randn: the second operand scaled by red ** -0.5; ramped: the reduction index scaled by logspace(-2, 1);
    integer: entries in {-1, 0, 1}, at most INT_LIVE non-zeros along every reduction, c integer in [-64, 64]."""
    g = torch.Generator().manual_seed(seed)
    E, M = len(counts), sum(counts)
    o = offsets_of(counts)
    if mode == 2:
        ashape, wshape, oshape = (M, N), (M, K), (E, N, K)
    else:
        ashape, wshape, oshape = (M, K), ((E, N, K) if mode == 0 else (E, K, N)), (M, N)
    if kind == "integer":
        a, w = _ints(ashape, g), _ints(wshape, g)
        if mode == 2:
            for e in range(E):
                a[o[e]:o[e + 1]] *= _live(counts[e], g)[:, None]
        else:
            a *= _live(K, g)[None, :]
        c = torch.randint(-64, 65, oshape, generator=g).float()
    else:
        a, w = torch.randn(ashape, generator=g), torch.randn(wshape, generator=g)
        red = max(1, max(counts)) if mode == 2 else K
        w = w * red ** -0.5
        if kind == "ramped":
            if mode == 2:
                a = a * torch.logspace(-2, 1, max(M, 1))[:M, None]
            else:
                a = a * torch.logspace(-2, 1, K)[None, :]
        c = torch.randn(oshape, generator=g)
    c = None if acc_dtype is None else c.to(acc_dtype)
    return _bf(a), _bf(w), c


# ------------------------------------------------------------------ the cases of tests/test_gemm_tiles_gpu.py
RAGGED = [0, 1, 255, 257, 0, 513, 3, 64]
G4_COUNTS = {"ragged": RAGGED, "one": [256], "dense": [1300]}
G4_RED = {2: (64, 128, 192, 320), 1: (64, 128, 192, 320), 0: (32, 64, 96, 128, 160, 224)}
G4_N = (8, 264, 320)
# every N on the ragged counts; the single full tile and the dense rows at one ragged N each
G4_COUNTS_N = [("ragged", N) for N in G4_N] + [("one", 264), ("dense", 320)]
G4_DW_NK = ((8, 8), (264, 520), (256, 256))
_E256 = [[0, 8, 8, 1, 0, 8, 33, 8][i % 8] for i in range(256)]
G4_DW_LAYOUTS = {
    "e8_bal65": [65] * 8, "e8_bal32": [32] * 8, "e8_bal127": [127] * 8,
    "e8_skew": [1, 31, 32, 33, 63, 64, 127, 129], "e5": [129, 0, 65, 1, 33],
    "e16": [96] * 16, "e256": _E256,
}
MOE_COUNTS = [0, 1, 255, 257, 0, 130, 3, 64]
MOE_RED = (8, 40, 72, 136)
MOE_N = (8, 200)
G8_SKEW64 = (torch.rand(64, generator=torch.Generator().manual_seed(5)) ** 3 * 150).long().tolist()
G8_E300 = (torch.rand(300, generator=torch.Generator().manual_seed(5)) ** 3 * 40).long().tolist()
G8_CASES = {                       # test_grouped_gemm8_elementwise's cases, shrunk to about a second each
    "ragged": ([300, 0, 129, 1, 64, 700, 0, 33], 320, 192),
    "last": ([0] * 7 + [513], 256, 512),
    "deep": ([257, 255], 320, 1024),
    "skew64": (G8_SKEW64, 576, 256),
    "e300": (G8_E300, 128, 64),
    "dense": ([1300], 512, 320),
}
WG8_T = (512, 1027, 4104, 0)
WG8_NK = (264, 136)
WG8_SPLITS = (0, 1, 3, 100)
FP8_K = (128, 256, 1024)
FP8_N = (264, 384)
FP8_COUNTS = [300, 0, 129, 1, 64, 0, 33]


def _seed(*key):
    """A seed that does not depend on the interpreter's string hashing."""
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


FP8_KINDS = ("randn", "ramped", "blockramp", "integer")
_BLOCK_EXP = (0, -6, 4, -3)        # blockramp: neighbouring 128-blocks differ by 6 to 10 binary exponents


def _blockramp(n):
    return torch.exp2(torch.tensor([_BLOCK_EXP[(i // 128) % 4] for i in range(n)], dtype=torch.float32))


def _int32(v, device):
    return torch.tensor(v, dtype=torch.int32, device=device)


def fp8_fwd_list():
    """(op, kind, N, K): op "rows" grouped_gemm_fp8, "blk" grouped_gemm_fp8_blk, "g8blk" gemm8_fp8_blk."""
    return [(op, kind, N, K) for op in ("rows", "blk", "g8blk") for K in FP8_K for N in FP8_N for kind in FP8_KINDS]


def fp8_fwd_case(M, op, kind, N, K, device, orders=("kernel",)):
    """Quantised operands of one fp8 forward product (``M``: ops.moe, whose quantisers run on ``device``), the
    fp64 product of the dequantised operands and the emulation(s). ``exact``: the quantiser kept the operands."""
    counts = FP8_COUNTS
    E, Np, o = len(counts), _cdiv(N, 128) * 128, offsets_of(counts)
    x, W, _ = make_inputs("randn" if kind == "blockramp" else kind, counts, Np, K, 0, _seed("fp8", "rows" if op == "rows" else "blk", kind, N, K))
    if kind == "blockramp":
        x = _bf(x.float() * _blockramp(K)[None, :])
        W = _bf(W.float() * _blockramp(Np)[None, :, None].roll(128, 1))
    x, W = x.to(device), W.to(device)
    off = _int32(o, device)
    if op == "rows":
        Wn = W[:, :N].contiguous()
        xq, sx = M.quant_rows_fp8(x)
        wq, sw = M.quant_rows_fp8(Wn.view(E * N, K))
        wq = wq.view(E, N, K)
        xd, wd = deq_rows(xq, sx), deq_rows(wq.view(E * N, K), sw).view(E, N, K)
        exact = bool((xd == x.double()).all() and (wd == Wn.double()).all())
    else:
        xq, sx = M.quant_act_fp8_blk(x)
        wq, _, sw, _ = M.quant_weight_fp8_blk_uncached(W)
        wq = wq[:, :N].contiguous()
        xd, wd = deq_act_blk(xq, sx), deq_w_blk(wq, sw)
        exact = bool((xd == x.double()).all() and (wd == W[:, :N].double()).all())
    ref = ref64(xd, wd, o, 0)
    lay = layout_of(tuple(counts), 0, tuple(ref.shape))
    emus = [emulate(xd, wd, o, 0, order, torch.bfloat16, depth=128) for order in orders]
    return dict(args=(xq, sx, wq, sw, off), xd=xd, wd=wd, sw=sw, off=o, ref=ref, lay=lay, emus=emus, exact=exact)


FP8_WG_COUNTS = [100, 0, 256, 1000, 129, 1]        # 1, 0, 2, 8, 2, 1 K-tiles of 128 tokens
FP8_WG_K = 136


def fp8_wgrad_list():
    """(kind, N, out dtype, acc): dW [E, N, FP8_WG_K] of wgrad_fp8_blk and wgrad8_fp8_blk."""
    return [(kind, N, dt, acc) for N in FP8_N for kind in ("integer", "randn", "ramped")
            for dt, acc in ((torch.bfloat16, False), (torch.bfloat16, True), (torch.float32, False), (torch.float32, True))]


def fp8_wgrad_case(M, kind, N, out_dtype, acc, device, orders=("kernel", "seq"), round_acc_first=False):
    counts = FP8_WG_COUNTS
    E, T, o = len(counts), sum(counts), offsets_of(counts)
    Nq, Kq = _cdiv(N, 128) * 128, _cdiv(FP8_WG_K, 128) * 128
    dy, x, c = make_inputs(kind, counts, Nq, Kq, 2, _seed("fp8wg", kind, N, out_dtype, acc), out_dtype if acc else None)
    c = None if c is None else c[:, :N, :FP8_WG_K].contiguous().to(device)
    off = _int32(o, device)
    poff = M.padded_offsets(off)
    ld = M.wgrad_ld(T, E)
    aq, sa = M.quant_t_fp8_seg(dy.to(device), off, poff, ld)
    bq, sb = M.quant_t_fp8_seg(x.to(device), off, poff, ld)
    aq, sa, bq, sb = aq[:N].contiguous(), sa[:N].contiguous(), bq[:FP8_WG_K].contiguous(), sb[:FP8_WG_K].contiguous()
    po = _olist(poff)
    used = po[-1]
    ad, bd = deq_act_blk(aq[:, :used], sa).t(), deq_act_blk(bq[:, :used], sb).t()       # [tokens, N], [tokens, K]
    ref = ref64(ad, bd, po, 2, c)
    lay = layout_of(tuple(counts), 2, tuple(ref.shape))
    raf = round_acc_first and acc and out_dtype == torch.bfloat16
    # fp32 outputs resolve the MFMA's own summation (mfma_f8_dot8); a bf16 output does not
    dot8 = MFMA_F8_BITS if out_dtype == torch.float32 else None
    emus = [emulate(ad, bd, po, 2, order, out_dtype, c, depth=16 if dot8 else 128, round_acc_first=raf, dot8=dot8)
            for order in orders]
    exact = all(bool((ad[po[e]:po[e] + counts[e]] == dy[o[e]:o[e + 1], :N].to(device).double()).all()) for e in range(E))
    return dict(args=(aq, sa, bq, sb, poff), c=c, ref=ref, lay=lay, emus=emus, exact=exact)


@functools.lru_cache(maxsize=64)
def layout_of(counts, mode, shape):
    return Layout(offsets_of(counts), mode, shape)


def case(name, kind, counts, N, K, mode, acc, depth=32, round_acc_first=False, device="cpu", orders=("kernel",),
         out_dtype=torch.bfloat16, slices=None):
    """Inputs, fp64 reference, layout and emulation(s) of one grouped product of bf16 operands on ``device``.
    ``round_acc_first``: True, False, or "g8:<tail>" for gemm8's full-tile rows in modes 0 / 1."""
    a, w, c = make_inputs(kind, counts, N, K, mode, _seed(name, kind, acc, out_dtype), out_dtype if acc else None)
    a, w = a.to(device), w.to(device)
    c = None if c is None else c.to(device)
    o = offsets_of(counts)
    ref = ref64(a, w, o, mode, c)
    lay = layout_of(tuple(counts), mode, tuple(ref.shape))
    raf = round_acc_first if acc else False
    if isinstance(raf, str):
        raf = g8_full_rows(counts, int(raf[3:]))
    emus = [emulate(a, w, o, mode, order, out_dtype, c, depth, slices, raf) for order in orders]
    return dict(a=a, w=w, c=c, off=o, ref=ref, lay=lay, emus=emus)


def g4_list(impl):
    """Every gemm4a mode 0 / 1 product of the GPU file for one pipeline: (name, kind, counts, N, K, mode, acc)."""
    return [(f"{cn}-N{N}-K{K}", kind, G4_COUNTS[cn], N, K, mode, acc) for K in G4_RED[impl] for cn, N in G4_COUNTS_N
            for mode in (0, 1) for kind in KINDS for acc in (False, True)]


def g4_dw_list():
    return [(f"{ln}-N{N}-K{K}", kind, cnt, N, K, 2, acc) for ln, cnt in G4_DW_LAYOUTS.items() for N, K in G4_DW_NK
            if not (ln == "e256" and N * K > 256 * 256)          # 256 experts: one tile per expert, or one block
            for kind in KINDS for acc in (False, True)]


def g8_list(cname):
    counts, N, K = G8_CASES[cname]
    modes = (0, 1, 2) if N % 64 == 0 else (0, 2)
    return [(f"g8-{cname}", kind, counts, N, K, mode, acc) for mode in modes for kind in KINDS for acc in (False, True)]


def moe_list():
    return [(f"moe-N{N}-K{K}", kind, MOE_COUNTS, N, K, mode, acc) for K in MOE_RED for N in MOE_N for mode in (0, 1, 2)
            for kind in KINDS for acc in (False, True)]


def wg8_list(T):
    """(name, kind, T, splits, out dtype, acc, strided) of the wgrad8 products."""
    return [(f"wg8-T{T}", kind, T, sp, dt, acc, strided) for sp in WG8_SPLITS for dt in (torch.bfloat16, torch.float32)
            for acc in (False, True) for kind in KINDS for strided in ((False, True) if sp in (0, 3) else (False,))]
