"""Weight-only decode for 5..16 rows on the GPU: skinny_gemm_w8 / skinny_gemm_w4 (csrc/kernels/skinny_gemm.hip) on the
fp8 and MXFP4 decode images. Exact where the arithmetic is exact (placement, integer sums), per 16 x 16 unit against
the fp64 oracle of tests/gemm_oracle.py elsewhere, row independence and sentinels bitwise, the refusals, the opt-in
routing from ``linear`` (``quantize_decode_weights(max_rows=)``) and quantised models decoding a batch of 8 through a
ragged, paged GraphDecoder against the full forward of a copy that holds the dequantised weights.

The images are built directly or by the torch formula (ops/reference.py quant_mxfp4), never by the HIP quantizers."""
import pytest
import torch

import gemm_oracle as G
from solvingpapers_amd.infer import GraphDecoder, clear_decode_weights, quantize_decode_weights
from solvingpapers_amd.ops import _ext, reference as R
from test_gemv_w4_gpu import Holder, block_exponents, block_weights, random_image

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
FMTS = ("fp8", "mxfp4")

# Copies of the constants of csrc/kernels/skinny_gemm.hip: change both together, or the shapes below stop reaching the
# paths they name. STEP: k per load step of 16 weight rows (4 * CH: 64 e4m3, 128 MXFP4); U: skinny_u<F>(), steps in
# flight of the unrolled loop; WAVES = SKINNY_WAVES (K slices of a block), MIN_BLOCKS = SKINNY_MIN_BLOCKS,
# MIN_KB = SKINNY_MIN_KB; plan() is skinny_plan.
STEP = {"fp8": 64, "mxfp4": 128}
U = {"fp8": 4, "mxfp4": 2}
WAVES, MIN_BLOCKS, MIN_KB = 4, 512, 2


def plan(N, K):
    """(n-tiles per wave, K splits over blocks, the 128-k blocks of each of the 4 S wave slices)"""
    NT = 2 if N < 8192 else 4
    nb = K // 128
    S = max(1, min(-(-MIN_BLOCKS // (N // (16 * NT))), nb // (WAVES * MIN_KB)))
    sl = [(i + 1) * nb // (WAVES * S) - i * nb // (WAVES * S) for i in range(WAVES * S)]
    return NT, S, sl


# The loop-boundary K: 27 scale blocks over S = 3 block splits x 4 waves gives wave slices of 2 and of 3 blocks.
# 2 blocks = 256 k is exactly one pass of the unrolled loop (U * STEP = 256 in both formats); 3 blocks add the
# remainder loop (2 steps e4m3, 1 step MXFP4); the slices end on wave and on block split boundaries.
KL = 27 * 128


def test_loop_boundary_k_reaches_every_path():
    for N in (256, 384):
        NT, S, sl = plan(N, KL)
        assert NT == 2 and S == 3 and set(sl) == {2, 3} and sum(sl) == KL // 128
    for f in FMTS:
        assert U[f] * STEP[f] == 2 * 128 and 3 * 128 % STEP[f] == 0
    assert KL < 10922                                        # the exact-sum bound of both formats


def op(fmt):
    return _ext.ops().skinny_gemm_w8 if fmt == "fp8" else _ext.ops().skinny_gemm_w4


def dequant(fmt, wq, s):
    return (R.dequant_w8 if fmt == "fp8" else R.dequant_w4)(wq, s)


def fp8_image(N, K, seed, lo=-6, hi=6, integer=False):
    """an e4m3 image built directly: values randn * 64 (or integers in [-8, 8]), one exponent in [lo, hi] per
    128 x 128 block"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-8, 9, (N, K), generator=g).float() if integer else (torch.randn(N, K, generator=g) * 64).clamp(-448, 448)
    s = (127 + torch.randint(lo, hi + 1, (N // 128, K // 128), generator=g)).to(torch.uint8)
    assert len(torch.unique(s)) > 1 or s.numel() == 1
    return v.to(torch.float8_e4m3fn).to(DEV), s.to(DEV)


def rand_image(fmt, N, K, seed):
    """per-block magnitudes spread over 2^-6 .. 2^6"""
    if fmt == "fp8":
        return fp8_image(N, K, seed)
    return R.quant_mxfp4(block_weights((N, K), seed))


def rows_x(M, K, base):
    """[M, K] fp64 with at most 5 + log2(base / 31) significant bits: rows 0 / 1 (mod 2) hold 1 + k % base and
    1 + k // base, which together name k; later pairs are those times -1 and powers of two."""
    k = torch.arange(K, dtype=torch.float64)
    f = (1 + k % base, 1 + k // base)
    return torch.stack([f[m % 2] * (-1.0) ** (m // 2) * 2.0 ** ((m // 2) % 5 - 2) for m in range(M)])


# ------------------------------------------------------------------ 1. placement
@pytest.mark.parametrize("fmt", FMTS)
def test_placement_exact(fmt):
    """Row r's only non-zero weight sits at k = r, so y[m, r] = x[m, r] * w[r, r]; the scale exponents differ between
    horizontal and vertical neighbour blocks, so a scale, nibble, byte or lane from the wrong place gives another
    number. x has at most 5 (fp8) / 6 (MXFP4) significant bits, the weights 3 / 2: every product is exact in bf16."""
    if fmt == "fp8":
        N = K = 256
        r = torch.arange(N)
        v = torch.zeros(N, K)
        v[r, r] = (1.0 + r % 7) * (1 - 2 * ((r // 7) % 2))
        s = torch.tensor([[127, 130], [132, 125]], dtype=torch.uint8)
        wq, s, base = v.to(torch.float8_e4m3fn).to(DEV), s.to(DEV), 31
    else:
        N = K = 128
        r = torch.arange(N)
        code = (1 + r % 7) | ((r // 7) % 2) << 3
        q = torch.zeros(N, K // 2, dtype=torch.int64)
        q[r, r // 2] = code << (4 * (r % 2))
        s = (127 + block_exponents(N, K // 32)).to(torch.uint8)
        assert not torch.equal(s[:, 0], s[:, 1]) and not torch.equal(s[0], s[1])
        wq, s, base = q.to(torch.uint8).to(DEV), s.to(DEV), 63
    w = dequant(fmt, wq, s).double()
    assert (w != 0).sum() == N and (w.diagonal() != 0).all()
    x = rows_x(16, K, base).to(DEV)
    assert torch.equal(x.to(BF).double(), x)
    for M in (5, 16):
        y = op(fmt)(x[:M].to(BF), wq, s)
        ref = x[:M, :N] * w.diagonal()[None, :]
        assert torch.equal(ref.to(BF).double(), ref)
        assert torch.equal(y.double(), ref), (fmt, M)


# ------------------------------------------------------------------ 2. exact sums
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_sums(fmt):
    """Integer x with |x| <= 8; fp8 weights integers in [-8, 8] (exact e4m3), MXFP4 any codes, block exponents in
    [-2, 2]: every product and partial sum is a multiple of 2^-2 (2^-3) below 2^24 of those units at K = KL
    (3456 * 8 * 8 * 4 * 4 < 2^24; 3456 * 8 * 6 * 4 * 8 < 2^24), so fp32 accumulation is exact in any order and over
    any split, and y is bf16(fp64 sum)."""
    N, K = 256, KL
    wq, s = fp8_image(N, K, 20, -2, 2, integer=True) if fmt == "fp8" else random_image((N, K), 20, -2, 2)
    w = dequant(fmt, wq, s).double()
    x = torch.randint(-8, 9, (16, K), generator=torch.Generator().manual_seed(21)).to(DEV)
    for M in (5, 9, 16):
        y = op(fmt)(x[:M].to(BF), wq, s)
        ref = (x[:M].double() @ w.t()).to(BF)
        assert torch.equal(y, ref), (fmt, M)


# ------------------------------------------------------------------ 3. random inputs, per 16 x 16 unit
SHAPES = [
    (5, 128, 128),            # one block, one scale block: a single live wave
    (9, 384, KL),             # unrolled loop, remainder loop, wave and block split boundaries
    (16, 256, KL),
    (13, 4096, 4096),         # LLaMA3-8B o-proj
    (16, 1024, 14336),        # down-proj's depth
]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_random_against_fp64_oracle_per_unit(fmt, M, N, K):
    """Kernel error per 16 x 16 unit within the bf16 margins in force of tests/gemm_oracle.py of an emulation's error
    on the same inputs (exact products, fp32 accumulation, one rounding): "kernel" order, 32-deep MFMA slices; the
    kernel splits K over waves and blocks, so per unit the larger of that and the "seq" order is the yardstick."""
    wq, s = rand_image(fmt, N, K, 30)
    x = torch.randn(M, K, device=DEV, dtype=BF, generator=torch.Generator(DEV).manual_seed(31))
    w = dequant(fmt, wq, s)[None]
    y = op(fmt)(x, wq, s)
    assert y.shape == (M, N) and y.dtype == BF
    off = [0, M]
    ref = G.ref64(x, w, off, 0)
    lay = G.layout_of((M,), 0, (M, N))
    yard = G.emulate(x, w, off, 0, order="kernel", depth=32)
    split = len([n for n in plan(N, K)[2] if n]) > 1
    yard2 = G.emulate(x, w, off, 0, order="seq", depth=32) if split else None
    rm, mm = G.margins(BF)
    w_rms, w_max = G.assert_blocks(y, ref, yard, f"skinny {fmt} {M}x{N}x{K}", lay, yard2, rm, mm)
    print(f"skinny_gemm {fmt} M={M} N={N} K={K}: worst unit RMS {w_rms:.3f} x, max-abs {w_max:.3f} x the yardstick "
          f"(margins {rm:.3f}, {mm:.1f}); rel {G.rel(y, ref):.3e}")


# ------------------------------------------------------------------ 4. row independence
@pytest.mark.parametrize("fmt", FMTS)
def test_rows_are_independent(fmt):
    N, K = 384, KL
    wq, s = rand_image(fmt, N, K, 40)
    x = torch.randn(16, K, device=DEV, dtype=BF, generator=torch.Generator(DEV).manual_seed(41))
    y = op(fmt)(x, wq, s)
    assert torch.isfinite(y).all()
    for m in (5, 11):
        assert torch.equal(op(fmt)(x[:m], wq, s), y[:m]), (fmt, m)
        xn = x.clone()
        xn[m:] = float("nan")
        yn = op(fmt)(xn, wq, s)
        assert torch.equal(yn[:m], y[:m]) and torch.isnan(yn[m:]).all(), (fmt, m)
    wide = torch.randn(16, K + 64, device=DEV, dtype=BF)
    wide[:, 8:K + 8] = x
    xs = wide[:, 8:K + 8]
    assert not xs.is_contiguous() and xs.data_ptr() % 16 == 0
    assert torch.equal(op(fmt)(xs, wq, s), y)


# ------------------------------------------------------------------ 5. sentinel
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M", [5, 9, 16])
def test_rows_past_m_are_never_read(fmt, M):
    """x is the first M rows of a buffer whose other rows are NaN (one of them directly behind row M - 1): the result
    is finite and bitwise that of a buffer of its own. The op returns a fresh [M, N] tensor, so there is no
    caller-visible output around it."""
    N, K = 256, KL
    wq, s = rand_image(fmt, N, K, 50)
    buf = torch.full((20, K), float("nan"), device=DEV, dtype=BF)
    buf[:M] = torch.randn(M, K, device=DEV, dtype=BF, generator=torch.Generator(DEV).manual_seed(51))
    y = op(fmt)(buf[:M], wq, s)
    assert y.shape == (M, N) and torch.isfinite(y).all()
    assert torch.equal(y, op(fmt)(buf[:M].clone(), wq, s))
    assert torch.isnan(buf[M:]).all()


# ------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("fmt", FMTS)
def test_rejects_bad_calls(fmt):
    f, N, K = op(fmt), 256, 384
    wq, s = rand_image(fmt, N, K, 60)
    o8, o4 = fp8_image(N, K, 61), R.quant_mxfp4(block_weights((N, K), 61))
    other = o4 if fmt == "fp8" else o8
    x = torch.randn(8, K, device=DEV, dtype=BF, generator=torch.Generator(DEV).manual_seed(62))
    good = f(x, wq, s)
    assert G.rel(good, R.gemv_w8(x, wq, s) if fmt == "fp8" else R.gemv_w4(x, wq, s)) < 1e-2
    kb = K // 128 if fmt == "fp8" else K // 32
    bad = [
        (x[:0], wq, s),                                         # M == 0
        (torch.cat([x, x, x])[:17], wq, s),                     # M > 16
        (x.float(), wq, s),                                     # x not bf16
        (x, wq.to(BF), s),                                      # bf16 weights are not an image
        (x, wq, s.to(torch.int8)),                              # scales not uint8
        (x, *other),                                            # an image of the other format
        (x, other[0], s),
        (x, wq, s[:, :kb - 1].contiguous()),                    # s of the wrong shape
        (x, wq, s.t().contiguous()),                            # s transposed
        (x, wq, s.t().contiguous().t()),
        (x[:, :256].contiguous(), wq, s),                       # x and wq disagree on K
        (torch.randn(8, K + 4, device=DEV, dtype=BF)[:, :K], wq, s),        # rows not 16-byte aligned
        (torch.randn(8, K + 8, device=DEV, dtype=BF)[:, 4:K + 4], wq, s),   # base not 16-byte aligned
        (x.cpu(), wq, s),
    ]
    if fmt == "fp8":
        bad.append((x[:, :320].contiguous(), wq[:, :320].contiguous(), s))  # K % 128 != 0
    for i, args in enumerate(bad):
        with pytest.raises((RuntimeError, NotImplementedError)):
            f(*args)
        assert torch.equal(f(x, wq, s), good), i                # a following good call is unharmed


# ------------------------------------------------------------------ 7. routing
@pytest.mark.parametrize("fmt", FMTS)
def test_linear_routes_5_to_max_rows_to_skinny_gemm(fmt):
    from solvingpapers_amd.ops.linear import linear
    h = Holder((256, 384), 7)
    w = h.w
    attr = "_spa_w8" if fmt == "fp8" else "_spa_w4"
    gemv = _ext.ops().gemv_w8 if fmt == "fp8" else _ext.ops().gemv_w4
    g = torch.Generator(DEV).manual_seed(70)
    x2, x8, x17 = (torch.randn(m, 1, 384, device=DEV, dtype=BF, generator=g) for m in (2, 8, 17))
    with torch.no_grad():
        y8_master, y17_master = linear(x8, w), linear(x17, w)
        rep = quantize_decode_weights(h, fmt=fmt)                   # the default: 8 rows read the masters
        assert rep["max_rows"] == 4 and w._spa_wrows == 4
        assert torch.equal(linear(x8, w), y8_master)
        y2 = linear(x2, w)
        rep = quantize_decode_weights(h, fmt=fmt, max_rows=16)
        assert rep["max_rows"] == 16 and rep["quantized"] == ["w"] and w._spa_wrows == 16
        wq, s = getattr(w, attr)[:2]
        y8 = linear(x8, w)
        assert y8.shape == (8, 1, 256)
        assert torch.equal(y8.view(8, 256), op(fmt)(x8.view(8, 384), wq, s))
        assert not torch.equal(y8, y8_master)
        assert torch.equal(linear(x2, w).view(2, 256), gemv(x2.view(2, 384), wq, s)) and torch.equal(linear(x2, w), y2)
        assert torch.equal(linear(x17, w), y17_master)              # 17 rows: the masters
        assert torch.equal(linear(x8, w, torch.zeros(256, device=DEV, dtype=BF)), linear(x8, w.detach().clone(),
                                                                                         torch.zeros(256, device=DEV, dtype=BF)))
    w.requires_grad_(True)                                          # autograd on the weight: the masters
    assert torch.equal(linear(x8, w).detach(), y8_master)
    w.requires_grad_(False)
    with torch.no_grad():
        w.mul_(2)
        with pytest.raises(RuntimeError, match=r"'w'.*quantize_decode_weights"):
            linear(x8, w)                                           # a stale image raises on an 8-row call
        w.mul_(0.5)
        clear_decode_weights(h)
        assert not hasattr(w, attr) and not hasattr(w, "_spa_wrows")
        assert torch.equal(linear(x8, w), y8_master)


# ------------------------------------------------------------------ 8. models
def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _llama():
    from solvingpapers_amd.models import llama3
    return llama3.Llama3(llama3.config("llama3_tiny"), device=DEV, dtype=BF, seed=1)


def _gemma():
    from solvingpapers_amd.models import gemma
    return gemma.Gemma(gemma.config("gemma_tiny"), device=DEV, dtype=BF, seed=1)


def _table(m):
    p = getattr(m, "tok_embeddings", None)
    return p if p is not None else m.embed


def _image_of(fmt, p):
    """(wq, s) of a weight by the torch formulas"""
    if fmt == "mxfp4":
        return R.quant_mxfp4(p)
    from solvingpapers_amd.ops.moe import quant_weight_fp8_blk_uncached
    wq, _, s, _ = quant_weight_fp8_blk_uncached(p.float().cpu()[None])
    return wq[0].to(p.device), s[0].to(p.device)


def _dequantised_copy(make, model, report, fmt):
    ref = make()
    ref.load_state_dict(model.state_dict())
    params = dict(model.named_parameters())
    attr = "_spa_w8" if fmt == "fp8" else "_spa_w4"
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name in report["quantized"]:
                w = dequant(fmt, *getattr(params[name], attr)[:2])
                assert torch.equal(w.to(p.dtype).float(), w)
                p.copy_(w)
    return ref.eval()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("make", [_llama, _gemma])
def test_models_decode_batch_8_from_the_images(make, fmt):
    """Batch 8, teacher-forced over 12 tokens through a ragged, paged GraphDecoder (replays only, from an empty cache)
    against the full forward of the dequantised copy, at the bound of tests/test_gemv_w8_gpu.py and
    tests/test_gemv_w4_gpu.py for this comparison (rel < 2e-2). Then slots 5..7 are parked (inactive, other tokens):
    slot 0's logits are bitwise the same."""
    torch.manual_seed(0)
    m = make().eval()
    p = _table(m)
    with torch.no_grad():                       # the table is also read by index from the masters: start it on-grid
        p.copy_(dequant(fmt, *_image_of(fmt, p.detach())))
    ids = torch.randint(0, m.c.vocab_size, (8, 12), device=DEV)
    with torch.no_grad():
        master = m(ids).float()
    rep = quantize_decode_weights(m, fmt=fmt, max_rows=16)
    assert rep["quantized"] and rep["max_rows"] == 16
    ref = _dequantised_copy(make, m, rep, fmt)
    with torch.no_grad():
        full = ref(ids).float()
        dec = GraphDecoder(m, 8, 24, ragged=True, page_size=16)
        for b in range(8):
            dec.reserve(b, 12)

        def run(tokens):
            lg = []
            for t in range(12):
                dec.ids.copy_(tokens[:, t:t + 1])
                dec.graph.replay()
                lg.append(dec.logits.clone())
            return torch.stack(lg, 1)

        dec.state.set(0)
        got = run(ids)
        print(f"{make.__name__[1:]}_tiny {fmt} batch-8 graph decode vs dequantised full forward: rel {rel(got, full):.3e}; "
              f"vs the bf16 master's logits (recorded, not asserted): {rel(got, master):.3e}")
        assert rel(got, full) < 2e-2, rel(got, full)
        dec.state.set(0)
        dec.state.active[5:] = 0
        other = ids.clone()
        other[5:] = (ids[5:] + 17) % m.c.vocab_size
        parked = run(other)
        assert torch.equal(parked[0], got[0]) and torch.equal(parked[:5], got[:5])
