"""The hand-written MFMA GEMMs per 16 x 16 output tile against an fp64 oracle (tests/gemm_oracle.py): every pipeline
of gemm4a.hip (ring, gemm4r, gemm4d), gemm8.hip (grouped_gemm8, wgrad8 and its reduce on either kind of partials),
the six tile shapes of moe.hip's grouped_gemm, and the fp8 products of moe_fp8.hip / gemm8_fp8.hip. Each kernel's
RMS and max-abs error per unit is held to a small multiple of the error of an fp32-accumulate emulation on the same
inputs (margins: gemm_oracle's docstring); the fp64 references are formed on the device, once per product, and
shared between the pipelines that compute it.

Input kinds: "randn", "ramped" (the reduction scaled by logspace(-2, 1)) and "integer" (entries in {-1, 0, 1}, at
most 192 live reduction indices and an old ``out`` in [-64, 64]: every partial sum and every output is an integer
of magnitude <= 256, exact in fp32 and in bf16, so the kernel must match bitwise and a mis-mapped fragment, a missed
wait or a stale LDS image is an exact mismatch with coordinates).

Output guards: wherever the op takes ``out=``, ``out`` is a contiguous view between guard rows filled with a NaN
bit pattern, which must be bitwise unchanged afterwards; without ``accumulate`` the view itself is prefilled with
the pattern, so that an element left unwritten, or an old value read, is a NaN in the result. The ops that allocate
their output themselves (gemm8_fp8_blk, grouped_gemm_fp8, grouped_gemm_fp8_blk, wgrad8's fp32 partials) carry no
guards.

Variants run: SPA_G4_SCHED=1 (the ring's DMA after the MFMA stream: the same product) and SPA_G4_POL 1 / 2 (cache
policies of gemm4r's loads). SPA_G4_SCHED 2-5 and SPA_GG8_ABLATE 1-3 compute wrong results by construction
(gemm4a.hip:323) and are not run. Each test prints its worst kernel / yardstick ratios.
"""
import pytest
import torch

import gemm_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
BF16_NAN, F32_NAN = 0x7FA5, 0x7FA5A5A5
_CACHE = {}
_WORST = {}


def _ops():
    from solvingpapers_amd.ops._ext import ops
    return ops()


def _cached(family, key, make):
    """One reference per product, shared by the pipelines of a family (dropped when another family starts)."""
    if _CACHE.get("family") != family:
        _CACHE.clear()
        _CACHE["family"] = family
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _off(o):
    return torch.tensor(o, dtype=torch.int32, device=DEV)


def _guarded(shape, dtype, c):
    """(buffer, out): ``out`` a contiguous view of ``shape`` between GUARD rows of NaN pattern; prefilled with the
    pattern, or with ``c`` (accumulate)."""
    cols = shape[-1]
    rows = 1
    for s in shape[:-1]:
        rows *= s
    it, pat = (torch.int16, BF16_NAN) if dtype == torch.bfloat16 else (torch.int32, F32_NAN)
    buf = torch.full((rows + 2 * GUARD, cols), pat, dtype=it, device=DEV).view(dtype)
    out = buf[GUARD:GUARD + rows].view(shape)
    if c is not None:
        out.copy_(c.view(shape))
    assert out.is_contiguous() and out.data_ptr() % 16 == 0
    return buf, out


def _guards_intact(buf, name):
    it, pat = (torch.int16, BF16_NAN) if buf.dtype == torch.bfloat16 else (torch.int32, F32_NAN)
    b = buf.view(it)
    assert bool((b[:GUARD] == pat).all()) and bool((b[-GUARD:] == pat).all()), f"{name}: guard rows written"


def _note(family, r):
    w = _WORST.setdefault(family, [0.0, 0.0])
    w[0], w[1] = max(w[0], r[0]), max(w[1], r[1])


def _check(family, name, cs, run, integer, yard2=None):
    """Run ``run(out, accumulate)`` on a guarded output and hold the result to the case's bound."""
    ref = cs["ref"]
    if integer:
        assert ref.abs().max().item() <= 256, name
    buf, out = _guarded(tuple(ref.shape), cs["emus"][0].dtype, cs["c"])
    res = run(out, cs["c"] is not None)
    assert res.data_ptr() == out.data_ptr(), f"{name}: the op did not write into out"
    _guards_intact(buf, name)
    r = G.assert_blocks(out, ref, cs["emus"][0], name, cs["lay"], yard2)
    if integer:
        assert torch.equal(out.double(), ref), name
    _note(family, r)


def _report(family):
    w = _WORST.get(family, [0.0, 0.0])
    print(f"GEMMTILES {family}: worst kernel / yardstick RMS {w[0]:.3f} max-abs {w[1]:.3f}")


# ------------------------------------------------------------------ gemm4a modes 0 / 1
def _g4_rows(impl, items, tag=""):
    ops = _ops()
    for name, kind, counts, N, K, mode, acc in items:
        cs = _cached("g4", (name, kind, mode, acc), lambda: G.case(name, kind, counts, N, K, mode, acc,
                                                                    round_acc_first=True, device=DEV))
        off = _off(cs["off"])
        _check("gemm4a", f"gemm4a impl {impl}{tag} mode {mode} {name} {kind} acc {acc}", cs,
               lambda out, a_: ops.gemm4a(cs["a"], cs["w"], off, mode, out, a_, impl), kind == "integer")


@pytest.mark.parametrize("impl,K", [(i, K) for i in (2, 1, 0) for K in G.G4_RED[i]])
def test_gemm4a_rows(impl, K):
    """Modes 0 / 1 of the three pipelines: reduction lengths over every residue of the unroll (ring by 4, two-buffer
    by 2) and below the ring's depth, ragged / empty / single-row experts, one full tile, a dense 1300 rows (four row
    tiles and a partial group at the default SPA_G4_GM), N of 8, 264 and 320, with and without accumulate."""
    _g4_rows(impl, [it for it in G.g4_list(impl) if it[4] == K])
    _report("gemm4a")


@pytest.mark.parametrize("gm", ["1", "3"])
@pytest.mark.parametrize("impl", [2, 1, 0])
def test_gemm4a_dense_tile_groups(impl, gm, monkeypatch):
    monkeypatch.setenv("SPA_G4_GM", gm)
    _g4_rows(impl, [it for it in G.g4_list(impl) if it[4] == 128 and it[2] == G.G4_COUNTS["dense"]], f" GM {gm}")
    _report("gemm4a")


# ------------------------------------------------------------------ gemm4a mode 2
def _g4_dw(impl, items, tag=""):
    ops = _ops()
    for name, kind, counts, N, K, mode, acc in items:
        cs = _cached("g4dw", (name, kind, acc), lambda: G.case(name, kind, counts, N, K, 2, acc,
                                                                round_acc_first=True, device=DEV))
        off = _off(cs["off"])
        _check("gemm4a_dw", f"gemm4a impl {impl}{tag} dW {name} {kind} acc {acc}", cs,
               lambda out, a_: ops.gemm4a(cs["a"], cs["w"], off, 2, out, a_, impl), kind == "integer")


@pytest.mark.parametrize("layout", list(G.G4_DW_LAYOUTS))
@pytest.mark.parametrize("impl", [2, 1, 0])
def test_gemm4a_dw(impl, layout):
    """Per-expert dW: token counts on both sides of a K-tile edge, the tile-to-expert mappings (balanced E % 8 == 0:
    snake order over tied ranks; skewed; E = 5; E = 16; E = 256 with many equal and many empty experts). With
    accumulate an expert mapped twice doubles its product and one never mapped keeps its old value; without, one
    never mapped keeps the NaN prefill."""
    _g4_dw(impl, [it for it in G.g4_dw_list() if it[0].startswith(layout + "-")])
    _report("gemm4a_dw")


@pytest.mark.parametrize("var,val,impl", [("SPA_G4_SCHED", "1", 0), ("SPA_G4_POL", "1", 1), ("SPA_G4_POL", "2", 1)])
def test_gemm4a_variants(var, val, impl, monkeypatch):
    """The variants the source describes as the same product: SPA_G4_SCHED=1 in all three modes of the ring,
    SPA_G4_POL 1 / 2 in gemm4r's mode 0."""
    monkeypatch.setenv(var, val)
    K = 160 if impl == 0 else 192
    rows = [it for it in G.g4_list(impl) if it[4] == K and it[3] == 264 and it[2] == G.RAGGED]
    if var == "SPA_G4_POL":
        rows = [it for it in rows if it[5] == 0]
    _g4_rows(impl, rows, f" {var}={val}")
    if var == "SPA_G4_SCHED":
        _g4_dw(impl, [it for it in G.g4_dw_list() if it[0] == "e5-N264-K520"], f" {var}={val}")
    _report("gemm4a")


# ------------------------------------------------------------------ gemm8
def _g8(cname, tail, tag=""):
    ops = _ops()
    for name, kind, counts, N, K, mode, acc in G.g8_list(cname):
        raf = True if mode == 2 else f"g8:{tail}"
        cs = _cached("g8", (name, kind, mode, acc, raf), lambda: G.case(name, kind, counts, N, K, mode, acc,
                                                                         round_acc_first=raf, device=DEV))
        off = _off(cs["off"])
        _check("gemm8", f"gemm8 tail {tail}{tag} mode {mode} {name} {kind} acc {acc}", cs,
               lambda out, a_: ops.grouped_gemm8(cs["a"], cs["w"], off, mode, out, a_), kind == "integer")


@pytest.mark.parametrize("tail", ["64", "0"])
@pytest.mark.parametrize("cname", list(G.G8_CASES))
def test_gemm8(cname, tail, monkeypatch):
    """grouped_gemm8 at test_grouped_gemm8_elementwise's cases (shrunk), all modes, with accumulate in every mode,
    on the 64-row tail tiles (which round acc + C once) and without them."""
    monkeypatch.setenv("SPA_GG8_TAIL", tail)
    _g8(cname, int(tail))
    _report("gemm8")


@pytest.mark.parametrize("gm", ["1", "3"])
def test_gemm8_dense_tile_groups(gm, monkeypatch):
    monkeypatch.setenv("SPA_G8_GM", gm)
    _g8("dense", 64, f" GM {gm}")
    _report("gemm8")


# ------------------------------------------------------------------ moe.hip grouped_gemm
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5])
def test_moe_grouped_gemm_cfgs(cfg):
    """The six tile shapes through the op's ``cfg`` argument, all modes, reduction lengths that are no multiple of
    the shape's BK (8, 40, 72, 136), N of 8 and 200."""
    ops = _ops()
    for name, kind, counts, N, K, mode, acc in G.moe_list():
        cs = _cached("moe", (name, kind, mode, acc), lambda: G.case(name, kind, counts, N, K, mode, acc, depth=16,
                                                                     device=DEV))
        off = _off(cs["off"])
        _check("moe", f"grouped_gemm cfg {cfg} mode {mode} {name} {kind} acc {acc}", cs,
               lambda out, a_: ops.grouped_gemm(cs["a"], cs["w"], off, mode, out, a_, cfg), kind == "integer")
    _report("moe")


# ------------------------------------------------------------------ wgrad8
def _wg8_case(name, kind, T, sp, dt, acc):
    N, K = G.WG8_NK
    return G.case(name, kind, [T], N, K, 2, acc, device=DEV, orders=("kernel", "seq"), out_dtype=dt,
                  slices=G.wgrad8_slices(T, N, K, sp))


def _widen(t):
    """The operand as a column slice of a wider tensor (row stride > width, % 8; 16-byte aligned)."""
    wide = torch.full((t.shape[0], t.shape[1] + 24), float("nan"), dtype=t.dtype, device=t.device)
    wide[:, 8:8 + t.shape[1]] = t
    return wide[:, 8:8 + t.shape[1]]


@pytest.mark.parametrize("T", G.WG8_T)
@pytest.mark.parametrize("g4", ["1", "0"])
def test_wgrad8(g4, T, monkeypatch):
    """The dense split-K weight gradient on gemm4r's partials and (SPA_WGRAD_G4=0) on the 8-phase kernel's: splits 0
    (default), 1, 3 and 100 (clamped to T / 512), bf16 and fp32 ``out``, accumulate, operands that are column slices
    of wider tensors. T = 0: the op zeroes ``out``, or with accumulate leaves it (gemm8.hip wgrad8)."""
    monkeypatch.setenv("SPA_WGRAD_G4", g4)
    ops = _ops()
    for name, kind, T_, sp, dt, acc, strided in G.wg8_list(T):
        cs = _cached("wg8", (name, kind, sp, dt, acc), lambda: _wg8_case(name, kind, T, sp, dt, acc))
        dy, x = (_widen(cs["a"]), _widen(cs["w"])) if strided else (cs["a"], cs["w"])
        cs1 = dict(cs, ref=cs["ref"][0], emus=[e[0] for e in cs["emus"]], c=None if cs["c"] is None else cs["c"][0])
        fam = "wgrad8_bf16" if dt == torch.bfloat16 else "wgrad8_fp32"
        _check(fam, f"wgrad8 G4={g4} T {T} splits {sp} {dt} {kind} acc {acc} strided {strided}", cs1,
               lambda out, a_: ops.wgrad8(dy, x, out, a_, sp), kind == "integer",
               yard2=None if dt == torch.bfloat16 else cs1["emus"][1])
    _report("wgrad8_bf16")
    _report("wgrad8_fp32")


class _Recorder:
    """Stands in for the op namespace and records which ops the Python dispatch calls."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self.real, name)


@pytest.mark.parametrize("T,routed", [(4096, True), (4088, False)])
def test_layout_wgrad_routing(T, routed, monkeypatch):
    """ops.layout.wgrad sends a narrow-operand product to wgrad8 from WGRAD8_MIN_TOKENS tokens on."""
    from solvingpapers_amd.ops import layout, _ext
    assert layout.WGRAD8 and layout.WGRAD8_MIN_TOKENS == 4096
    rec = _Recorder(_ext.ops())
    monkeypatch.setattr(layout._ext, "ops", lambda: rec)
    N, K = G.WG8_NK
    cs = _wg8_case(f"route-T{T}", "randn", T, 0, torch.bfloat16, False)
    got = layout.wgrad(cs["a"], cs["w"])
    assert ("wgrad8" in rec.calls) == routed, rec.calls
    if routed:
        _note("wgrad8_bf16", G.assert_blocks(got.view(1, N, K), cs["ref"], cs["emus"][0], f"layout.wgrad T {T}", cs["lay"]))
    else:
        assert G.rel(got, cs["ref"][0]) < 1e-2


# ------------------------------------------------------------------ fp8
def _moe():
    from solvingpapers_amd.ops import moe
    return moe


@pytest.mark.parametrize("K", G.FP8_K)
@pytest.mark.parametrize("op", ["rows", "blk", "g8blk"])
def test_fp8_forward(op, K):
    """grouped_gemm_fp8 (row scales), grouped_gemm_fp8_blk and gemm8_fp8_blk against the product of the dequantised
    operands per tile: 1, 2 and 8 K-tiles, N of 264 and 384, ragged and empty experts, block scales that differ by
    6-10 exponents between neighbouring blocks, and the integer kind where the quantiser keeps the integers."""
    M, ops = _moe(), _ops()
    fn = {"rows": ops.grouped_gemm_fp8, "blk": ops.grouped_gemm_fp8_blk, "g8blk": ops.gemm8_fp8_blk}[op]
    ran_integer = False
    for op_, kind, N, K_ in G.fp8_fwd_list():
        if op_ != op or K_ != K:
            continue
        cs = _cached("fp8", ("blk" if op == "g8blk" else op, kind, N, K), lambda: G.fp8_fwd_case(M, op, kind, N, K, DEV))
        integer = kind == "integer"
        if integer and not cs["exact"]:
            continue                        # the row quantiser's amax / 448 does not reproduce the integers
        ran_integer |= integer
        name = f"fp8 {op} N {N} K {K} {kind}"
        if integer:
            assert cs["ref"].abs().max().item() <= 256
        y = fn(*cs["args"])
        _note("fp8_fwd", G.assert_blocks(y, cs["ref"], cs["emus"][0], name, cs["lay"]))
        if integer:
            assert torch.equal(y.double(), cs["ref"]), name
    assert ran_integer or op == "rows"
    _report("fp8_fwd")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("op", ["wgrad_fp8_blk", "wgrad8_fp8_blk"])
def test_fp8_wgrad(op, dt):
    """The fp8 expert dW of both kernels on the padded 128-token segments of quant_t_fp8_seg (1, 2 and 8 K-tiles, an
    empty expert), bf16 and fp32 outputs with and without accumulate.

    The fp32 outputs resolve the summation inside the block-scaled e4m3 MFMA, which cuts every product of a group
    of 8 k to 13 bits below the group's largest exponent sum (gemm_oracle's mfma_f8_dot8, tools/probe_fp8_mfma.py):
    against exact products accumulated in fp32 both kernels sit 2^-14.6 of a unit's largest value away, 18151 -
    39992 x that emulation's RMS error, with identical figures; against the emulation that cuts the products as the
    instruction does they measure 1.000 x (max-abs 1.003 x). The bf16 cases do not resolve it (1.00 - 1.05 x)."""
    M, ops = _moe(), _ops()
    fn = getattr(ops, op)
    tag = "bf16" if dt == torch.bfloat16 else "fp32"
    for kind, N, dt_, acc in G.fp8_wgrad_list():
        if dt_ != dt:
            continue
        raf = op == "wgrad8_fp8_blk" and acc and dt == torch.bfloat16          # gemm8_fp8.hip:466, :482
        cs = _cached("fp8wg", (kind, N, dt, acc, raf), lambda: G.fp8_wgrad_case(M, kind, N, dt, acc, DEV,
                                                                                round_acc_first=raf))
        integer = kind == "integer" and cs["exact"]
        _check(f"fp8_wgrad_{tag}", f"{op} N {N} {dt} {kind} acc {acc}", cs, lambda out, a_: fn(*cs["args"], out, a_),
               integer, yard2=None if dt == torch.bfloat16 else cs["emus"][1])
    _report(f"fp8_wgrad_{tag}")


# ------------------------------------------------------------------ routing of ops.moe.grouped_gemm / grouped_linear
def test_grouped_gemm_routing(monkeypatch):
    """At default settings: modes 0 / 1 with a reduction % 64 -> grouped_gemm8, otherwise moe.hip's grouped_gemm;
    mode 2 -> gemm4a (gemm4r) up to 256 experts, grouped_gemm8 above."""
    M = _moe()
    assert M.GG8 and M.GG_DW_G4
    rec = _Recorder(M.ops())
    monkeypatch.setattr(M, "ops", lambda: rec)

    def routed(counts, N, K, mode, want, depth=32, raf=False):
        cs = G.case(f"route-E{len(counts)}-N{N}-K{K}", "randn", counts, N, K, mode, False, depth=depth, device=DEV)
        rec.calls.clear()
        got = M.grouped_gemm(cs["a"], cs["w"], _off(cs["off"]), mode)
        assert rec.calls == [want], (mode, N, K, rec.calls)
        G.assert_blocks(got, cs["ref"], cs["emus"][0], f"grouped_gemm -> {want} mode {mode}", cs["lay"])

    for mode in (0, 1):
        routed(G.RAGGED, 264, 128, mode, "grouped_gemm8")
        routed(G.RAGGED, 264, 72, mode, "grouped_gemm", depth=16)
    routed(G.G4_DW_LAYOUTS["e5"], 264, 520, 2, "gemm4a")
    routed([(i * 7) % 5 for i in range(300)], 264, 136, 2, "grouped_gemm8")      # E > 256: gemm4a takes at most 256

    from solvingpapers_amd.ops.moe import MoEPlan
    counts = G.RAGGED
    a, w, _ = G.make_inputs("randn", counts, 320, 128, 0, 11)      # both reductions (128 forward, 320 dX) % 64
    a, w = a.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    off = _off(G.offsets_of(counts))
    plan = MoEPlan(None, None, off, off[1:] - off[:-1], 1, sum(counts))
    rec.calls.clear()
    y = M.grouped_linear(a, w, plan)
    assert rec.calls == ["grouped_gemm8"], rec.calls
    rec.calls.clear()
    y.backward(torch.ones_like(y))
    assert sorted(rec.calls) == ["gemm4a", "grouped_gemm8"], rec.calls
    assert a.grad is not None and w.grad is not None
