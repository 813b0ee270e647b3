"""tests/gemm_oracle.py on the CPU: the spread between the two emulation orders over every case and input kind of
tests/test_gemm_tiles_gpu.py (printed, and held to gemm_oracle.SPREADS, from which the bf16 RMS margin derives);
deliberate faults applied to the kernel-order emulation at the shapes of the older GPU tests, each measured against
the older whole-tensor bound and the per-tile bound; and the CPU routes of ops.moe under the same assertions."""
import pytest
import torch

import gemm_oracle as G

BF = torch.bfloat16


def _spread_of(cs):
    return G.spread(cs["emus"][0], cs["emus"][1], cs["ref"], cs["lay"])


def _moe():
    from solvingpapers_amd.ops import moe
    return moe


def _family_cases(family):
    """Every product of one family of the GPU file as (label, out dtype, thunk -> case with both orders)."""
    two = ("kernel", "seq")
    if family == "gemm4a":
        seen = {}
        for impl in (2, 1, 0):
            for it in G.g4_list(impl):
                seen[(it[0], it[1], it[5], it[6])] = it
        for name, kind, counts, N, K, mode, acc in list(seen.values()) + G.g4_dw_list():
            yield (name, BF, lambda a=(name, kind, counts, N, K, mode, acc): G.case(*a, round_acc_first=True, orders=two))
    elif family == "gemm8":
        for cname in G.G8_CASES:
            for name, kind, counts, N, K, mode, acc in G.g8_list(cname):
                for tail in (64, 0):
                    raf = True if mode == 2 else f"g8:{tail}"
                    yield (name, BF, lambda a=(name, kind, counts, N, K, mode, acc), r=raf:
                           G.case(*a, round_acc_first=r, orders=two))
                    if mode == 2 or not acc:
                        break                      # the tail tile differs on accumulate in modes 0 / 1 only
    elif family == "moe":
        for a in G.moe_list():
            yield (a[0], BF, lambda a=a: G.case(*a, depth=16, orders=two))
    elif family == "wgrad8":
        N, K = G.WG8_NK
        for T in G.WG8_T:
            for name, kind, T_, sp, dt, acc, strided in G.wg8_list(T):
                if not strided:
                    yield (name, dt, lambda a=(name, kind, [T], N, K, 2, acc), dt=dt, sp=sp, T=T:
                           G.case(*a, orders=two, out_dtype=dt, slices=G.wgrad8_slices(T, N, K, sp)))
    elif family == "fp8":
        M = _moe()
        for op, kind, N, K in G.fp8_fwd_list():
            if op != "g8blk":                      # gemm8_fp8_blk computes grouped_gemm_fp8_blk's products
                yield (f"{op}-{kind}-N{N}-K{K}", BF, lambda a=(op, kind, N, K): G.fp8_fwd_case(M, *a, "cpu", two))
        for kind, N, dt, acc in G.fp8_wgrad_list():
            for raf in ((False, True) if acc and dt == BF else (False,)):      # wgrad_fp8_blk / wgrad8_fp8_blk
                yield (f"wgrad-{kind}-N{N}", dt, lambda a=(kind, N, dt, acc), r=raf:
                       G.fp8_wgrad_case(M, *a, "cpu", two, round_acc_first=r))


@pytest.mark.parametrize("family", list(G.SPREADS))
def test_spreads(family):
    """Worst per-unit ratio between the two emulation orders, bf16 and fp32 outputs apart. A unit that one order
    gets exactly right must be exact in the other too: the bound asks the kernel for exactness there."""
    w = [0.0, 0.0, 0.0, 0.0]
    n = 0
    cases = list(_family_cases(family))
    spreads = [_spread_of(thunk()) for _, _, thunk in cases]
    for (label, dt, _), (r, m, mismatch) in zip(cases, spreads):
        # bf16: ONE yardstick, so a unit it gets exactly right must be exact in the other order too, or the bound
        # would ask a kernel for an exactness that a legitimate order does not have. fp32: the yardstick is the
        # larger of the two orders, zero only where both are exact.
        assert mismatch == 0 or dt != BF, (label, mismatch)
        i = 0 if dt == BF else 2
        w[i], w[i + 1] = max(w[i], r), max(w[i + 1], m)
        n += 1
    print(f"SPREAD {family}: {n} products, bf16 RMS {w[0]:.4f} max-abs {w[1]:.3f}, fp32 RMS {w[2]:.3f} max-abs {w[3]:.3f}")
    assert all(got <= pin for got, pin in zip(w, G.SPREADS[family])), (family, w, G.SPREADS[family])


def test_margin_follows_spreads():
    assert G.RMS_MARGIN == 1.5 * max(v[0] for v in G.SPREADS.values()) and G.RMS_MARGIN < 2.0
    assert G.margins(BF) == (G.RMS_MARGIN, 4.0) and G.margins(torch.float32) == (4.0, 4.0)


def test_units_cover_every_element():
    for m, n in [(1, 8), (3, 8), (1, 320), (15, 264), (17, 264), (257, 264), (513, 320), (264, 520), (64, 8), (7, 24)]:
        ids, nu, first = G._unit_map(m, n)
        cnt = torch.bincount(ids.reshape(-1), minlength=nu)
        assert ids.shape == (m, n) and len(first) == nu and int(cnt.sum()) == m * n
        assert bool((cnt >= min(G.MIN_UNIT, m * n)).all()) and int(cnt.max()) <= 256 + G.MIN_UNIT, (m, n, cnt)
    lay = G.Layout(G.offsets_of(G.RAGGED), 0, (sum(G.RAGGED), 264))
    assert lay.ids.numel() == sum(G.RAGGED) * 264 and len(lay.where) == lay.n == int(lay.ids.max()) + 1
    assert {e for e, _, _ in lay.where} == {1, 2, 3, 5, 6, 7}


def test_assertion_names_the_fragment():
    cs = G.case("msg", "randn", G.RAGGED, 264, 128, 0, False)
    x = cs["emus"][0].clone()
    o = cs["off"]
    x[o[5] + 32:o[5] + 48, 48:64] *= 1.05
    with pytest.raises(AssertionError, match=r"expert 5, row block 2, column block 3"):
        G.assert_blocks(x, cs["ref"], cs["emus"][0], "msg", cs["lay"])
    cs = G.case("msg", "integer", G.RAGGED, 264, 128, 0, False)
    x = cs["emus"][0].clone()
    x[o[7] + 17, 250] += 1
    with pytest.raises(AssertionError, match=r"must be exact.*expert 7, row block 1, column block 15"):
        G.assert_blocks(x, cs["ref"], cs["emus"][0], "msg", cs["lay"])


# ------------------------------------------------------------------ mutations
def _g4_shape(counts, mode, acc=False):
    """The operands of tests/test_gemm4a_gpu.py test_gemm4a_modes_match_fp32 (N, K = 320, 512; W scaled by 0.05)."""
    g = torch.Generator().manual_seed(len(counts))
    E, Mt, N, K = len(counts), sum(counts), 320, 512
    x = torch.randn(Mt, K, generator=g).to(BF)
    if mode == 0:
        a, w = x, (torch.randn(E, N, K, generator=g) * 0.05).to(BF)
    elif mode == 1:
        a, w = torch.randn(Mt, 2 * N, generator=g).to(BF), (torch.randn(E, 2 * N, K, generator=g) * 0.05).to(BF)
    else:
        a, w = torch.randn(Mt, 2 * N, generator=g).to(BF), x
    shape = G.out_shape(a, w, G.offsets_of(counts), mode)
    c = torch.randn(shape, generator=g).to(BF) if acc else None
    return a, w, c


def _moe_shape(counts, N, K):
    """The forward operands of tests/test_moe_gpu.py test_grouped_gemm_all_modes."""
    g = torch.Generator().manual_seed(3)
    return torch.randn(sum(counts), K, generator=g).to(BF), (torch.randn(len(counts), N, K, generator=g) / K ** 0.5).to(BF), None


def _verdict(x, ref, yard, lay, old_bound):
    """(passes the older whole-tensor bound, fails the per-tile bound, the whole-tensor figure)."""
    r = G.rel(x, ref)
    try:
        G.assert_blocks(x, ref, yard, "mutation", lay)
        caught = False
    except AssertionError:
        caught = True
    return r < old_bound, caught, r


MOE_COUNTS = [300, 0, 129, 1, 64, 700, 0, 33]
BAL16 = [768] * 16
# (mutation, shape) -> does it pass the older bound there? Measured here; the per-tile bound catches every one.
MUTATIONS = [
    ("drop_last_slice", "g4-ragged", True), ("drop_last_slice", "moe-256x512", True),
    ("next_expert_row", "g4-ragged", False), ("next_expert_row", "g4-bal16", False), ("next_expert_row", "moe-1408x2048", False),
    ("extra_token_dw", "g4-bal16-dw", True),
    ("unwritten_cols", "g4-ragged", False), ("unwritten_cols", "g4-bal16", False), ("unwritten_cols", "moe-1408x2048", False),
    ("truncate", "g4-ragged", True), ("truncate", "moe-256x512", True),
    ("acc_ignores_c", "g4-bal16-dw", True), ("acc_twice", "g4-bal16-dw", True),
    ("swap_fragments", "g4-ragged", False), ("swap_fragments", "g4-dense", False), ("swap_fragments", "moe-1408x2048", False),
]


def _shape(sname):
    if sname == "g4-ragged":
        return G.RAGGED, 0, _g4_shape(G.RAGGED, 0)
    if sname == "g4-bal16":
        return BAL16, 0, _g4_shape(BAL16, 0)
    if sname == "g4-dense":
        return [4096], 0, _g4_shape([4096], 0)
    if sname == "g4-bal16-dw":
        return BAL16, 2, _g4_shape(BAL16, 2, acc=True)
    N, K = (256, 512) if sname == "moe-256x512" else (1408, 2048)
    return MOE_COUNTS, 0, _moe_shape(MOE_COUNTS, N, K)


@pytest.mark.parametrize("mut,sname,passes_old", MUTATIONS)
def test_mutation(mut, sname, passes_old):
    """A deliberate fault in the kernel-order emulation at a shape of the older GPU tests: the per-tile bound fails
    it; whether the older ``rel < 1e-2`` passes it is recorded in MUTATIONS and held."""
    counts, mode, (a, w, c) = _shape(sname)
    o = G.offsets_of(counts)
    kw = dict(round_acc_first=True)
    if mut not in ("acc_ignores_c", "acc_twice"):
        c = None
    if mut == "extra_token_dw":
        c = None
    ref = G.ref64(a, w, o, mode, c)
    lay = G.layout_of(tuple(counts), mode, tuple(ref.shape))
    yard = G.emulate(a, w, o, mode, "kernel", BF, c, **kw)
    x = yard.clone()
    big = max(range(len(counts)), key=lambda e: counts[e])
    r0 = o[big]
    if mut == "drop_last_slice":
        K = a.shape[1]
        short = G.emulate(a[:, :K - 32], w[:, :, :K - 32], o, mode, "kernel", BF)
        x[r0 + 16:r0 + 32, 32:48] = short[r0 + 16:r0 + 32, 32:48]
    elif mut == "next_expert_row":
        e = next(e for e in range(len(counts) - 1) if counts[e] > 0 and counts[e + 1] > 0)
        row = o[e + 1] - 1
        x[row] = G.emulate(a[row:row + 1], w[e + 1:e + 2], [0, 1], mode, "kernel", BF)[0]
    elif mut == "extra_token_dw":
        x[3] = G.emulate(a[o[3]:o[4] + 1], w[o[3]:o[4] + 1], [0, counts[3] + 1], 2, "kernel", BF)[0]
    elif mut == "unwritten_cols":
        x[r0:r0 + 256, -8:] = 0
    elif mut == "truncate":
        x = G.emulate(a, w, o, mode, "kernel", BF, rounding="trunc")
    elif mut == "acc_ignores_c":
        x[3, :256, 256:512] = G.emulate(a, w, o, mode, "kernel", BF)[3, :256, 256:512]
    elif mut == "acc_twice":
        x[3, :256, 256:512] = G.emulate(a, w, o, mode, "kernel", BF, 2 * c, **kw)[3, :256, 256:512]
    elif mut == "swap_fragments":
        blk = x[r0 + 128:r0 + 160, 128:256].clone()
        x[r0 + 128:r0 + 144, 128:256], x[r0 + 144:r0 + 160, 128:256] = blk[16:], blk[:16]
    assert not torch.equal(x, yard)
    old, caught, r = _verdict(x, ref, yard, lay, 1e-2)
    print(f"MUTATION {mut} at {sname}: whole-tensor rel {r:.4f} ({'passes' if old else 'fails'} 1e-2), per-tile bound "
          f"{'fails it' if caught else 'PASSES it'}")
    assert caught
    assert old == passes_old, r


@pytest.mark.parametrize("expert,passes_old", [(3, True), (4, False)])
def test_mutation_fp8_scale_byte(expert, passes_old):
    """One E8M0 weight-block scale off by one exponent at the shape of test_grouped_gemm_fp8_blk_exact_on_dequantized
    (E 8 ragged, N 384, K 512, x ramped): on the expert with one row it passes the older ``rel < 5e-3``."""
    M = _moe()
    g = torch.Generator().manual_seed(2)
    counts = MOE_COUNTS
    E, N, K, Mt, o = len(counts), 384, 512, sum(counts), G.offsets_of(counts)
    x = (torch.randn(Mt, K, generator=g) * torch.logspace(-2, 1, K)).to(BF)
    W = (torch.randn(E, N, K, generator=g) * 0.05).to(BF)
    xq, sx = M.quant_act_fp8_blk(x)
    wq, _, sw, _ = M.quant_weight_fp8_blk_uncached(W)
    xd, wd = G.deq_act_blk(xq, sx), G.deq_w_blk(wq, sw)
    ref = G.ref64(xd, wd, o, 0)
    lay = G.layout_of(tuple(counts), 0, tuple(ref.shape))
    yard = G.emulate(xd, wd, o, 0, "kernel", BF, depth=128)
    sw2 = sw.clone()
    sw2[expert, 1, 2] += 1
    bad = G.emulate(xd, G.deq_w_blk(wq, sw2), o, 0, "kernel", BF, depth=128)
    old, caught, r = _verdict(bad, ref, yard, lay, 5e-3)
    print(f"MUTATION fp8 scale byte, expert {expert}: whole-tensor rel {r:.4f}, per-tile bound "
          f"{'fails it' if caught else 'PASSES it'}")
    assert caught
    assert old == passes_old, r


# ------------------------------------------------------------------ the CPU routes
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_cpu_routes(mode, kind):
    """ops.moe._cpu_grouped and grouped_gemm(out=, accumulate) on CPU tensors under the per-tile bound. The CPU
    route adds a bf16 product onto ``out``: round_acc_first."""
    M = _moe()
    counts, N, K = G.MOE_COUNTS, 200, 136
    cs = G.case("cpu-route", kind, counts, N, K, mode, True, round_acc_first=True)
    off = torch.tensor(cs["off"], dtype=torch.int32)
    plain = G.emulate(cs["a"], cs["w"], cs["off"], mode)
    ref0 = G.ref64(cs["a"], cs["w"], cs["off"], mode)
    G.assert_blocks(M._cpu_grouped(cs["a"], cs["w"], off, mode), ref0, plain, "_cpu_grouped", cs["lay"])
    G.assert_blocks(M.grouped_gemm(cs["a"], cs["w"], off, mode), ref0, plain, "grouped_gemm", cs["lay"])
    out = torch.full(ref0.shape, float("nan"), dtype=BF)
    assert M.grouped_gemm(cs["a"], cs["w"], off, mode, out=out) is out
    G.assert_blocks(out, ref0, plain, "grouped_gemm out=", cs["lay"])
    out = cs["c"].clone()
    M.grouped_gemm(cs["a"], cs["w"], off, mode, out=out, accumulate=True)
    G.assert_blocks(out, cs["ref"], cs["emus"][0], "grouped_gemm accumulate", cs["lay"])
    if kind == "integer":
        assert torch.equal(out.double(), cs["ref"])
