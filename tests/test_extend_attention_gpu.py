"""Extend attention on the GPU (csrc/kernels/attention_extend.hip): attn_extend / attn_extend_paged, many
query rows against a cache whose length comes per sequence from the device.

NaN stands in every row that must not be read (cache rows at or past a length, unused pages, the null
page, each last page's tail), so a finite result proves none was. Per sequence the result is held to the
tile bounds of tests/attn_oracle.py with the module's own margins (RMS 2.13, max-abs 4.0, lse 4.0). The
bf16 yardstick is emulate_bf16(order="blockwise", block=32, defer_log2=8.0): the kernel keeps the flash
forward's deferred rescale (its file header says so). The lse yardsticks are the fp32 ones of
tests/test_attention_tiles_gpu.py (the kernel sums l in fp32 before P is rounded): the fp32 emulation in
both orders and lse_log2_fp32. The paged op is bitwise the contiguous one; the wrappers return the ops'
bits; the decode kernel on groups of 16 / G tokens agrees with the extend result within the same bound (the
difference of the two results against the yardstick's error, at the same margins); bad calls raise; and the oracle run on lengths one too
short fails the bound, so the bound sees an off-by-one in a length. The issue's cases run over TK = 300 cache
rows, where the launch never splits along the keys; a second set over 640 rows runs the key-split path."""
import functools
import math

import pytest
import torch

import attn_oracle as A
from solvingpapers_amd.ops import _ext, reference as R
from solvingpapers_amd.ops.attention import PagedKV, decode_attention, kv_cache_attend

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
TK = 300
DEFER_LOG2 = 8.0    # attention_extend.hip keeps kRescaleThr

SHAPES = [
    # B, H, Hkv, hd, lens (each raised to at least Tq)
    (3, 8, 2, 128, (0, 65, 300)),
    (2, 4, 1, 64, (129, 300)),
    (2, 4, 1, 256, (33, 300)),
]
# Tq 17: the first row count past the decode kernel's 16 at G = 1; 40: a full 32-row wave tile and a
# ragged one; 130 (hd 128 only): a second 128-row query block
CASES = [(si, Tq, TK) for si in range(3) for Tq in (17, 40)] + [(0, 130, TK)]
# The launch splits a small grid along the keys only when every split keeps 256 cache rows: never at TK = 300.
# The same checks over 640 cache rows run the two-split path and its merge (a sequence of Tq rows has one
# key tile: its second split is empty).
TK2 = 640
LENS2 = [(0, 321, 640), (257, 640), (129, 640)]
CASES += [(0, 40, TK2), (1, 17, TK2), (2, 40, TK2), (0, 130, TK2)]
PAGES = (16, 64)


def i32(x):
    return torch.tensor(x, device=DEV, dtype=torch.int32)


def kv_rows(shape, lo, hi, gen):
    e = torch.randint(lo, hi + 1, (*shape[:-1], 1), device=DEV, generator=gen)
    return (torch.randn(*shape, device=DEV, generator=gen) * torch.exp2(e.float())).to(BF)


def build_pools(k, v, lens, page, table):
    """Pools of ``P`` pages holding rows [0, lens[b]) of k / v [B, TK, Hkv, hd] through ``table`` (host
    int [B, NP]); every other pool row -- unused pages, the null page, each last page's tail -- is NaN."""
    B, _, Hkv, hd = k.shape
    P = 2 * int(sum(-(-n // page) for n in lens)) + 1
    kp = torch.full((P, page, Hkv, hd), float("nan"), device=DEV, dtype=BF)
    vp = torch.full((P, page, Hkv, hd), float("nan"), device=DEV, dtype=BF)
    bt = table.to(DEV, torch.int32).contiguous()
    for b, n in enumerate(lens):
        rows = R.paged_rows(bt[b:b + 1], torch.arange(n, device=DEV), page)[0]
        kp.view(-1, Hkv, hd)[rows] = k[b, :n]
        vp.view(-1, Hkv, hd)[rows] = v[b, :n]
    return kp, vp, bt


def tables(lens, page, seed, tk):
    B, NP = len(lens), -(-tk // page)
    used = [-(-n // page) for n in lens]
    P = 2 * sum(used) + 1
    ident, perm = torch.zeros(B, NP, dtype=torch.int64), torch.zeros(B, NP, dtype=torch.int64)
    order = (torch.randperm(P - 1, generator=torch.Generator().manual_seed(seed)) + 1).tolist()
    nxt = 1
    for b, u in enumerate(used):        # entries past a sequence's pages stay 0: never read
        ident[b, :u] = torch.arange(nxt, nxt + u)
        perm[b, :u] = torch.tensor(order[nxt - 1:nxt - 1 + u])
        nxt += u
    return ident, perm


def oracle(q, k, v, n, sc):
    """(ref64 (O, lse), bf16 yardstick O, fp32 lse yardsticks) of one sequence over its first n rows."""
    kb, vb = k[:, :n], v[:, :n]
    do = torch.ones_like(q)
    ref = A.ref64(q, kb, vb, do, True, sc)
    yard = A.emulate_bf16(q, kb, vb, do, True, sc, order="blockwise", block=32, defer_log2=DEFER_LOG2)
    ylse = [A.emulate_fp32(q, kb, vb, do, True, sc)[1],
            A.emulate_fp32(q, kb, vb, do, True, sc, order="blockwise", block=16)[1],
            A.lse_log2_fp32(q, kb, True, sc)]
    return ref[0], ref[1], yard[0], ylse


@functools.lru_cache(maxsize=None)
def data(si, Tq, tk=TK):
    """q, the contiguous cache (NaN at and past each length), per page size an identity-table and a
    shuffled-table pool of the same rows, the lengths, the ops' results on the contiguous cache and the
    per-sequence oracle: built once per (shape, Tq, cache rows)."""
    B, H, Hkv, hd, lens = SHAPES[si]
    lens = tuple(max(n, Tq) for n in (lens if tk == TK else LENS2[si]))
    g = torch.Generator(device=DEV).manual_seed(100 * si + Tq + tk)
    q = torch.randn(B, Tq, H, hd, device=DEV, generator=g).to(BF)
    k, v = kv_rows((B, tk, Hkv, hd), -3, 0, g), kv_rows((B, tk, Hkv, hd), -6, 6, g)
    pools = {}
    for page in PAGES:
        ident, perm = tables(lens, page, si + page, tk)
        pools[page] = {"ident": build_pools(k, v, lens, page, ident), "perm": build_pools(k, v, lens, page, perm)}
    kn, vn = k.clone(), v.clone()
    for b, n in enumerate(lens):
        kn[b, n:] = float("nan")
        vn[b, n:] = float("nan")
    sc = 1 / math.sqrt(hd)
    out, lse = _ext.ops().attn_extend(q, kn, vn, sc, i32(lens), True)
    orc = [oracle(q[b:b + 1], k[b:b + 1], v[b:b + 1], n, sc) for b, n in enumerate(lens)]
    return q, kn, vn, pools, lens, sc, (out, lse), orc


def check_bounds(name, out, lse, orc):
    """(b) of every sequence; returns the sequences that failed, with the message."""
    failed = []
    for b, (o64, l64, yard, ylse) in enumerate(orc):
        try:
            rr, rm = A.assert_tiles(out[b:b + 1], o64, yard, f"{name} b{b} O")
            rl = A.assert_lse(lse[b:b + 1], l64, ylse, f"{name} b{b} lse")
            print(f"{name} b{b}: O rms {float(rr):.2f} maxabs {float(rm):.2f} lse {float(rl):.2f}")
        except AssertionError as e:
            failed.append((b, str(e)))
    return failed


@pytest.mark.parametrize("si,Tq,tk", CASES)
def test_contiguous_finite_and_bounds(si, Tq, tk):
    q, kn, vn, pools, lens, sc, (out, lse), orc = data(si, Tq, tk)
    # (a) no NaN: no cache row at or past a sequence's length was read
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    # (b) per sequence, per 32-row tile
    failed = check_bounds(f"s{si} Tq{Tq} Tk{tk}", out, lse, orc)
    assert not failed, failed


@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("si,Tq,tk", CASES)
def test_paged_bitwise(si, Tq, tk, page):
    q, kn, vn, pools, lens, sc, (out, lse), _ = data(si, Tq, tk)
    op = _ext.ops().attn_extend_paged
    kp, vp, bt = pools[page]["perm"]
    po, pl = op(q, kp, vp, bt, sc, tk, i32(lens), True)
    # (a) no NaN: no unused page, no null-page row, no tail of a last page was read
    assert torch.isfinite(po).all() and torch.isfinite(pl).all()
    # (c) the shuffled table, the identity table and the contiguous cache: the same bits
    ki, vi, bi = pools[page]["ident"]
    io, il = op(q, ki, vi, bi, sc, tk, i32(lens), True)
    assert torch.equal(po, io) and torch.equal(pl, il)
    assert torch.equal(po, out) and torch.equal(pl, lse)


@pytest.mark.parametrize("si,Tq,tk", [(0, 17, TK), (1, 40, TK), (2, 17, TK), (0, 40, TK2)])
def test_wrappers(si, Tq, tk):
    q, kn, vn, pools, lens, sc, (out, lse), _ = data(si, Tq, tk)
    B, _, H, hd = q.shape
    Hkv = kn.shape[2]
    kv_len = i32(lens)
    # (d) the wrappers return the ops' bits, both cache forms
    assert torch.equal(decode_attention(q, kn, vn, kv_len=kv_len, per_row=True), out)
    assert torch.equal(kv_cache_attend(q, (kn, vn), kv_len=kv_len, per_row=True), out)
    for page in PAGES:
        layer = PagedKV(*pools[page]["perm"], page, tk)
        assert torch.equal(kv_cache_attend(q, layer, kv_len=kv_len, per_row=True), out)
        assert torch.equal(decode_attention(q, layer, kv_len=kv_len, per_row=True), out)
    # q as the q heads of a packed qkv buffer (strided)
    x4 = torch.zeros(B, Tq, H + 2 * Hkv, hd, device=DEV, dtype=BF)
    x4[:, :, :H] = q
    assert torch.equal(kv_cache_attend(x4[:, :, :H], (kn, vn), kv_len=kv_len, per_row=True), out)
    # one entry for all (per_row=False) against per_row with equal lengths
    n = min(lens)
    one = _ext.ops().attn_extend(q, kn, vn, sc, i32([n]), False)
    each = _ext.ops().attn_extend(q, kn, vn, sc, i32([n] * B), True)
    assert torch.isfinite(one[0]).all()
    assert torch.equal(one[0], each[0]) and torch.equal(one[1], each[1])
    kp, vp, bt = pools[16]["perm"]
    pone = _ext.ops().attn_extend_paged(q, kp, vp, bt, sc, tk, i32([n]), False)
    assert torch.equal(pone[0], one[0]) and torch.equal(pone[1], one[1])
    assert torch.equal(kv_cache_attend(q, (kn, vn), kv_len=i32([n])), one[0])


@pytest.mark.parametrize("si,Tq,tk", CASES)
def test_agrees_with_decode_kernel(si, Tq, tk):
    """(e) groups of 16 / G tokens through attn_decode at the matching kv_len: the decode result meets (b)
    itself, and the difference extend - decode, per 32-row tile and relative to the reference tile as in
    (b), stays within the bound of (b): RMS 2.13 and max-abs 4.0 times the yardstick's own error."""
    q, kn, vn, pools, lens, sc, (out, lse), orc = data(si, Tq, tk)
    G = q.shape[2] // kn.shape[2]
    tg = 16 // G
    dec = torch.empty_like(out)
    dlse = torch.empty_like(lse)
    for t0 in range(0, Tq, tg):
        t1 = min(t0 + tg, Tq)
        o, l = _ext.ops().attn_decode(q[:, t0:t1], kn, vn, sc, True, 0, i32([n - (Tq - t1) for n in lens]), True)
        dec[:, t0:t1] = o
        dlse[:, :, t0:t1] = l
    assert torch.isfinite(dec).all()
    failed = check_bounds(f"s{si} Tq{Tq} Tk{tk} decode", dec, dlse, orc)
    assert not failed, failed
    for b, (o64, _, yard, _) in enumerate(orc):
        er, em = A.tile_errors(o64 + (out[b:b + 1].double() - dec[b:b + 1].double()), o64)
        yr, ym = A.yard_errors(yard, o64)
        print(f"s{si} Tq{Tq} b{b}: extend - decode rms ratio {float((er / yr).max()):.2f} "
              f"maxabs ratio {float((em / ym).max()):.2f}")
        assert bool((er <= A.RMS_MARGIN * yr).all()) and bool((em <= A.MAX_MARGIN * ym).all()), b


@pytest.mark.parametrize("si,Tq,tk", [(0, 40, TK), (1, 17, TK), (2, 40, TK), (0, 40, TK2)])
def test_bound_sees_a_length_off_by_one(si, Tq, tk):
    """(g) the oracle run on lengths one too short (where that still holds the query tokens) must fail (b)."""
    q, kn, vn, pools, lens, sc, (out, lse), _ = data(si, Tq, tk)
    short = [oracle(q[b:b + 1], kn[b:b + 1], vn[b:b + 1], n - 1, sc) for b, n in enumerate(lens) if n - 1 >= Tq]
    keep = [b for b, n in enumerate(lens) if n - 1 >= Tq]
    failed = check_bounds(f"s{si} Tq{Tq} short", out[keep], lse[keep], short)
    print("failed:", [b for b, _ in failed])
    assert failed


def test_bad_calls_raise_and_write_nothing():
    q, kn, vn, pools, lens, sc, _, _ = data(0, 17)
    kp, vp, bt = pools[16]["perm"]
    ops = _ext.ops()
    B = q.shape[0]
    kv_len = i32(lens)
    keep = [t.clone() for t in (q, kn, vn, kp, vp)]
    with pytest.raises(RuntimeError):                               # one length for a batch of 3
        ops.attn_extend(q, kn, vn, sc, i32([300]), True)
    with pytest.raises(RuntimeError):
        ops.attn_extend_paged(q, kp, vp, bt, sc, TK, i32([300, 300]), True)
    with pytest.raises(RuntimeError):                               # int64 lengths
        ops.attn_extend(q, kn, vn, sc, kv_len.long(), True)
    for t in (bt.long(), bt.cpu(), bt[:B - 1].contiguous()):        # int64, on the host, a sequence short
        with pytest.raises(RuntimeError):
            ops.attn_extend_paged(q, kp, vp, t, sc, TK, kv_len, True)
    q96, k96 = q[..., :96].contiguous(), kn[..., :96].contiguous()  # head dim 96
    with pytest.raises(RuntimeError):
        ops.attn_extend(q96, k96, k96, sc, kv_len, True)
    with pytest.raises(RuntimeError):
        ops.attn_extend_paged(q96, kp[..., :96].contiguous(), kp[..., :96].contiguous(), bt, sc, TK, kv_len, True)
    with pytest.raises(RuntimeError):                               # Tq > Tk
        ops.attn_extend(q, kn[:, :16], vn[:, :16], sc, kv_len, True)
    with pytest.raises(RuntimeError):
        ops.attn_extend_paged(q, kp, vp, bt, sc, 16, kv_len, True)
    with pytest.raises(RuntimeError):                               # Tk past the table's rows
        ops.attn_extend_paged(q, kp, vp, bt, sc, bt.shape[1] * 16 + 1, kv_len, True)
    # the wrappers: what the extend kernel does not take keeps raising ValueError
    with pytest.raises(ValueError):
        decode_attention(q96, k96, k96, kv_len=kv_len, per_row=True)
    with pytest.raises(ValueError):
        decode_attention(q.float(), kn.float(), vn.float(), kv_len=kv_len, per_row=True)
    with pytest.raises(ValueError):
        decode_attention(q, kn, vn, causal=False, kv_len=kv_len, per_row=True)
    torch.cuda.synchronize()
    for t, t0 in zip((q, kn, vn, kp, vp), keep):
        assert torch.equal(t.view(torch.int16), t0.view(torch.int16))
