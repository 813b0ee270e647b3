"""Paged KV cache on the GPU: attn_decode_paged through shuffled block tables bitwise against
attn_decode on the gathered rows (NaN in every pool row that must not be read), rope_kv_write_paged_
bitwise against rope_kv_write_, bad calls, and LLaMA3 / Gemma decoding from a pool smaller than the
contiguous cache (eager ragged steps, GraphDecoder replays, free + prefill_row mid-stream, CacheFull,
inactive rows) bitwise against the contiguous-cache run of the same path."""
import functools
import math

import pytest
import torch

from solvingpapers_amd.infer import CacheFull, GraphDecoder, RaggedDecodeState
from solvingpapers_amd.ops import _ext, reference as R
from solvingpapers_amd.ops.attention import PagedKV, decode_attention, kv_cache_attend, rope_kv_cache_write_
from solvingpapers_amd.ops.rope import RopeCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
TK = 300   # logical row bound, as tests/test_ragged_decode_gpu.py: a load batch covers 64 / 128 / 32 keys at
           # hd 128 / 64 / 256, so a 64-row page is one batch, half a batch or two, and a 16-row page puts
           # several pages inside every batch; the lengths straddle the batch and page boundaries


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def i32(x):
    return torch.tensor(x, device=DEV, dtype=torch.int32)


# ------------------------------------------------------------------ decode attention through the table
SHAPES = [
    # B, H, Hkv, hd, lens
    (4, 8, 2, 128, (1, 64, 65, 300)),
    (3, 16, 1, 64, (5, 129, 300)),
    (2, 16, 1, 256, (33, 300)),
]
ATTN_CASES = [(s, 1) for s in range(3)] + [(0, 3)]   # Tq = 3 fits 16 rows per block on the GQA shape only


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


@functools.lru_cache(maxsize=None)
def attn_data(si, Tq, page):
    """q, the contiguous cache, an identity-table pool and a shuffled-table pool of the same rows, the
    lengths and the oracle's per-sequence (out, lse): built once per (shape, Tq, page)."""
    B, H, Hkv, hd, lens = SHAPES[si]
    lens = tuple(max(n, Tq) for n in lens)
    g = torch.Generator(device=DEV).manual_seed(100 * si + Tq)
    q = torch.randn(B, Tq, H, hd, device=DEV, generator=g).to(BF)
    k, v = kv_rows((B, TK, Hkv, hd), -3, 0, g), kv_rows((B, TK, Hkv, hd), -6, 6, g)
    NP = -(-TK // page)
    used = [-(-n // page) for n in lens]
    P = 2 * sum(used) + 1
    ident, perm = torch.zeros(B, NP, dtype=torch.int64), torch.zeros(B, NP, dtype=torch.int64)
    order = (torch.randperm(P - 1, generator=torch.Generator().manual_seed(si + page)) + 1).tolist()
    nxt = 1
    for b, u in enumerate(used):        # entries past a sequence's pages stay 0: never read
        ident[b, :u] = torch.arange(nxt, nxt + u)
        perm[b, :u] = torch.tensor(order[nxt - 1:nxt - 1 + u])
        nxt += u
    pools = {"ident": build_pools(k, v, lens, page, ident), "perm": build_pools(k, v, lens, page, perm)}
    sc = 1 / math.sqrt(hd)
    ref = [R.attention(q[b:b + 1].float(), k[b:b + 1, :n].float(), v[b:b + 1, :n].float(), True, sc)
           for b, n in enumerate(lens)]
    return q, k, v, pools, lens, sc, ref


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("ns", [0, 1, 7])
@pytest.mark.parametrize("si,Tq", ATTN_CASES)
def test_attn_decode_paged(si, Tq, ns, page):
    q, k, v, pools, lens, sc, ref = attn_data(si, Tq, page)
    op = _ext.ops().attn_decode_paged
    kp, vp, bt = pools["perm"]
    out, lse = op(q, kp, vp, bt, sc, True, ns, TK, i32(lens), True)
    # no NaN: no row at or past a sequence's length, no unused page and no null-page row was read
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    # (a) the identity table and the shuffled one: same bits
    ki, vi, bi = pools["ident"]
    oi, li = op(q, ki, vi, bi, sc, True, ns, TK, i32(lens), True)
    assert torch.equal(out, oi) and torch.equal(lse, li)
    # (b) attn_decode on the contiguous cache with the same kv_len / per_row / nsplit: same bits
    oc, lc = _ext.ops().attn_decode(q, k, v, sc, True, ns, i32(lens), True)
    assert torch.equal(out, oc) and torch.equal(lse, lc)
    # (c) the oracle, per sequence
    for b, n in enumerate(lens):
        e, dl = rel(out[b:b + 1], ref[b][0]), (lse[b:b + 1] - ref[b][1]).abs().max().item()
        print(f"page {page} b {b} len {n}: rel L2 {e:.3e}  max |dlse| {dl:.3e}")
        assert e < 1e-2 and dl < 1e-2, (b, n, e, dl)
    # (d) the wrappers return the op's bits
    layer = PagedKV(kp, vp, bt, page, TK)
    assert torch.equal(kv_cache_attend(q, layer, nsplit=ns, kv_len=i32(lens), per_row=True), out)
    assert torch.equal(decode_attention(q, layer, nsplit=ns, kv_len=i32(lens), per_row=True), out)


@pytest.mark.parametrize("page", [16, 64])
@pytest.mark.parametrize("si,Tq", ATTN_CASES)
def test_attn_decode_paged_host_length(si, Tq, page):
    """(e) kv_len=None (the eager step's host Tk) against the device kv_len forms, uniform length."""
    B, H, Hkv, hd, _ = SHAPES[si]
    n = 129
    g = torch.Generator(device=DEV).manual_seed(si + Tq)
    q = torch.randn(B, Tq, H, hd, device=DEV, generator=g).to(BF)
    k, v = kv_rows((B, TK, Hkv, hd), -3, 0, g), kv_rows((B, TK, Hkv, hd), -6, 6, g)
    NP, u = -(-TK // page), -(-n // page)
    table = torch.zeros(B, NP, dtype=torch.int64)
    order = torch.randperm(2 * B * u, generator=torch.Generator().manual_seed(page)) + 1
    for b in range(B):
        table[b, :u] = order[b * u:(b + 1) * u]
    kp, vp, bt = build_pools(k, v, (n,) * B, page, table)
    op = _ext.ops().attn_decode_paged
    sc = 1 / math.sqrt(hd)
    for ns in (0, 3):
        out, lse = op(q, kp, vp, bt, sc, True, ns, n, None, False)
        assert torch.isfinite(out).all() and torch.isfinite(lse).all()
        for kv_len, per_row in ((i32([n]), False), (i32([n] * B), True)):
            o2, l2 = op(q, kp, vp, bt, sc, True, ns, n, kv_len, per_row)
            assert torch.equal(out, o2) and torch.equal(lse, l2)
        oc, lc = _ext.ops().attn_decode(q, k[:, :n], v[:, :n], sc, True, ns)
        assert torch.equal(out, oc) and torch.equal(lse, lc)
        assert torch.equal(kv_cache_attend(q, PagedKV(kp, vp, bt, page), n, nsplit=ns), out)


def test_attend_falls_back_to_gather():
    """More than 16 rows per block (a prompt chunk at a later position): rows gathered, flash kernel."""
    q, k, v, pools, lens, sc, _ = attn_data(1, 1, 16)
    kp, vp, bt = pools["perm"]
    n = min(lens)
    q5 = torch.randn(q.shape[0], 5, q.shape[2], q.shape[3], device=DEV).to(BF)     # 5 x 16 rows per kv head
    got = kv_cache_attend(q5, PagedKV(kp, vp, bt, 16), n)
    want = decode_attention(q5, k[:, :n].contiguous(), v[:, :n].contiguous())
    assert torch.equal(got, want)


# ------------------------------------------------------------------ RoPE + cache write through the table
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("mode", [0, 1])
def test_rope_kv_write_paged_bitwise(mode, hd):
    B, T, H, Hkv, Tmax, page = 4, 1, 4, 2, 48, 16
    rows = (0, 17, 47, 48)             # sequence 2: past its reservation (null page); 3: past the table (dropped)
    reserved = (16, 32, 32, 48)
    g = torch.Generator(device=DEV).manual_seed(10 * mode + hd)
    x = torch.randn(B, T, H + 2 * Hkv, hd, device=DEV, generator=g).to(BF)
    x[:, :, H + Hkv:] = kv_rows((B, T, Hkv, hd), -6, 6, g)
    cos, sin = RopeCache.get(Tmax, hd, 500000.0, DEV)
    index = torch.tensor(rows, device=DEV)
    pos = index.clamp_max(Tmax - 1).int()[:, None].contiguous()
    P = 2 * 8 + 1
    order = (torch.randperm(P - 1, generator=torch.Generator().manual_seed(hd + mode)) + 1).tolist()
    table = torch.zeros(B, Tmax // page, dtype=torch.int64)
    nxt = 0
    for b, n in enumerate(reserved):
        table[b, :n // page] = torch.tensor(order[nxt:nxt + n // page])
        nxt += n // page
    bt = table.to(DEV, torch.int32)
    kp = kv_rows((P, page, Hkv, hd), -3, 3, g)
    vp = kv_rows((P, page, Hkv, hd), -3, 3, g)
    layer = PagedKV(kp, vp, bt, page)
    kc, vc = layer.gathered(Tmax)       # the contiguous cache with the same contents
    k0, v0 = kp.clone(), vp.clone()
    xa, xb = x.clone(), x.clone()
    rope_kv_cache_write_(layer, xa, cos, sin, pos, index, H, Hkv, mode, per_row=True)
    rope_kv_cache_write_((kc, vc), xb, cos, sin, pos, index, H, Hkv, mode, per_row=True)
    assert torch.equal(xa, xb)          # q rotated in place, bitwise the contiguous op's
    gk, gv = layer.gathered(Tmax)
    for b, n in enumerate(reserved):    # every reserved row holds the contiguous cache's bits
        assert torch.equal(gk[b, :n], kc[b, :n]) and torch.equal(gv[b, :n], vc[b, :n]), b
    written = [int(R.paged_rows(bt[b:b + 1], torch.tensor([r], device=DEV), page)) for b, r in ((0, 0), (1, 17))]
    keep = torch.ones(P * page, dtype=torch.bool, device=DEV)
    keep[written] = False
    keep[:page] = False                 # the null page took sequence 2's row
    for pool, p0 in ((kp, k0), (vp, v0)):
        flat, f0 = pool.view(-1, Hkv, hd), p0.view(-1, Hkv, hd)
        assert torch.equal(flat[keep], f0[keep])
        assert not torch.equal(flat[written], f0[written])
        assert torch.equal(flat[1:15], f0[1:15]) and not torch.equal(flat[15], f0[15])   # row 47 -> page 0, row 15
    # the scalar-index form against the contiguous op
    one = torch.tensor([5], device=DEV)
    rope_kv_cache_write_(layer, xa, cos, sin, pos, one, H, Hkv, mode)
    rope_kv_cache_write_((kc, vc), xb, cos, sin, pos, one, H, Hkv, mode)
    assert torch.equal(xa, xb)
    assert torch.equal(layer.gathered(16)[0], kc[:, :16]) and torch.equal(layer.gathered(16)[1], vc[:, :16])


# ------------------------------------------------------------------ bad calls
def test_bad_calls_raise_and_write_nothing():
    q, k, v, pools, lens, sc, _ = attn_data(0, 1, 16)
    kp, vp, bt = pools["perm"]
    ops = _ext.ops()
    B, NP = bt.shape
    kv_len = i32(lens)
    bad_tables = (bt.long(),                                        # int64
                  bt.cpu(),                                         # on the host
                  bt[:B - 1].contiguous(),                          # a sequence short
                  bt.reshape(-1),                                   # 1-D
                  bt.t().contiguous().t())                          # not contiguous
    for t in bad_tables:
        with pytest.raises(RuntimeError):
            ops.attn_decode_paged(q, kp, vp, t, sc, True, 0, TK, kv_len, True)
    odd = kp.view(-1, *kp.shape[2:])[:4 * 24].view(4, 24, *kp.shape[2:])           # page_size 24
    with pytest.raises(RuntimeError):
        ops.attn_decode_paged(q, odd, odd, bt, sc, True, 0, 24, kv_len, True)
    with pytest.raises(RuntimeError):                               # Tk past the table's NP * page_size rows
        ops.attn_decode_paged(q, kp, vp, bt, sc, True, 0, NP * 16 + 1, kv_len, True)
    with pytest.raises(RuntimeError):                               # per_row without lengths
        ops.attn_decode_paged(q, kp, vp, bt, sc, True, 0, TK, None, True)
    with pytest.raises(RuntimeError):                               # one length for a batch of 4
        ops.attn_decode_paged(q, kp, vp, bt, sc, True, 0, TK, i32([300]), True)
    with pytest.raises(ValueError):
        kv_cache_attend(q, PagedKV(kp, vp, bt, 16), per_row=True)

    H, Hkv, hd, page = 4, 2, 64, 16
    x = torch.randn(B, 1, H + 2 * Hkv, hd, device=DEV).to(BF)
    x0 = x.clone()
    cos, sin = RopeCache.get(NP * page, hd, 500000.0, DEV)
    pos = torch.zeros(B, 1, device=DEV, dtype=torch.int32)
    index = torch.zeros(B, device=DEV, dtype=torch.long)
    wk = torch.zeros(8, page, Hkv, hd, device=DEV, dtype=BF)
    wv = torch.zeros(8, page, Hkv, hd, device=DEV, dtype=BF)
    wt = torch.ones(B, NP, device=DEV, dtype=torch.int32)
    for t in (wt.long(), wt.cpu(), wt[:B - 1].contiguous(), wt.reshape(-1), wt.t().contiguous().t()):
        with pytest.raises(RuntimeError):
            ops.rope_kv_write_paged_(x, cos, sin, pos, index, wk, wv, t, H, Hkv, 0, True)
    w24 = torch.zeros(8, 24, Hkv, hd, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError):
        ops.rope_kv_write_paged_(x, cos, sin, pos, index, w24, w24, wt, H, Hkv, 0, True)
    with pytest.raises(RuntimeError):                               # one index for a batch of 4
        ops.rope_kv_write_paged_(x, cos, sin, pos, index[:1], wk, wv, wt, H, Hkv, 0, True)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and (wk == 0).all() and (wv == 0).all() and (w24 == 0).all()


# ------------------------------------------------------------------ models
LENS = (5, 17, 24)
STEPS, CACHE = 8, 40
PAGED = dict(page_size=16, num_pages=6)    # 1 + 2 + 2 pages and the null page; the contiguous cache: 9 pages' worth


@functools.lru_cache(maxsize=None)
def model_data(name):
    """The bf16 model, three sequences of len_b + STEPS tokens, the right-padded prompt batch and each
    sequence's own full forward: built once."""
    if name == "llama3_tiny":
        from solvingpapers_amd.models import llama3
        m = llama3.Llama3(llama3.config(name), device=DEV, dtype=BF, seed=0).eval()
    else:
        from solvingpapers_amd.models import gemma
        m = gemma.Gemma(gemma.config(name), device=DEV, dtype=BF, seed=0).eval()
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, m.c.vocab_size, (n + STEPS,), generator=g).to(DEV) for n in LENS]
    ids = torch.full((len(LENS), max(LENS)), 3, dtype=torch.long, device=DEV)   # right-padded with token 3
    for b, n in enumerate(LENS):
        ids[b, :n] = seqs[b][:n]
    with torch.no_grad():
        full = [m(s[None]).float()[0] for s in seqs]
    return m, seqs, ids, full


def step_tokens(seqs, i):
    return torch.stack([s[n + i] for s, n in zip(seqs, LENS)])[:, None]


def check_against_full(name, path, lg0, lgs, full):
    for b, n in enumerate(LENS):
        e0 = rel(lg0[b], full[b][n - 1])
        es = [rel(lg[b], full[b][n + i]) for i, lg in enumerate(lgs)]
        print(f"{name} {path} row {b} (len {n}): prefill rel {e0:.3e}, steps max rel {max(es):.3e}")
        assert e0 < 2e-2, (b, e0)
        assert max(es) < 2e-2, (b, es)


@torch.no_grad()
def run_eager(name, **paged):
    m, seqs, ids, _ = model_data(name)
    lens = torch.tensor(LENS, device=DEV)
    cache = m.new_cache(len(LENS), CACHE, **paged)
    if paged:
        for b, n in enumerate(LENS):
            cache.reserve(b, n + STEPS)
        assert cache.pages_used == 5 and cache.pages_free == 0
    lg0 = m.step(ids, cache, 0, last=lens - 1)
    state = RaggedDecodeState(len(LENS), CACHE, DEV)
    state.set(lens)
    lgs = []
    for i in range(STEPS):
        lgs.append(m.step_graph(step_tokens(seqs, i), cache, state))
        state.advance()
    return lg0, lgs


@torch.no_grad()
def run_graph(name, steps=STEPS, **paged):
    m, seqs, ids, _ = model_data(name)
    dec = GraphDecoder(m, len(LENS), CACHE, ragged=True, **paged)
    lg0 = dec.prefill(ids, LENS)
    if paged:
        for b, n in enumerate(LENS):      # whatever the replays will write, before them
            dec.reserve(b, n + STEPS)
    lgs = []
    for i in range(steps):
        dec.ids.copy_(step_tokens(seqs, i))
        dec.graph.replay()
        lgs.append(dec.logits.clone())
    return dec, lg0, lgs


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_model_eager_ragged_steps(name):
    full = model_data(name)[3]
    lg0, lgs = run_eager(name, **PAGED)
    c0, cs = run_eager(name)
    assert torch.equal(lg0, c0) and all(torch.equal(a, b) for a, b in zip(lgs, cs))
    check_against_full(name, "eager paged", lg0, lgs, full)


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_graph_decoder_ragged_replays(name):
    full = model_data(name)[3]
    dec, lg0, lgs = run_graph(name, **PAGED)
    _, c0, cs = run_graph(name)
    assert torch.equal(lg0, c0) and all(torch.equal(a, b) for a, b in zip(lgs, cs))
    check_against_full(name, "graph paged", lg0, lgs, full)
    assert dec.cache.pages_used == 5 and dec.cache.nbytes() < model_data(name)[0].new_cache(3, CACHE).nbytes()


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
@torch.no_grad()
def test_free_and_prefill_row_mid_stream(name):
    m, seqs, ids, full = model_data(name)
    dec, _, _ = run_graph(name, steps=4, **PAGED)
    ctl, _, _ = run_graph(name, steps=4, **PAGED)       # the control: same stream, no prefill_row
    assert dec.cache.pages_used == 5
    g = torch.Generator().manual_seed(7)
    new = torch.randint(0, m.c.vocab_size, (9 + 2,), generator=g).to(DEV)
    full_new = m(new[None]).float()[0]
    dec.free(1)
    assert dec.cache.pages_used == 3 and dec.cache.pages_free == 2
    lg_row = dec.prefill_row(1, new[:9], reserve=11)
    assert dec.cache.pages_used == 4 and dec.cache.held(1) == 1     # 11 rows: one 16-row page
    assert rel(lg_row, full_new[8]) < 2e-2, rel(lg_row, full_new[8])
    assert dec.state.index.tolist() == [LENS[0] + 4, 9, LENS[2] + 4]
    for i in range(2):                                  # slot 1 continues the new prompt, 0 and 2 their own
        tok = step_tokens(seqs, 4 + i)
        ctl.ids.copy_(tok)
        ctl.graph.replay()
        tok[1, 0] = new[9 + i]
        dec.ids.copy_(tok)
        dec.graph.replay()
        e = rel(dec.logits[1], full_new[9 + i])
        print(f"{name} slot 1 after prefill_row, step {i}: rel {e:.3e}")
        assert e < 2e-2, e
        for b in (0, 2):                                # untouched slots: the same bits as the control
            assert torch.equal(dec.logits[b], ctl.logits[b]), (i, b)
            assert rel(dec.logits[b], full[b][LENS[b] + 4 + i]) < 2e-2
    with pytest.raises(CacheFull):                      # 3 pages for slot 1: it holds 1 and 1 is free
        dec.prefill_row(1, new[:9], reserve=40)
    assert dec.cache.pages_used == 4 and dec.cache.held(1) == 1 and dec.state.index[1].item() == 11


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
@torch.no_grad()
def test_graph_decoder_uniform(name):
    m, seqs, _, _ = model_data(name)
    x = torch.stack([seqs[2], seqs[2].flip(0)])

    def run(**paged):
        dec = GraphDecoder(m, 2, CACHE, **paged)
        out = [dec.prefill(x[:, :24])]
        if paged:
            for b in range(2):
                dec.reserve(b, 24 + STEPS)
        for i in range(STEPS):
            dec.ids.copy_(x[:, 24 + i:25 + i])
            dec.graph.replay()
            out.append(dec.logits.clone())
        return torch.stack(out)

    assert torch.equal(run(page_size=16), run())


@torch.no_grad()
def test_generate_cache_full_leaves_the_decoder_alone():
    m, seqs, ids, _ = model_data("llama3_tiny")
    # 12 new tokens: rows (17, 29, 36) need 2 + 2 + 3 pages; 6 and the null page are one short, while the
    # prompts alone (1 + 2 + 2) fit
    dec = GraphDecoder(m, len(LENS), CACHE, ragged=True, page_size=16, num_pages=7)
    dec.prefill(ids, LENS)
    idx, kvl, table = dec.state.index.clone(), dec.state.kv_len.clone(), dec.cache.table.clone()
    with pytest.raises(CacheFull):
        dec.generate(ids, 12, prompt_lens=LENS)
    assert torch.equal(dec.state.index, idx) and torch.equal(dec.state.kv_len, kvl)
    assert torch.equal(dec.cache.table, table) and torch.equal(dec.cache.block_table.cpu(), table)
    assert dec.cache.pages_used == 5
    dec.graph.replay()                                  # still a working decoder: one replay, one position
    assert dec.state.index.tolist() == (idx + 1).tolist() and torch.isfinite(dec.logits).all()
    ok = GraphDecoder(m, len(LENS), CACHE, ragged=True, page_size=16, num_pages=8)
    out = ok.generate(ids, 12, prompt_lens=LENS, pad_token_id=1000)
    assert ok.cache.pages_used == 7
    ref = GraphDecoder(m, len(LENS), CACHE, ragged=True).generate(ids, 12, prompt_lens=LENS, pad_token_id=1000)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
@torch.no_grad()
def test_inactive_row_stays_put(name):
    seqs = model_data(name)[1]
    dec, _, _ = run_graph(name, steps=1, **PAGED)
    dec.state.active[1] = 0
    idx0 = dec.state.index.tolist()
    before = [(l.k.clone(), l.v.clone()) for l in dec.cache]
    for i in range(3):
        dec.ids.copy_(step_tokens(seqs, 1 + i))
        dec.graph.replay()
        assert torch.isfinite(dec.logits).all()
    assert dec.state.index.tolist() == [idx0[0] + 3, idx0[1], idx0[2] + 3]
    # written: the parked row's own row idx0[1], over and over; rows idx0[b] .. idx0[b] + 2 of the two
    # active sequences. Every other pool row outside the null page holds the bits it held.
    wrote = [(1, idx0[1])] + [(b, idx0[b] + i) for b in (0, 2) for i in range(3)]
    keep = torch.ones(dec.cache.num_pages * 16, dtype=torch.bool, device=DEV)
    keep[:16] = False
    for b, r in wrote:
        keep[int(R.paged_rows(dec.cache.block_table[b:b + 1], torch.tensor([r], device=DEV), 16))] = False
    for l, (k0, v0) in zip(dec.cache, before):
        assert torch.equal(l.k.flatten(0, 1)[keep], k0.flatten(0, 1)[keep])
        assert torch.equal(l.v.flatten(0, 1)[keep], v0.flatten(0, 1)[keep])
    ctl, _, _ = run_graph(name, steps=4, **PAGED)       # rows 0 and 2 after the same 4 steps, row 1 active
    for l, c in zip(dec.cache, ctl.cache):
        for b in (0, 2):
            n = LENS[b] + 4
            for pl, pc in ((l.k, c.k), (l.v, c.v)):
                assert torch.equal(R.paged_gather(pl, dec.cache.block_table, n)[b],
                                   R.paged_gather(pc, ctl.cache.block_table, n)[b])
