"""Paged KV cache on the CPU: the host allocator (free list, host mirror, null page), the layout
(reference.paged_gather after the cache writers against the contiguous cache after the same writes,
bitwise), LLaMA3 / Gemma generating and teacher-forced decoding from pages against the contiguous
cache (the CPU route is gather + the same oracle: the same floating-point operations, so equal bits),
pool sizing and the refusals."""
import pytest
import torch

from solvingpapers_amd.infer import CacheFull, PagedKVCache, RaggedDecodeState, generate
from solvingpapers_amd.infer.graph import DecodeState
from solvingpapers_amd.ops import reference as R
from solvingpapers_amd.ops.attention import (PagedKV, decode_attention, kv_cache_attend, kv_cache_write,
                                             rope_kv_cache_write_)

LENS = (5, 17, 24)
STEPS, CACHE, PAGE = 8, 40, 16


def make(batch=3, max_len=CACHE, num_pages=None, layers=2, page=PAGE, dtype=torch.float32):
    return PagedKVCache(layers, batch, max_len, 2, 8, page_size=page, num_pages=num_pages, dtype=dtype)


# ------------------------------------------------------------------ allocator
def test_allocator_null_page_and_idempotent_reserve():
    c = make()
    assert c.pages_per_seq == 3 and c.num_pages == 3 * 3 + 1 and c.pages_free == 9 and c.pages_used == 0
    assert all(l.block_table is c.block_table for l in c)           # one table for every layer
    assert c.block_table.dtype == torch.int32 and c.block_table.shape == (3, 3) and (c.block_table == 0).all()
    c.reserve(0, 17)
    row = c.table[0].tolist()
    assert row[2] == 0 and 0 not in row[:2] and c.pages_used == 2
    c.reserve(0, 17)
    c.reserve(0, 5)                                                # never shrinks, never reshuffles
    assert c.table[0].tolist() == row and c.pages_used == 2
    c.reserve(0, 33)                                               # grows: the first two pages stay
    assert c.table[0].tolist()[:2] == row[:2] and c.table[0, 2] != 0 and c.pages_used == 3
    for b in (1, 2):
        c.reserve(b, CACHE)
    handed = c.table.flatten().tolist()
    assert sorted(handed) == list(range(1, 10))                     # every page but 0, each once
    assert torch.equal(c.block_table.cpu(), c.table)
    with pytest.raises(ValueError):
        c.reserve(0, 49)                                           # past the table's NP * page_size rows


def test_cache_full_changes_nothing_and_free_reuses():
    c = make(num_pages=5)
    c.reserve(0, 32)
    c.reserve(1, 16)
    table, free = c.table.clone(), list(c._free)
    with pytest.raises(CacheFull) as e:
        c.reserve(2, 17)                                           # needs 2, 1 free
    assert isinstance(e.value, RuntimeError)
    assert torch.equal(c.table, table) and c._free == free and torch.equal(c.block_table.cpu(), table)
    assert c.pages_free == 1 and c.pages_used == 3
    mine = c.table[0, :2].tolist()
    c.free(0)
    assert c.table[0].tolist() == [0, 0, 0] and c.pages_free == 3 and set(mine) <= set(c._free)
    assert torch.equal(c.block_table.cpu(), c.table) and c.table[1].tolist() == table[1].tolist()
    c.reserve(2, 17)
    assert c.table[2, :2].tolist() == mine                         # the freed pages, reused
    c.free_all()
    assert c.pages_used == 0 and (c.block_table == 0).all() and sorted(c._free) == [1, 2, 3, 4]
    assert c.nbytes() == 2 * 2 * 5 * PAGE * 2 * 8 * 4 + 3 * 3 * 4


def test_rows_shares_pools_and_allocator():
    c = make()
    sub = c.rows(1, 2)
    assert isinstance(sub, PagedKVCache) and len(sub) == len(c) and sub.batch == 1
    for l, s in zip(c, sub):
        assert s.k.data_ptr() == l.k.data_ptr() and s.v.data_ptr() == l.v.data_ptr()
        assert s.block_table.data_ptr() == c.block_table[1:2].data_ptr() and s.block_table.is_contiguous()
    sub.reserve(0, 20)                                             # slot 0 of the view is slot 1 here
    assert c.held(1) == 2 and c.pages_used == 2 and torch.equal(sub.block_table, c.block_table[1:2])
    k = torch.randn(1, 20, 2, 8)
    kv_cache_write(sub[0], k, -k, 0)
    assert torch.equal(R.paged_gather(c[0].k, c.block_table, 20)[1], k[0])
    with pytest.raises(IndexError):
        c.rows(2, 4)


# ------------------------------------------------------------------ layout
def test_paged_rows_and_gather_define_the_layout():
    bt = torch.tensor([[3, 1, 0], [2, 0, 0]], dtype=torch.int32)
    rows = R.paged_rows(bt, torch.tensor([0, 15, 16, 31, 32]), 16)
    assert rows.tolist() == [[48, 63, 16, 31, 0], [32, 47, 0, 15, 0]]
    assert R.paged_rows(bt, torch.tensor([[17], [1]]), 16).tolist() == [[17], [33]]
    pool = torch.arange(4 * 16, dtype=torch.float32)[:, None, None].expand(-1, 2, 4).reshape(4, 16, 2, 4).contiguous()
    got = R.paged_gather(pool, bt, 20)
    assert got.shape == (2, 20, 2, 4)
    assert got[0, :, 0, 0].tolist() == list(range(48, 64)) + list(range(16, 20))
    with pytest.raises(IndexError):
        R.paged_rows(bt, torch.tensor([48]), 16)
    with pytest.raises(ValueError):
        R.paged_rows(bt, torch.tensor([0]), 24)


def test_kv_cache_write_matches_contiguous():
    g = torch.Generator().manual_seed(0)
    c = make(num_pages=6)
    for b, n in enumerate(LENS):
        c.reserve(b, n)                                            # 1 + 2 + 2 pages
    kc, vc = torch.zeros(3, CACHE, 2, 8), torch.zeros(3, CACHE, 2, 8)
    k, v = torch.randn(3, 24, 2, 8, generator=g), torch.randn(3, 24, 2, 8, generator=g)
    kv_cache_write(c[1], k, v, 0)                                  # right-padded prefill: 24 rows each
    kv_cache_write((kc, vc), k, v, 0)
    assert (c[0].k == 0).all()                                     # another layer's pools: untouched
    gk, gv = c[1].gathered(CACHE)
    for b, n in enumerate(LENS):                                   # reserved rows hold the contiguous cache's bits
        r = c.held(b) * PAGE
        assert torch.equal(gk[b, :min(r, 24)], kc[b, :min(r, 24)]) and torch.equal(gv[b, :min(r, 24)], vc[b, :min(r, 24)])
    # sequence 0 reserved 16 rows: its pad rows 16..23 went to the null page and cost nothing
    assert c.pages_used == 5 and not (c[1].k[0] == 0).all()
    k1, v1 = torch.randn(3, 1, 2, 8, generator=g), torch.randn(3, 1, 2, 8, generator=g)
    kv_cache_write(c[1], k1, v1, 7)
    kv_cache_write((kc, vc), k1, v1, 7)
    assert torch.equal(c[1].gathered(8)[0], kc[:, :8]) and torch.equal(c[1].gathered(8)[1], vc[:, :8])
    with pytest.raises(ValueError):
        kv_cache_write(c[1], k, v, 30)                             # rows [30, 54) past the table's 48


@pytest.mark.parametrize("mode", [0, 1])
def test_rope_kv_cache_write_matches_contiguous(mode):
    B, H, Hkv, hd, Tmax = 4, 4, 2, 16, 48
    g = torch.Generator().manual_seed(mode)
    c = PagedKVCache(1, B, Tmax, Hkv, hd, page_size=PAGE, dtype=torch.float32)
    for b, n in enumerate((16, 32, 32, 48)):
        c.reserve(b, n)
    for t in (c[0].k, c[0].v):
        t.copy_(torch.randn(t.shape, generator=g))
    kc, vc = c[0].gathered(Tmax)                                   # the contiguous cache with the same contents
    cos, sin = R.rope_tables(Tmax, hd, 500000.0)
    # sequence 2 writes row 47, past its 32-row reservation: the null page; sequence 3 writes row 48,
    # past the table: dropped
    index = torch.tensor([0, 17, 47, 48])
    pos = index.clamp_max(Tmax - 1).int()[:, None]
    x = torch.randn(B, 1, H + 2 * Hkv, hd, generator=g)
    xa, xb = x.clone(), x.clone()
    k0, v0 = c[0].k.clone(), c[0].v.clone()
    rope_kv_cache_write_(c[0], xa, cos, sin, pos, index, H, Hkv, mode, per_row=True)
    rope_kv_cache_write_((kc, vc), xb, cos, sin, pos, index, H, Hkv, mode, per_row=True)
    assert torch.equal(xa, xb)
    gk, gv = c[0].gathered(Tmax)
    for b, n in enumerate((16, 32, 32, 48)):                       # every reserved row, bitwise
        assert torch.equal(gk[b, :n], kc[b, :n]) and torch.equal(gv[b, :n], vc[b, :n]), b
    written = [int(R.paged_rows(c.block_table[b:b + 1], [r], PAGE)) for b, r in ((0, 0), (1, 17))]
    keep = torch.ones(c.num_pages * PAGE, dtype=torch.bool)
    keep[written] = False
    keep[:PAGE] = False                                            # the null page took sequence 2's row
    for pool, p0 in ((c[0].k, k0), (c[0].v, v0)):
        flat, f0 = pool.view(-1, Hkv, hd), p0.view(-1, Hkv, hd)
        assert torch.equal(flat[keep], f0[keep])
        assert not torch.equal(flat[written], f0[written])
        assert not torch.equal(flat[15], f0[15])                   # row 47 & 15 of page 0
    # a row >= NP * page_size alone: every pool byte unchanged
    k1, v1 = c[0].k.clone(), c[0].v.clone()
    far = torch.tensor([48, 49, 1000, -1])
    rope_kv_cache_write_(c[0], x.clone(), cos, sin, pos, far, H, Hkv, mode, per_row=True)
    assert torch.equal(c[0].k, k1) and torch.equal(c[0].v, v1)
    # the scalar-index form
    rope_kv_cache_write_(c[0], xa, cos, sin, pos, torch.tensor([3]), H, Hkv, mode)
    rope_kv_cache_write_((kc, vc), xb, cos, sin, pos, torch.tensor([3]), H, Hkv, mode)
    assert torch.equal(c[0].gathered(16)[0], kc[:, :16]) and torch.equal(c[0].gathered(16)[1], vc[:, :16])


def test_attend_routes_through_the_oracles():
    g = torch.Generator().manual_seed(3)
    c = make(layers=1)
    for b in range(3):
        c.reserve(b, CACHE)
    for t in (c[0].k, c[0].v):
        t.copy_(torch.randn(t.shape, generator=g))
    kc, vc = c[0].gathered(CACHE)
    q = torch.randn(3, 1, 4, 8, generator=g)
    lens = torch.tensor(LENS, dtype=torch.int32)
    want = kv_cache_attend(q, (kc, vc), kv_len=lens, per_row=True)
    assert torch.equal(kv_cache_attend(q, c[0], kv_len=lens, per_row=True), want)
    assert torch.equal(decode_attention(q, c[0], kv_len=lens, per_row=True), want)
    assert torch.equal(R.attention_paged(q, c[0], CACHE, lens, True)[0], want)
    assert torch.equal(kv_cache_attend(q, c[0], 24), kv_cache_attend(q, (kc, vc), 24))
    one = torch.tensor([17], dtype=torch.int32)
    assert torch.equal(kv_cache_attend(q, c[0], kv_len=one), kv_cache_attend(q, (kc, vc), kv_len=one))
    assert torch.equal(kv_cache_attend(q, c[0], 24, fresh=(kc[:, :1], vc[:, :1])),
                       kv_cache_attend(q, (kc[:, :1], vc[:, :1]), 1))
    with pytest.raises(ValueError):
        kv_cache_attend(q, c[0], per_row=True)
    with pytest.raises(ValueError):
        kv_cache_attend(q, c[0], 49)


# ------------------------------------------------------------------ models
def model(name):
    if name == "llama3_tiny":
        from solvingpapers_amd.models import llama3
        return llama3.Llama3(llama3.config(name), seed=0).eval()
    from solvingpapers_amd.models import gemma
    return gemma.Gemma(gemma.config(name), seed=0).eval()


def prompts(m):
    g = torch.Generator().manual_seed(0)
    return torch.randint(0, m.c.vocab_size, (len(LENS), max(LENS)), generator=g)


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_generate_tokens_equal_contiguous(name):
    m = model(name)
    ids = prompts(m)
    assert torch.equal(generate(m, ids, STEPS, greedy=True, page_size=PAGE), generate(m, ids, STEPS, greedy=True))
    want = generate(m, ids, STEPS, greedy=True, prompt_lens=LENS)
    assert torch.equal(generate(m, ids, STEPS, greedy=True, prompt_lens=LENS, page_size=PAGE), want)
    # lens (5, 17, 24) + 8 new tokens at page 16: 1 + 2 + 2 pages and the null page
    assert torch.equal(generate(m, ids, STEPS, greedy=True, prompt_lens=LENS, page_size=PAGE, num_pages=6), want)


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_pool_one_page_short_raises_before_any_step(name):
    m = model(name)
    calls = []
    step = m.step
    m.step = lambda *a, **k: calls.append(1) or step(*a, **k)
    with pytest.raises(CacheFull):
        generate(m, prompts(m), STEPS, greedy=True, prompt_lens=LENS, page_size=PAGE, num_pages=5)
    assert not calls
    with pytest.raises(CacheFull):                                 # uniform: 3 x ceil(32 / 16) = 6 pages + null
        generate(m, prompts(m), STEPS, greedy=True, page_size=PAGE, num_pages=6)
    assert not calls


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
@torch.no_grad()
def test_teacher_forced_logits_equal_contiguous(name):
    m = model(name)
    g = torch.Generator().manual_seed(1)
    seqs = [torch.randint(0, m.c.vocab_size, (n + STEPS,), generator=g) for n in LENS]
    ids = torch.full((len(LENS), max(LENS)), 3, dtype=torch.long)
    for b, n in enumerate(LENS):
        ids[b, :n] = seqs[b][:n]
    lens = torch.tensor(LENS)

    def ragged(**kw):
        cache = m.new_cache(len(LENS), CACHE, **kw)
        if kw:
            for b, n in enumerate(LENS):
                cache.reserve(b, n + STEPS)
            assert cache.pages_used == 5
        out = [m.step(ids, cache, 0, last=lens - 1)]
        state = RaggedDecodeState(len(LENS), CACHE, "cpu")
        state.set(lens)
        for i in range(STEPS):
            out.append(m.step_graph(torch.stack([s[n + i] for s, n in zip(seqs, LENS)])[:, None], cache, state))
            state.advance()
        return torch.stack(out)

    assert torch.equal(ragged(page_size=PAGE, num_pages=6), ragged())

    def uniform(**kw):
        cache = m.new_cache(2, CACHE, **kw)
        if kw:
            for b in range(2):
                cache.reserve(b, 24 + STEPS)
        x = torch.stack([seqs[2], seqs[2].flip(0)])
        out = [m.step(x[:, :20], cache, 0)]
        for i in range(4):                                         # eager steps with a host position
            out.append(m.step(x[:, 20 + i:21 + i], cache, 20 + i))
        state = DecodeState(2, CACHE, "cpu")
        state.set(24)
        for i in range(4):                                         # ... then the graph step's uniform state
            out.append(m.step_graph(x[:, 24 + i:25 + i], cache, state))
            state.advance()
        return torch.stack(out)

    assert torch.equal(uniform(page_size=PAGE), uniform())


# ------------------------------------------------------------------ refusals
def test_refusals():
    m = model("llama3_tiny")
    ids = prompts(m)
    with pytest.raises(NotImplementedError, match="fp8"):
        generate(m, ids, 2, greedy=True, kv_cache="fp8", page_size=PAGE)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.new_cache(2, CACHE, kv_cache="fp8", page_size=PAGE)
    with pytest.raises(NotImplementedError, match="fp8"):
        model("gemma_tiny").new_cache(2, CACHE, kv_cache="fp8", page_size=PAGE)
    for bad in (24, 8, 512, 0, -16, 16.0, "16"):
        with pytest.raises(ValueError):
            m.new_cache(2, CACHE, page_size=bad)
        with pytest.raises(ValueError):
            PagedKVCache(1, 2, CACHE, 2, 8, page_size=bad)
    with pytest.raises(ValueError):
        generate(m, ids, 2, greedy=True, page_size=48)
    with pytest.raises(ValueError):
        m.new_cache(2, CACHE, num_pages=4)                         # num_pages without page_size
    with pytest.raises(ValueError):
        PagedKVCache(1, 2, CACHE, 2, 8, page_size=PAGE, num_pages=1)
    for ps in (16, 32, 64, 128, 256):
        assert PagedKVCache(1, 1, 300, 2, 8, page_size=ps, dtype=torch.float32).pages_per_seq == -(-300 // ps)
    assert PagedKVCache(1, 1, 300, 2, 8, dtype=torch.float32).page_size == 64      # the default

    from solvingpapers_amd.models import deepseekv3, gpt
    d = deepseekv3.DeepSeekV3(deepseekv3.config("dsv3_tiny"), seed=0).eval()
    with pytest.raises(NotImplementedError, match="DeepSeek"):
        d.new_cache(2, 16, page_size=PAGE)
    with pytest.raises(NotImplementedError, match="DeepSeek"):
        generate(d, torch.zeros(1, 4, dtype=torch.long), 2, greedy=True, page_size=PAGE)
    gm = gpt.GPT(gpt.config("gpt_tiny_cpu"), seed=0).eval()
    with pytest.raises(NotImplementedError, match="GPT"):
        gm.new_cache(2, 16, page_size=PAGE)
    with pytest.raises(NotImplementedError, match="GPT"):
        generate(gm, torch.zeros(1, 4, dtype=torch.long), 2, greedy=True, page_size=PAGE)
    with pytest.raises(ValueError):
        PagedKV(torch.zeros(4, 16, 2, 8), torch.zeros(4, 16, 2, 8), torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        PagedKV(torch.zeros(4, 24, 2, 8), torch.zeros(4, 24, 2, 8), torch.zeros(2, 3, dtype=torch.int32))
