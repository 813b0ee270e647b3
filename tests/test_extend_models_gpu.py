"""Multi-token steps behind a live cache on the GPU: LLaMA3 / Gemma ``extend`` (the extend-attention
kernel, csrc/kernels/attention_extend.hip, behind the fused RoPE + cache write), chunked
``GraphDecoder.prefill`` and ``extend_row`` between replays, contiguous and paged (page 16). Logits are held
to rel L2 2e-2 of each sequence's own full forward (the bound and comparison of
tests/test_paged_kv_gpu.py::check_against_full); paged and contiguous runs give the same bits."""
import functools

import pytest
import torch

from solvingpapers_amd.infer import CacheFull, GraphDecoder

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
LENS = (5, 17, 24)
EXT, STEPS, CACHE = 20, 8, 64
PAGED = dict(page_size=16)
NAMES = ["llama3_tiny", "gemma_tiny"]
BOUND = 2e-2


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


@functools.lru_cache(maxsize=None)
def model_data(name):
    """The bf16 model, three sequences of len_b + EXT + STEPS tokens, the right-padded prompt batch and
    each sequence's own full forward: built once."""
    if name == "llama3_tiny":
        from solvingpapers_amd.models import llama3
        m = llama3.Llama3(llama3.config(name), device=DEV, dtype=BF, seed=0).eval()
    else:
        from solvingpapers_amd.models import gemma
        m = gemma.Gemma(gemma.config(name), device=DEV, dtype=BF, seed=0).eval()
    g = torch.Generator().manual_seed(0)
    seqs = [torch.randint(0, m.c.vocab_size, (n + EXT + STEPS,), generator=g).to(DEV) for n in LENS]
    ids = torch.full((len(LENS), max(LENS)), 3, dtype=torch.long, device=DEV)   # right-padded with token 3
    for b, n in enumerate(LENS):
        ids[b, :n] = seqs[b][:n]
    with torch.no_grad():
        full = [m(s[None]).float()[0] for s in seqs]
    return m, seqs, ids, full


def tokens_at(seqs, at):
    return torch.stack([s[a] for s, a in zip(seqs, at)])[:, None]


def check(what, lg, full, at):
    for b, a in enumerate(at):
        e = rel(lg[b], full[b][a])
        print(f"{what} row {b} at {a}: rel {e:.3e}")
        assert e < BOUND, (what, b, e)


# ------------------------------------------------------------------ model.extend
@pytest.mark.parametrize("name", NAMES)
@torch.no_grad()
def test_extend_after_ragged_prefill(name):
    """20 more tokens per sequence behind a ragged prefill: 40 (LLaMA3, G = 2) and 160 (Gemma, G = 8) rows per
    kv head, both past the decode kernel's 16."""
    m, seqs, ids, full = model_data(name)
    lens = torch.tensor(LENS, device=DEV)
    new = torch.stack([s[n:n + EXT] for s, n in zip(seqs, LENS)])

    def run(**paged):
        cache = m.new_cache(len(LENS), CACHE, **paged)
        if paged:
            for b, n in enumerate(LENS):
                cache.reserve(b, n + EXT)
        lg0 = m.step(ids, cache, 0, last=lens - 1)
        return lg0, m.extend(new, cache, list(LENS)), m.extend(new, cache, lens, last=torch.full_like(lens, 6))

    got, pg = run(), run(**PAGED)
    assert all(torch.equal(a, b) for a, b in zip(got, pg))
    check(f"{name} prefill", got[0], full, [n - 1 for n in LENS])
    check(f"{name} extend", got[1], full, [n + EXT - 1 for n in LENS])
    check(f"{name} extend last=6", got[2], full, [n + 6 for n in LENS])


# ------------------------------------------------------------------ chunked GraphDecoder.prefill
# chunk 16 over 24 columns leaves a second block of 8: 64 rows per kv head on Gemma (G = 8, the extend
# kernel) but 16 on LLaMA3 (G = 2, still the decode kernel); chunk 12 makes it 12 columns, 24 rows on
# LLaMA3, so the extend kernel runs behind a chunk on both models
@pytest.mark.parametrize("chunk", [16, 12])
@pytest.mark.parametrize("name", NAMES)
@torch.no_grad()
def test_chunked_prefill_and_replays(name, chunk):
    m, seqs, ids, full = model_data(name)
    C = chunk

    def run(chunk, **paged):
        dec = GraphDecoder(m, len(LENS), CACHE, ragged=True, **paged)
        lg0 = dec.prefill(ids, LENS, chunk=chunk)
        used = dec.cache.pages_used if paged else None
        if paged:
            for b, n in enumerate(LENS):
                dec.reserve(b, n + STEPS)
        lgs = []
        for i in range(STEPS):
            dec.ids.copy_(tokens_at(seqs, [n + i for n in LENS]))
            dec.graph.replay()
            lgs.append(dec.logits.clone())
        return lg0, lgs, used

    c0, cs, _ = run(C)
    p0, ps, used = run(C, **PAGED)
    _, _, used_plain = run(None, **PAGED)
    assert torch.equal(c0, p0) and all(torch.equal(a, b) for a, b in zip(cs, ps))
    assert used == used_plain == 5              # 1 + 2 + 2 pages: a chunk's pad rows cost none
    check(f"{name} chunked prefill", c0, full, [n - 1 for n in LENS])
    for i, lg in enumerate(cs):
        check(f"{name} replay {i} after chunked prefill", lg, full, [n + i for n in LENS])
    u0, _, _ = run(None)
    check(f"{name} unchunked prefill", u0, full, [n - 1 for n in LENS])
    with pytest.raises(ValueError, match="prompt_lens"):
        GraphDecoder(m, len(LENS), CACHE).prefill(ids, chunk=C)


# ------------------------------------------------------------------ extend_row between replays
@pytest.mark.parametrize("paged", [{}, PAGED], ids=["contiguous", "paged"])
@pytest.mark.parametrize("name", NAMES)
@torch.no_grad()
def test_extend_row_mid_stream(name, paged):
    m, seqs, ids, full = model_data(name)
    g = torch.Generator().manual_seed(7)
    turn = torch.randint(0, m.c.vocab_size, (EXT + 4,), generator=g).to(DEV)
    joined = torch.cat([seqs[1][:LENS[1] + 4], turn])
    full1 = m(joined[None]).float()[0]

    def start():
        dec = GraphDecoder(m, len(LENS), CACHE, ragged=True, **paged)
        dec.prefill(ids, LENS, reserve=[n + 8 for n in LENS] if paged else None)
        for i in range(4):
            dec.ids.copy_(tokens_at(seqs, [n + i for n in LENS]))
            dec.graph.replay()
        return dec

    dec, ctl = start(), start()                 # the control: the same stream, no extend_row
    lg = dec.extend_row(1, turn[:EXT], reserve=LENS[1] + 4 + EXT + 4)
    e = rel(lg, full1[LENS[1] + 4 + EXT - 1])
    print(f"{name} extend_row logits: rel {e:.3e}")
    assert e < BOUND, e
    assert dec.state.index.tolist() == [LENS[0] + 4, LENS[1] + 4 + EXT, LENS[2] + 4]
    if paged:
        assert dec.cache.held(1) == 3 and dec.cache.held(0) == ctl.cache.held(0)   # 45 rows: three 16-row pages
    for i in range(4):
        tok = tokens_at(seqs, [n + 4 + i for n in LENS])
        ctl.ids.copy_(tok)
        ctl.graph.replay()
        tok[1, 0] = turn[EXT + i]
        dec.ids.copy_(tok)
        dec.graph.replay()
        e = rel(dec.logits[1], full1[LENS[1] + 4 + EXT + i])
        print(f"{name} slot 1 after extend_row, step {i}: rel {e:.3e}")
        assert e < BOUND, e
        for b in (0, 2):                        # untouched slots: the same bits as the control
            assert torch.equal(dec.logits[b], ctl.logits[b]), (i, b)


@torch.no_grad()
def test_extend_row_refusals():
    m, seqs, ids, _ = model_data("llama3_tiny")
    dec = GraphDecoder(m, len(LENS), CACHE, ragged=True, page_size=16, num_pages=6)   # 1 + 2 + 2 pages + null
    dec.prefill(ids, LENS)
    idx, kvl, table = dec.state.index.clone(), dec.state.kv_len.clone(), dec.cache.table.clone()
    with pytest.raises(CacheFull):              # 5 + 20 rows need a second page; none is free
        dec.extend_row(0, seqs[0][:EXT])
    assert dec.cache.pages_used == 5 and torch.equal(dec.cache.table, table)
    assert torch.equal(dec.cache.block_table.cpu(), table)
    assert torch.equal(dec.state.index, idx) and torch.equal(dec.state.kv_len, kvl)
    with pytest.raises(ValueError):             # 24 + 40 rows reach the end of the cache
        dec.extend_row(2, torch.zeros(CACHE - LENS[2], dtype=torch.long, device=DEV))
    assert torch.equal(dec.state.index, idx)
    with pytest.raises(ValueError, match="ragged"):
        GraphDecoder(m, len(LENS), CACHE).extend_row(0, seqs[0][:EXT])
