"""Multi-token steps behind a live cache on the CPU (fp32, the oracle routes): ExtendState, model.extend,
chunked prefill, extend_row and generate(prefill_chunk=) on LLaMA3 and Gemma, contiguous and paged,
against each sequence's own full forward with the cached-versus-full tolerance of
tests/test_ragged_decode_cpu.py (atol = rtol = 1e-4); paged and contiguous logits are bitwise equal (the
CPU paged route is gather + the same oracle); and the refusals."""
import pytest
import torch

from solvingpapers_amd.infer import CacheFull, ExtendState, RaggedDecodeState, generate
from solvingpapers_amd.infer.graph import DecodeState, chunked_prefill, extend_row

LENS = (5, 17, 24)
EXT, STEPS, CACHE, PAGE = 20, 4, 64, 16
TOL = dict(atol=1e-4, rtol=1e-4)
NAMES = ["llama3_tiny", "gemma_tiny"]


def model(name):
    if name == "llama3_tiny":
        from solvingpapers_amd.models import llama3
        return llama3.Llama3(llama3.config(name), seed=0).eval()
    from solvingpapers_amd.models import gemma
    return gemma.Gemma(gemma.config(name), seed=0).eval()


def sequences(m, extra):
    """Three sequences of len_b + extra tokens, their right-padded prompt batch and full forwards."""
    g = torch.Generator().manual_seed(1)
    seqs = [torch.randint(0, m.c.vocab_size, (n + extra,), generator=g) for n in LENS]
    ids = torch.full((len(LENS), max(LENS)), 3, dtype=torch.long)
    for b, n in enumerate(LENS):
        ids[b, :n] = seqs[b][:n]
    with torch.no_grad():
        full = [m(s[None]).float()[0] for s in seqs]
    return seqs, ids, full


def new_cache(m, paged, rows):
    cache = m.new_cache(len(LENS), CACHE, **(dict(page_size=PAGE) if paged else {}))
    if paged:
        for b, r in enumerate(rows):
            cache.reserve(b, r)
    return cache


def step_tokens(seqs, at):
    return torch.stack([s[a] for s, a in zip(seqs, at)])[:, None]


# ------------------------------------------------------------------ ExtendState
def test_extend_state_fields_and_refusals():
    st = ExtendState([3, 0, 10], 4, 16, "cpu")
    assert st.per_row and st.batch == 3 and st.max_len == 16
    assert st.index.dtype == torch.long and st.index.tolist() == [3, 0, 10]
    assert st.positions.dtype == torch.int32 and st.positions.tolist() == [[3, 4, 5, 6], [0, 1, 2, 3], [10, 11, 12, 13]]
    assert st.kv_len.dtype == torch.int32 and st.kv_len.tolist() == [7, 4, 14]
    assert isinstance(st, RaggedDecodeState)
    assert ExtendState(torch.tensor([12]), 4, 16, "cpu").kv_len.tolist() == [16]     # start + T == max_len fits
    for starts, T in (([-1, 0], 2), ([0, 13], 4), ([0], 17), ([0], 0), ([], 1)):
        with pytest.raises(ValueError):
            ExtendState(starts, T, 16, "cpu")


# ------------------------------------------------------------------ model.extend
@pytest.mark.parametrize("name", NAMES)
@torch.no_grad()
def test_extend_matches_full_forward(name):
    m = model(name)
    seqs, ids, full = sequences(m, EXT + STEPS)
    lens = torch.tensor(LENS)
    new = torch.stack([s[n:n + EXT] for s, n in zip(seqs, LENS)])
    short = (EXT, 12, 7)                      # the same step right-padded: logits at each row's last real token

    def run(paged):
        cache = new_cache(m, paged, [n + EXT + STEPS for n in LENS])
        out = [m.step(ids, cache, 0, last=lens - 1)]
        out.append(m.extend(new, cache, list(LENS)))
        padded = new.clone()
        for b, n in enumerate(short):
            padded[b, n:] = 3
        out.append(m.extend(padded, cache, lens, last=torch.tensor(short) - 1))    # rewrites the same rows
        m.extend(new, cache, list(LENS))      # ... and the real tokens again, for the steps that follow
        state = RaggedDecodeState(len(LENS), CACHE, "cpu")
        state.set(lens + EXT)
        for i in range(STEPS):
            out.append(m.step_graph(step_tokens(seqs, [n + EXT + i for n in LENS]), cache, state))
            state.advance()
        return out

    got, pg = run(False), run(True)
    assert all(torch.equal(a, b) for a, b in zip(got, pg))
    for b, n in enumerate(LENS):
        assert torch.allclose(got[0][b], full[b][n - 1], **TOL)
        assert torch.allclose(got[1][b], full[b][n + EXT - 1], **TOL)
        assert torch.allclose(got[2][b], full[b][n + short[b] - 1], **TOL)
        for i in range(STEPS):
            assert torch.allclose(got[3 + i][b], full[b][n + EXT + i], **TOL)


# ------------------------------------------------------------------ chunked prefill
@pytest.mark.parametrize("name", NAMES)
@torch.no_grad()
def test_chunked_prefill_matches_full_forward(name):
    m = model(name)
    seqs, ids, full = sequences(m, STEPS)
    lens = torch.tensor(LENS)

    def run(paged, chunk):
        cache = new_cache(m, paged, [n + STEPS for n in LENS])
        out = [chunked_prefill(m, cache, ids, lens, chunk)]
        state = RaggedDecodeState(len(LENS), CACHE, "cpu")
        state.set(lens)
        for i in range(STEPS):
            out.append(m.step_graph(step_tokens(seqs, [n + i for n in LENS]), cache, state))
            state.advance()
        return out, (cache.pages_used if paged else None)

    for chunk in (16, 7, 24, 100):            # two chunks, four ragged ones, exactly one, more than the prompt
        (got, _), (pg, used) = run(False, chunk), run(True, chunk)
        assert all(torch.equal(a, b) for a, b in zip(got, pg))
        assert used == 5                      # 1 + 2 + 2 pages: the pads cost none
        for b, n in enumerate(LENS):
            for i, lg in enumerate(got):
                assert torch.allclose(lg[b], full[b][n - 1 + i], **TOL), (chunk, b, i)
    # a chunk that holds the whole prompt is the unchunked pass, bitwise
    cache = new_cache(m, False, None)
    assert torch.equal(run(False, 100)[0][0], m.step(ids, cache, 0, last=lens - 1))


def test_chunked_prefill_skips_chunks_past_every_length():
    m = model("llama3_tiny")
    ids = torch.full((2, 40), 3, dtype=torch.long)
    calls = []
    ext = m.extend
    m.extend = lambda x, cache, starts, last=None: calls.append(list(starts)) or ext(x, cache, starts, last=last)
    with torch.no_grad():
        chunked_prefill(m, m.new_cache(2, CACHE), ids, torch.tensor([3, 20]), 8)
    assert calls == [[8, 8], [16, 16]]        # columns 24.. lie past both lengths


# ------------------------------------------------------------------ extend_row
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("name", NAMES)
@torch.no_grad()
def test_extend_row_mid_stream(name, paged):
    m = model(name)
    seqs, ids, full = sequences(m, 2 * STEPS)
    lens = torch.tensor(LENS)
    g = torch.Generator().manual_seed(5)
    turn = torch.randint(0, m.c.vocab_size, (EXT + STEPS,), generator=g)
    joined = torch.cat([seqs[1][:LENS[1] + STEPS], turn])
    full1 = m(joined[None]).float()[0]

    def run(with_turn):
        cache = new_cache(m, paged, [n + 2 * STEPS for n in LENS])
        m.step(ids, cache, 0, last=lens - 1)
        state = RaggedDecodeState(len(LENS), CACHE, "cpu")
        state.set(lens)
        out = []
        for i in range(2 * STEPS):
            if i == STEPS and with_turn:
                lg = extend_row(m, cache, state, 1, turn[:EXT], reserve=LENS[1] + STEPS + EXT + STEPS)
                assert torch.allclose(lg, full1[LENS[1] + STEPS + EXT - 1], **TOL)
                assert state.index.tolist() == [LENS[0] + STEPS, LENS[1] + STEPS + EXT, LENS[2] + STEPS]
                assert state.kv_len.tolist() == [p + 1 for p in state.index.tolist()]
            tok = step_tokens(seqs, [n + i for n in LENS])
            if i >= STEPS and with_turn:
                tok[1, 0] = turn[EXT + i - STEPS]
            out.append(m.step_graph(tok, cache, state))
            state.advance()
        return out

    got, ctl = run(True), run(False)
    for i in range(2 * STEPS):
        for b in (0, 2):                      # the other slots: the bits of a run that saw no extend_row
            assert torch.equal(got[i][b], ctl[i][b])
    for i in range(STEPS):                    # slot 1 goes on behind its new turn
        assert torch.allclose(got[STEPS + i][1], full1[LENS[1] + STEPS + EXT + i], **TOL)


@torch.no_grad()
def test_extend_row_refusals():
    m = model("llama3_tiny")
    _, ids, _ = sequences(m, 0)
    lens = torch.tensor(LENS)
    cache = m.new_cache(len(LENS), CACHE, page_size=PAGE, num_pages=6)     # 1 + 2 + 2 pages and the null page
    for b, n in enumerate(LENS):
        cache.reserve(b, n)
    m.step(ids, cache, 0, last=lens - 1)
    state = RaggedDecodeState(len(LENS), CACHE, "cpu")
    state.set(lens)
    table, idx, kvl = cache.table.clone(), state.index.clone(), state.kv_len.clone()
    pool = [(l.k.clone(), l.v.clone()) for l in cache]
    with pytest.raises(CacheFull):            # 5 + 20 rows: a second page for slot 0, none is free
        extend_row(m, cache, state, 0, torch.zeros(EXT, dtype=torch.long))
    with pytest.raises(ValueError):           # 24 + 40 rows reach the end of the cache
        extend_row(m, cache, state, 2, torch.zeros(CACHE - LENS[2], dtype=torch.long))
    with pytest.raises(ValueError):
        extend_row(m, cache, state, 1, torch.zeros(0, dtype=torch.long))
    with pytest.raises(IndexError):
        extend_row(m, cache, state, 3, torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError, match="ragged"):
        extend_row(m, cache, DecodeState(len(LENS), CACHE, "cpu"), 0, torch.zeros(2, dtype=torch.long))
    assert cache.pages_used == 5 and torch.equal(cache.table, table) and torch.equal(cache.block_table, table)
    assert torch.equal(state.index, idx) and torch.equal(state.kv_len, kvl)
    assert all(torch.equal(l.k, k) and torch.equal(l.v, v) for l, (k, v) in zip(cache, pool))
    lg = extend_row(m, cache, state, 0, torch.zeros(11, dtype=torch.long))     # 16 rows: the page it holds
    assert torch.isfinite(lg).all() and cache.pages_used == 5 and state.index.tolist() == [16, 17, 24]


# ------------------------------------------------------------------ generate(prefill_chunk=)
@pytest.mark.parametrize("name", NAMES)
def test_generate_prefill_chunk_returns_the_unchunked_tokens(name):
    m = model(name)
    ids = torch.randint(0, m.c.vocab_size, (len(LENS), max(LENS)), generator=torch.Generator().manual_seed(0))
    want = generate(m, ids, 6, greedy=True, prompt_lens=LENS)
    for chunk in (16, 5):
        assert torch.equal(generate(m, ids, 6, greedy=True, prompt_lens=LENS, prefill_chunk=chunk), want)
        assert torch.equal(generate(m, ids, 6, greedy=True, prompt_lens=LENS, prefill_chunk=chunk, page_size=PAGE,
                                    num_pages=6), want)
    assert torch.equal(generate(m, ids, 6, greedy=True, prompt_lens=LENS, prefill_chunk=None), want)


def test_prefill_chunk_refusals():
    m = model("llama3_tiny")
    ids = torch.zeros(2, 8, dtype=torch.long)
    with pytest.raises(ValueError, match="prompt_lens"):           # a uniform batch
        generate(m, ids, 2, greedy=True, prefill_chunk=4)
    for bad in (0, -4, 4.0, True):
        with pytest.raises(ValueError):
            generate(m, ids, 2, greedy=True, prompt_lens=[8, 3], prefill_chunk=bad)
    from solvingpapers_amd.models import deepseekv3, gpt
    d = deepseekv3.DeepSeekV3(deepseekv3.config("dsv3_tiny"), seed=0).eval()
    with pytest.raises(NotImplementedError, match="DeepSeek"):
        generate(d, torch.zeros(2, 4, dtype=torch.long), 2, greedy=True, prompt_lens=[4, 2], prefill_chunk=2)
    gm = gpt.GPT(gpt.config("gpt_tiny_cpu"), seed=0).eval()
    with pytest.raises(NotImplementedError, match="GPT"):
        generate(gm, torch.zeros(2, 4, dtype=torch.long), 2, greedy=True, prompt_lens=[4, 2], prefill_chunk=2)
    assert not hasattr(d, "extend") and not hasattr(gm, "extend")
    with pytest.raises(NotImplementedError, match="extend"):
        chunked_prefill(gm, None, torch.zeros(2, 4, dtype=torch.long), torch.tensor([4, 2]), 2)
