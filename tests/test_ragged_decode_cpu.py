"""Ragged-batch decoding on the CPU oracles: generate(prompt_lens=) token-for-token against
single-sequence runs (both cache formats, eos), RaggedDecodeState arithmetic, KVCache.rows views,
the models that do not cover ragged batches, and the scalar oracles against the per-row ones."""
import math

import pytest
import torch

from solvingpapers_amd.infer import KVCache, RaggedDecodeState, generate
from solvingpapers_amd.models import deepseekv3, gemma, gpt, llama3
from solvingpapers_amd.ops import reference as R
from solvingpapers_amd.ops.attention import KV8, decode_attention, kv_cache_attend, rope_kv_cache_write_
from solvingpapers_amd.ops.layout import gather_rows
from solvingpapers_amd.ops.rope import RopeCache

LENS = (3, 9, 6)
T0, N, PAD = 9, 7, 1023
SEED = 0   # model and prompt seed: the top-2 gap precondition below holds for it (asserted, not assumed)


def _model(name):
    if name == "llama3_tiny":
        return llama3.Llama3(llama3.config(name), dtype=torch.float32, seed=SEED).eval()
    return gemma.Gemma(gemma.config(name), dtype=torch.float32, seed=SEED).eval()


def _padded_prompts(m, filler):
    g = torch.Generator().manual_seed(SEED)
    ids = torch.randint(0, m.c.vocab_size - 1, (len(LENS), T0), generator=g)
    for b, n in enumerate(LENS):          # what stands right of a prompt must not matter
        ids[b, n:] = filler
    return ids


@torch.no_grad()
def _single(m, prompt, n, kv_cache, eos=None):
    """Greedy single-sequence run through step(): (tokens [n], smallest top-2 logit gap met)."""
    cache = m.new_cache(1, prompt.shape[1] + n, kv_cache=kv_cache)
    lg = m.step(prompt, cache, 0)
    pos, toks, gap = prompt.shape[1], [], math.inf
    for i in range(n):
        top = lg[0].topk(2).values
        gap = min(gap, float(top[0] - top[1]))
        toks.append(int(lg[0].argmax()))
        if i + 1 == n or toks[-1] == eos:
            break
        lg = m.step(torch.tensor([[toks[-1]]]), cache, pos)
        pos += 1
    return toks, gap


@pytest.mark.parametrize("kv_cache", [None, "fp8"])
@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_generate_prompt_lens_matches_single_sequences(name, kv_cache):
    m = _model(name)
    ids = _padded_prompts(m, filler=7)
    singles = [_single(m, ids[b:b + 1, :n], N, kv_cache) for b, n in enumerate(LENS)]
    for toks, gap in singles:             # precondition: greedy equality is no coin toss
        assert gap > 1e-3, gap
    out = m.generate(ids, N, greedy=True, kv_cache=kv_cache, prompt_lens=list(LENS), pad_token_id=PAD)
    assert out.shape == (len(LENS), T0 + N)
    for b, n in enumerate(LENS):
        ref = m.generate(ids[b:b + 1, :n], N, greedy=True, kv_cache=kv_cache)[0]
        assert ref[n:].tolist() == singles[b][0]
        assert torch.equal(out[b, :n + N], ref), (b, out[b], ref)
        assert (out[b, n + N:] == PAD).all()
    # the pads to the right of a prompt are ignored, and prompt_lens may be a tensor
    out2 = generate(m, _padded_prompts(m, filler=11), N, greedy=True, kv_cache=kv_cache,
                    prompt_lens=torch.tensor(LENS), pad_token_id=PAD)
    assert torch.equal(out2, out)


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_generate_prompt_lens_eos_stops_rows_independently(name):
    m = _model(name)
    ids = _padded_prompts(m, filler=7)
    free = [_single(m, ids[b:b + 1, :n], N, None) for b, n in enumerate(LENS)]
    eos = free[1][0][2]                   # row 1 emits it as its third token
    singles = [_single(m, ids[b:b + 1, :n], N, None, eos=eos) for b, n in enumerate(LENS)]
    assert len(singles[1][0]) <= 3 and any(len(t) == N for t, _ in singles), [t for t, _ in singles]
    for _, gap in singles:
        assert gap > 1e-3, gap
    out = m.generate(ids, N, greedy=True, eos_token_id=eos, prompt_lens=LENS, pad_token_id=PAD)
    assert out.shape == (len(LENS), T0 + N)
    for b, n in enumerate(LENS):
        toks = singles[b][0]              # up to and including the row's first eos
        ref = m.generate(ids[b:b + 1, :n], N, greedy=True, eos_token_id=eos)[0]
        assert ref[n:n + len(toks)].tolist() == toks
        assert out[b, :n].tolist() == ids[b, :n].tolist()
        assert out[b, n:n + len(toks)].tolist() == toks
        assert (out[b, n + len(toks):] == PAD).all()


def test_prompt_lens_validation():
    m = _model("llama3_tiny")
    ids = _padded_prompts(m, filler=7)
    for bad in ([3, 9], [0, 9, 6], [3, 10, 6]):
        with pytest.raises(ValueError):
            m.generate(ids, 2, greedy=True, prompt_lens=bad)


def test_ragged_state_arithmetic():
    s = RaggedDecodeState(3, 40, "cpu")
    assert s.per_row and s.index.shape == (3,) and s.index.dtype == torch.long
    assert s.positions.shape == (3, 1) and s.positions.dtype == torch.int32
    assert s.kv_len.shape == (3,) and s.kv_len.dtype == torch.int32
    assert s.active.dtype == torch.int32 and s.active.tolist() == [1, 1, 1]
    s.set(4)
    assert s.index.tolist() == [4, 4, 4] and s.kv_len.tolist() == [5, 5, 5]
    s.set(torch.tensor([5, 17, 24]))
    assert s.index.tolist() == [5, 17, 24] and s.positions[:, 0].tolist() == [5, 17, 24]
    assert s.kv_len.tolist() == [6, 18, 25]
    s.set([1, 2, 3])
    assert s.index.tolist() == [1, 2, 3]
    s.set_row(1, 9)
    assert s.index.tolist() == [1, 9, 3] and s.positions[:, 0].tolist() == [1, 9, 3] and s.kv_len.tolist() == [2, 10, 4]
    s.active[2] = 0
    for _ in range(3):
        s.advance()
    assert s.index.tolist() == [4, 12, 3] and s.positions[:, 0].tolist() == [4, 12, 3]
    assert s.kv_len.tolist() == [5, 13, 4]
    with pytest.raises(ValueError):
        s.set([1, 2])
    from solvingpapers_amd.infer import DecodeState
    assert DecodeState(2, 8, "cpu").per_row is False


@pytest.mark.parametrize("quant", [None, "fp8"])
def test_kv_cache_rows_are_views(quant):
    c = KVCache(2, 3, 8, 2, 16, dtype=torch.float32, quant=quant)
    sub = c.rows(1, 2)
    assert isinstance(sub, KVCache) and len(sub) == 2 and sub.quant == quant and sub.max_len == 8
    g = torch.Generator().manual_seed(0)
    k, v = torch.randn(1, 4, 2, 16, generator=g), torch.randn(1, 4, 2, 16, generator=g)
    kd, vd = sub.write(1, k, v, 2)        # through the view ...
    pk, pv = c.dequantized(1, 6)          # ... shows in the parent, batch row 1 only
    assert torch.equal(pk[1:2, 2:6], kd[:, 2:6]) and torch.equal(pv[1:2, 2:6], vd[:, 2:6])
    assert pk[1, 2:6].abs().sum() > 0 and pk[0].abs().sum() == 0 and pk[2].abs().sum() == 0
    if quant:
        assert isinstance(sub[1], KV8)
        assert sub[1].kq.data_ptr() == c[1].kq[1:2].data_ptr() and sub[1].ks.data_ptr() == c[1].ks[1:2].data_ptr()
        assert (c[1].ks[1, :, 2:6] != 0).any() and (c[1].ks[0] == 0).all()
    else:
        assert torch.equal(pk[1:2, 2:6], k) and sub[1][0].data_ptr() == c[1][0][1:2].data_ptr()
        assert (c[0][0] == 0).all()
    with pytest.raises(IndexError):
        c.rows(2, 4)


def test_gpt_and_deepseek_raise_on_ragged():
    m = gpt.GPT(gpt.config("gpt_tiny_cpu", block_size=16)).eval()
    ids = torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="ragged"):
        m.generate(ids, 2, prompt_lens=[2, 4])
    with pytest.raises(NotImplementedError, match="ragged"):
        generate(m, ids, 2, greedy=True, prompt_lens=[2, 4])
    d = deepseekv3.DeepSeekV3(deepseekv3.config("dsv3_tiny")).eval()
    with pytest.raises(NotImplementedError, match="ragged"):
        d.generate(ids, 2, greedy=True, prompt_lens=[2, 4])
    with pytest.raises(NotImplementedError, match="ragged"):
        generate(d, ids, 2, greedy=True, prompt_lens=[2, 4])
    with pytest.raises(NotImplementedError, match="ragged"):
        d.step_graph(ids[:, :1], d.new_cache(2, 8), RaggedDecodeState(2, 8, "cpu"))


def _packed(B, T, H, Hkv, hd, seed):
    return torch.randn(B, T, H + 2 * Hkv, hd, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fp8", [False, True])
def test_rope_kv_write_oracle_scalar_vs_per_row(mode, fp8):
    B, T, H, Hkv, hd, Tmax = 3, 2, 4, 2, 16, 12
    cos, sin = RopeCache.get(Tmax, hd, 10000.0, "cpu")

    def cache():
        return KV8.zeros(B, Tmax, Hkv, hd, dtype=torch.float32) if fp8 else \
            (torch.zeros(B, Tmax, Hkv, hd), torch.zeros(B, Tmax, Hkv, hd))

    def same(a, b):
        ts = (("kq", "ks", "vq", "vs") if fp8 else (0, 1))
        get = (lambda c, t: getattr(c, t).view(torch.uint8)) if fp8 else (lambda c, t: c[t])
        return all(torch.equal(get(a, t), get(b, t)) for t in ts)

    pos = torch.tensor([[5, 6]] * B, dtype=torch.int32)
    xa, xb = _packed(B, T, H, Hkv, hd, 1), _packed(B, T, H, Hkv, hd, 1)
    ca, cb = cache(), cache()
    rope_kv_cache_write_(ca, xa, cos, sin, pos, torch.tensor([5]), H, Hkv, mode)                      # scalar
    rope_kv_cache_write_(cb, xb, cos, sin, pos, torch.tensor([5, 5, 5]), H, Hkv, mode, per_row=True)  # equal rows
    assert torch.equal(xa, xb) and same(ca, cb)
    # q rotated as reference.rope does it, k / v where the scalar writer of one sequence puts them
    x = _packed(B, T, H, Hkv, hd, 1)
    assert torch.equal(xa[:, :, :H], R.rope(x[:, :, :H], cos, sin, interleaved=mode == 0, positions=pos))
    idx = torch.tensor([0, 7, Tmax - 1])
    posr = idx[:, None].int() + torch.arange(T, dtype=torch.int32)[None]
    posr = posr.clamp_max(Tmax - 1)
    xr, cr = _packed(B, T, H, Hkv, hd, 2), cache()
    rope_kv_cache_write_(cr, xr, cos, sin, posr, idx, H, Hkv, mode, per_row=True)   # last row: t = 1 is dropped
    cs = cache()
    for b in range(B):
        xs = _packed(B, T, H, Hkv, hd, 2)[b:b + 1]
        sub = KV8(cs.kq[b:b + 1], cs.ks[b:b + 1], cs.vq[b:b + 1], cs.vs[b:b + 1], cs.dtype) if fp8 else \
            (cs[0][b:b + 1], cs[1][b:b + 1])
        rope_kv_cache_write_(sub, xs, cos, sin, posr[b:b + 1], idx[b:b + 1], H, Hkv, mode)
        assert torch.equal(xs, xr[b:b + 1])
    assert same(cr, cs)


def test_attention_oracle_scalar_vs_per_row():
    B, Tk, H, Hkv, hd = 3, 20, 4, 2, 16
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, 1, H, hd, generator=g)
    k, v = torch.randn(B, Tk, Hkv, hd, generator=g), torch.randn(B, Tk, Hkv, hd, generator=g)
    scalar = decode_attention(q, k, v, kv_len=torch.tensor([11], dtype=torch.int32))
    assert torch.equal(scalar, R.attention(q, k[:, :11], v[:, :11])[0])
    rows = decode_attention(q, k, v, kv_len=torch.tensor([11, 11, 11], dtype=torch.int32), per_row=True)
    assert torch.allclose(rows, scalar, atol=1e-6, rtol=0)
    lens = torch.tensor([1, 20, 7], dtype=torch.int32)
    rag = decode_attention(q, k, v, kv_len=lens, per_row=True)
    for b, n in enumerate(lens.tolist()):
        assert torch.equal(rag[b:b + 1], R.attention(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n])[0])
    # the cache helper: a (k, v) pair and an fp8 layer (the oracle over its dequantised rows)
    assert torch.equal(kv_cache_attend(q, (k, v), kv_len=lens, per_row=True), rag)
    c8 = KV8.zeros(B, Tk, Hkv, hd, dtype=torch.float32)
    for x, qd, sd in ((k, c8.kq, c8.ks), (v, c8.vq, c8.vs)):
        xq, xs = R.quant_kv8(x)
        qd.view(torch.uint8).copy_(xq.view(torch.uint8))
        sd.copy_(xs)
    kd, vd = c8.dequantized(Tk)
    assert torch.equal(kv_cache_attend(q, c8, kv_len=lens, per_row=True),
                       R.attention_per_row(q, kd, vd, lens)[0])
    with pytest.raises(ValueError):
        decode_attention(q, k, v, per_row=True)                                   # per_row without lengths
    with pytest.raises(ValueError):
        decode_attention(q, k, v, kv_len=torch.tensor([3], dtype=torch.int32), per_row=True)


def test_gather_rows_oracle():
    x = torch.randn(3, 5, 8, generator=torch.Generator().manual_seed(0))
    idx = torch.tensor([4, 0, 2])
    got = gather_rows(x, idx)
    assert got.shape == (3, 1, 8)
    assert torch.equal(got, x[torch.arange(3), idx][:, None])


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_step_graph_runs_on_cpu_for_the_uniform_state(name):
    from solvingpapers_amd.infer import DecodeState
    m = _model(name)
    ids = torch.randint(0, m.c.vocab_size, (2, 8), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        full = m(ids).float()
        cache = m.new_cache(2, 8)
        m.step(ids[:, :5], cache, 0)
        st = DecodeState(2, 8, "cpu")
        st.set(5)
        for t in range(5, 8):
            lg = m.step_graph(ids[:, t:t + 1], cache, st)
            st.advance()
            assert torch.allclose(lg, full[:, t], atol=1e-4, rtol=1e-4)
