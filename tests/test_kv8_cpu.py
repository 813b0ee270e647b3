"""fp8 KV cache on the CPU oracle path: quantiser contract, cached generation with
``kv_cache="fp8"``, layer-0 exactness against the unquantised cache, cache size, and E_ref (the
fp8-cache vs bf16-cache logit error the GPU tests bound)."""
import pytest
import torch

from solvingpapers_amd.infer import GenerationStats, KVCache, generate
from solvingpapers_amd.ops import reference as R


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _model(name, dtype=torch.float32):
    if name == "llama3_tiny":
        from solvingpapers_amd.models import llama3
        return llama3.Llama3(llama3.config(name), dtype=dtype, seed=1).eval()
    if name == "gemma_tiny":
        from solvingpapers_amd.models import gemma
        return gemma.Gemma(gemma.config(name), dtype=dtype, seed=1).eval()
    from solvingpapers_amd.models import gpt
    return gpt.GPT(gpt.GPTConfig(vocab_size=256, emb_dim=64, num_heads=4, num_layers=2, block_size=32,
                                 dropout_rate=0.0), dtype=dtype, seed=1).eval()


def kv_rows(B, T, Hkv, hd, lo, hi, gen):
    """randn * 2^e, e random in [lo, hi] per (b, token, head): many distinct row scales."""
    e = torch.randint(lo, hi + 1, (B, T, Hkv, 1), generator=gen)
    return (torch.randn(B, T, Hkv, hd, generator=gen) * torch.exp2(e.float())).bfloat16()


def test_quant_kv8_contract():
    g = torch.Generator().manual_seed(0)
    x = kv_rows(2, 9, 3, 64, -6, 6, g)
    x[0, 0, 0] = 0                      # an all-zero row: scale byte 127, zero bytes
    x[1, 2, 1, 5] = 448.0 * 2.0 ** 3    # amax exactly 448 * 2^e: no round-up of the exponent
    q, s = R.quant_kv8(x)
    assert q.dtype == torch.float8_e4m3fn and q.shape == x.shape
    assert s.dtype == torch.uint8 and s.shape == (2, 3, 9) and s.is_contiguous()
    assert s.unique().numel() > 1
    assert s[0, 0, 0] == 127 and (q[0, 0, 0].float() == 0).all()
    e = s.transpose(1, 2).float() - 127                      # [B, T, Hkv]
    amax = x.float().abs().amax(-1)
    assert (amax <= 448 * torch.exp2(e)).all()               # fits ...
    nz = amax > 0
    assert (amax[nz] > 448 * torch.exp2(e[nz] - 1)).all()    # ... and e is the smallest that does
    d = R.dequant_kv8(q, s)
    assert torch.equal(d, d.bfloat16().float())              # every dequantised value exact in bf16
    # scaled values lie in [-448, 448], where the widest e4m3 step is 32: |x - d| <= 16 * 2^e
    assert ((x.float() - d).abs() <= 16 * torch.exp2(e)[..., None]).all()
    assert rel(d, x) < 0.04
    # quantising the dequantised rows reproduces them (the cache is a fixed point of its own quantiser)
    q2, s2 = R.quant_kv8(d)
    assert torch.equal(R.dequant_kv8(q2, s2), d)


def test_reference_attn_decode_q8_is_attention_on_dequantised_rows():
    g = torch.Generator().manual_seed(1)
    k, v = kv_rows(2, 20, 2, 64, -3, 0, g), kv_rows(2, 20, 2, 64, -6, 6, g)
    q = torch.randn(2, 2, 4, 64, generator=g).bfloat16()
    (kq, ks), (vq, vs) = R.quant_kv8(k), R.quant_kv8(v)
    out, lse = R.attn_decode_q8(q, kq, ks, vq, vs, True, 0.125)
    o2, l2 = R.attention(q.float(), R.dequant_kv8(kq, ks), R.dequant_kv8(vq, vs), True, 0.125)
    assert torch.equal(out, o2) and torch.equal(lse, l2)


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny", "gpt_tiny"])
def test_cached_generation_with_fp8_cache(name):
    m = _model(name)
    torch.manual_seed(0)
    ids = torch.randint(0, m.c.vocab_size, (2, 6))
    st8, st16 = GenerationStats(), GenerationStats()
    out8 = generate(m, ids, 5, greedy=True, stats=st8, kv_cache="fp8")
    out16 = generate(m, ids, 5, greedy=True, stats=st16)
    assert out8.shape == out16.shape == (2, 11) and torch.equal(out8[:, :6], ids)
    assert (st8.cached, st8.prompt_tokens, st8.new_tokens) == (st16.cached, st16.prompt_tokens, st16.new_tokens) \
        == (True, 12, 10)
    # the model's own generate passes the argument through; "bf16" is the default cache
    kw = {"greedy": True}
    assert torch.equal(m.generate(ids, 5, kv_cache="fp8", **kw), out8)
    assert torch.equal(m.generate(ids, 5, kv_cache="bf16", **kw), out16)
    with pytest.raises(ValueError):
        m.new_cache(2, 8, kv_cache="int4")


def _teacher_forced(m, ids, kv_cache):
    B, T = ids.shape
    cache = m.new_cache(B, T, kv_cache=kv_cache)
    with torch.no_grad():
        lg = [m.step(ids[:, t:t + 1], cache, t) for t in range(T)]
    return torch.stack(lg, 1), cache


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny", "gpt_tiny"])
def test_layer0_cache_is_quantised_bf16_cache(name):
    m = _model(name)
    torch.manual_seed(0)
    ids = torch.randint(0, m.c.vocab_size, (2, 16))
    _, c8 = _teacher_forced(m, ids, "fp8")
    _, c16 = _teacher_forced(m, ids, None)
    assert c8.quant == "fp8" and c16.quant is None
    k, v = c16.dequantized(0, 16)
    k8, v8 = c8.dequantized(0, 16)
    assert k8.dtype == k.dtype
    assert torch.equal(k8, R.dequant_kv8(*R.quant_kv8(k), k.dtype))
    assert torch.equal(v8, R.dequant_kv8(*R.quant_kv8(v), v.dtype))
    assert c8[0].ks.unique().numel() > 1 or c8[0].vs.unique().numel() > 1
    # a multi-token prefill writes the same rows as token-by-token steps (layer 0 sees only embeddings)
    cp = m.new_cache(2, 16, kv_cache="fp8")
    with torch.no_grad():
        m.step(ids, cp, 0)
    assert torch.equal(cp[0].kq.view(torch.uint8), c8[0].kq.view(torch.uint8))
    assert torch.equal(cp[0].vs, c8[0].vs)


def test_nbytes_counts_data_and_scales():
    L, B, Tmax, Hkv, hd = 3, 2, 40, 2, 64
    bf = KVCache(L, B, Tmax, Hkv, hd, dtype=torch.bfloat16)
    f8 = KVCache(L, B, Tmax, Hkv, hd, dtype=torch.bfloat16, quant="fp8")
    assert bf.nbytes() == 2 * L * B * Tmax * Hkv * hd * 2
    assert f8.nbytes() == bf.nbytes() // 2 + 2 * L * B * Tmax * Hkv
    lay = f8[0]
    assert lay.kq.dtype == torch.float8_e4m3fn and lay.kq.shape == (B, Tmax, Hkv, hd)
    assert lay.ks.dtype == torch.uint8 and lay.ks.shape == (B, Hkv, Tmax) and lay.ks.is_contiguous()
    assert KVCache(L, B, Tmax, Hkv, hd, quant=None).quant is None
    with pytest.raises(ValueError):
        KVCache(L, B, Tmax, Hkv, hd, quant="fp4")
    with pytest.raises(ValueError):      # overflow is refused, as for the bf16 cache
        f8.write(0, torch.zeros(B, 2, Hkv, hd), torch.zeros(B, 2, Hkv, hd), Tmax - 1)


def test_deepseek_latent_cache_refuses_fp8():
    from solvingpapers_amd.models import deepseekv3
    m = deepseekv3.DeepSeekV3(deepseekv3.config("dsv3_tiny"), seed=1).eval()
    with pytest.raises(NotImplementedError, match="latent"):
        m.new_cache(1, 8, kv_cache="fp8")
    with pytest.raises(NotImplementedError, match="latent"):
        m.generate(torch.zeros(1, 4, dtype=torch.long), 2, kv_cache="fp8")
    assert len(m.new_cache(1, 8, kv_cache="bf16")) == len(m.new_cache(1, 8))


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_print_e_ref(name, capsys):
    """E_ref: rel L2 of the fp8-cache teacher-forced logits against the bf16-cache ones on the CPU
    oracle path (model(seed=1), torch.manual_seed(0), ids (2, 16)). Recorded in
    profiles/fp8_kv_cache.txt; tests/test_kv8_gpu.py bounds the GPU figure by 2 x the bf16 value."""
    for dtype in (torch.float32, torch.bfloat16):
        m = _model(name, dtype)
        torch.manual_seed(0)
        ids = torch.randint(0, m.c.vocab_size, (2, 16))
        l8, _ = _teacher_forced(m, ids, "fp8")
        l16, _ = _teacher_forced(m, ids, None)
        e = rel(l8, l16)
        with capsys.disabled():
            print(f"\nE_ref {name} {str(dtype).split('.')[-1]}: {e:.4e}")
        assert torch.isfinite(l8).all() and 0 < e < 0.1
