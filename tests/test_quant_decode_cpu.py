"""fp8 weight-only decode on the CPU (solvingpapers_amd/infer/quant.py): which parameters
quantize_decode_weights gives an image, that the images are ops.moe's CPU formula bit for bit,
and that a quantised model's token-by-token decode equals the full forward of a copy holding the
dequantised weights (the oracle product behind linear / grouped_linear)."""
import pytest
import torch

from solvingpapers_amd.infer import clear_decode_weights, quantize_decode_weights
from solvingpapers_amd.models import deepseekv3, llama3
from solvingpapers_amd.ops import moe as M, reference as R


def _llama(**kw):
    return llama3.Llama3(llama3.config("llama3_tiny", **kw), seed=1).eval()


def _dsv3():
    return deepseekv3.DeepSeekV3(deepseekv3.config("dsv3_tiny"), seed=1).eval()


def _eligible(p):
    return p.dim() in (2, 3) and p.shape[-1] % 128 == 0 and p.shape[-2] % 128 == 0


def _teacher_forced(m, ids):
    with torch.no_grad():
        cache = m.new_cache(ids.shape[0], ids.shape[1])
        return torch.stack([m.step(ids[:, t:t + 1], cache, t) for t in range(ids.shape[1])], 1)


def _fp8_exact_lookup_table_(m):
    """The token table is also READ BY INDEX, and a lookup takes the master rows (a few rows per
    step: nothing to save there), while the dequantised copy below looks its rows up in the
    dequantised table. So the table alone starts from fp8-representable values (quantising is
    idempotent: they are their own image); every product still runs on weights that differ from
    their images."""
    p = getattr(m, "tok_embeddings", None)
    p = p if p is not None else m.embed
    with torch.no_grad():
        wq, _, s, _ = M.quant_weight_fp8_blk_uncached(p.detach()[None])
        p.copy_(R.dequant_w8(wq[0], s[0]))
        again = M.quant_weight_fp8_blk_uncached(p.detach()[None])
        assert torch.equal(R.dequant_w8(again[0][0], again[2][0]).to(p.dtype), p)


def _dequantised_copy(make, model, report):
    ref = make()
    ref.load_state_dict(model.state_dict())
    params = dict(model.named_parameters())
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name in report["quantized"]:
                p.copy_(R.dequant_w8(*params[name]._spa_w8[:2]))
    return ref


@pytest.mark.parametrize("make", [_llama, _dsv3])
def test_report_and_images(make):
    m = make()
    keys = list(m.state_dict().keys())
    rep = quantize_decode_weights(m)
    params = dict(m.named_parameters())
    assert set(rep["quantized"]) | set(rep["bf16"]) == set(params) and not set(rep["quantized"]) & set(rep["bf16"])
    assert sorted(rep["quantized"]) == sorted(n for n, p in params.items() if _eligible(p))
    assert all(params[n].dim() != 1 for n in rep["quantized"])
    assert all(n in rep["bf16"] and rep["bf16"][n] for n, p in params.items() if p.dim() == 1)
    if make is _llama:
        for n in ("output", "layers.0.wqkv", "layers.0.wo", "layers.1.w13", "layers.1.w2"):
            assert n in rep["quantized"]
    else:
        experts = [n for n, p in params.items() if p.dim() == 3]
        assert experts and all(n in rep["quantized"] for n in experts)
        assert "layers.1.ffn.gate" in rep["bf16"] and "layers.0.attn.wdkv" in rep["bf16"]
    nbytes = 0
    for n in rep["quantized"]:
        p = params[n]
        wq, s, version, ptr, name = p._spa_w8
        want = M.quant_weight_fp8_blk(p.detach() if p.dim() == 3 else p.detach()[None])   # ops.moe's CPU formula
        wq_ref, s_ref = (want[0], want[2]) if p.dim() == 3 else (want[0][0], want[2][0])
        assert wq.dtype == torch.float8_e4m3fn and s.dtype == torch.uint8
        assert wq.shape == p.shape and s.shape == (*p.shape[:-2], p.shape[-2] // 128, p.shape[-1] // 128)
        assert torch.equal(wq.view(torch.uint8), wq_ref.view(torch.uint8)) and torch.equal(s, s_ref)
        assert (version, ptr, name) == (p._version, p.data_ptr(), n)
        nbytes += wq.numel() + s.numel()
    assert rep["image_bytes"] == nbytes
    assert list(m.state_dict().keys()) == keys
    assert quantize_decode_weights(m, skip=("layers.0.*",))["bf16"].get("layers.0.ffn_norm") is not None
    assert not any(hasattr(p, "_spa_w8") for n, p in params.items() if n.startswith("layers.0."))
    clear_decode_weights(m)
    assert not any(hasattr(p, "_spa_w8") for p in m.parameters())


@pytest.mark.parametrize("make", [_llama, _dsv3])
def test_cpu_decode_matches_dequantised_full_forward(make):
    """tests/test_infer_cpu.py asks cached decoding to pick the full forward's greedy token at every
    position; here teacher-forced, plus the logits themselves (fp32, same weights, another summation
    order: 1e-4 is two orders above what that leaves)."""
    torch.manual_seed(0)
    m = make()
    _fp8_exact_lookup_table_(m)
    ids = torch.randint(0, m.c.vocab_size, (2, 16))
    with torch.no_grad():
        master = m(ids)
    rep = quantize_decode_weights(m)
    ref = _dequantised_copy(make, m, rep)
    with torch.no_grad():
        full = ref(ids)
    got = _teacher_forced(m, ids)
    err = ((got - full).norm() / full.norm()).item()
    assert torch.equal(got.argmax(-1), full.argmax(-1))
    assert err < 1e-4, err
    # the decode really ran on the images: the master's logits are a quantisation error away
    assert ((got - master).norm() / master.norm()).item() > 1e-3
    clear_decode_weights(m)
    assert ((_teacher_forced(m, ids) - master).norm() / master.norm()).item() < 1e-4


def test_stale_image_raises_and_clear_restores():
    from solvingpapers_amd.ops.linear import linear
    m = _llama()
    w = m.layers[0].wo
    x = torch.randn(2, 1, w.shape[1])
    with torch.no_grad():
        y0 = linear(x, w)
    quantize_decode_weights(m)
    with torch.no_grad():
        y8 = linear(x, w)
        assert torch.equal(y8.view(2, -1), R.gemv_w8(x.view(2, -1), *w._spa_w8[:2]))
        assert not torch.equal(y8, y0)
        # more rows than a decode step, or autograd on the weight: the master weights
        x8 = torch.randn(8, w.shape[1])
        assert torch.allclose(linear(x8, w), x8 @ w.t(), rtol=1e-4, atol=1e-5)
    assert torch.allclose(linear(x, w), x @ w.t(), rtol=1e-4, atol=1e-5)
    with torch.no_grad():
        w.add_(1e-3)
        with pytest.raises(RuntimeError, match=r"layers\.0\.wo.*quantize_decode_weights"):
            linear(x, w)
        with pytest.raises(RuntimeError, match=r"layers\.0\.wo"):
            m.step(torch.zeros(1, 1, dtype=torch.long), m.new_cache(1, 4), 0)
        quantize_decode_weights(m)                     # requantise: valid again
        linear(x, w)
        w.data = w.data.clone()                        # moved storage is stale too
        with pytest.raises(RuntimeError, match="stale"):
            linear(x, w)
        clear_decode_weights(m)
        assert torch.allclose(linear(x, w), x @ w.t(), rtol=1e-4, atol=1e-5)


def test_model_without_eligible_parameter_is_untouched():
    torch.manual_seed(0)
    make = lambda: _llama(vocab_size=160, dim=96, n_heads=4, n_kv_heads=2, ffn_hidden=160, max_seq_len=32)  # noqa: E731
    m = make()
    ids = torch.randint(0, 160, (2, 8))
    before = _teacher_forced(m, ids)
    rep = quantize_decode_weights(m)
    assert rep["quantized"] == [] and rep["image_bytes"] == 0
    assert set(rep["bf16"]) == {n for n, _ in m.named_parameters()}
    assert not any(hasattr(p, "_spa_w8") for p in m.parameters())
    assert torch.equal(_teacher_forced(m, ids), before)
