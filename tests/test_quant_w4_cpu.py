"""MXFP4 weight-only decode on the CPU: the quantisation rule (ops/reference.py quant_mxfp4) against
a brute-force fp64 nearest-code search, its byte layout and idempotence, what
quantize_decode_weights(fmt="mxfp4") attaches and reports, and a quantised model's token-by-token
decode against the full forward of a copy holding the dequantised weights."""
import pytest
import torch

from mxfp4_cases import brute_force_mxfp4, rule_cases
from solvingpapers_amd.infer import clear_decode_weights, quantize_decode_weights
from solvingpapers_amd.models import deepseekv3, llama3
from solvingpapers_amd.ops import reference as R


def _llama(**kw):
    return llama3.Llama3(llama3.config("llama3_tiny", **kw), seed=1).eval()


def _dsv3():
    return deepseekv3.DeepSeekV3(deepseekv3.config("dsv3_tiny"), seed=1).eval()


def _eligible(p):
    return p.dim() in (2, 3) and p.shape[-1] % 128 == 0 and p.shape[-2] % 128 == 0


@pytest.mark.parametrize("name", list(rule_cases()))
def test_quant_mxfp4_is_the_brute_force_nearest_code(name):
    W = rule_cases()[name]
    wq, s = R.quant_mxfp4(W)
    wq_ref, s_ref = brute_force_mxfp4(W)
    assert wq.dtype == torch.uint8 and s.dtype == torch.uint8
    assert wq.shape == (W.shape[0], W.shape[1] // 2) and s.shape == (W.shape[0], W.shape[1] // 32)
    assert torch.equal(s, s_ref), name
    assert torch.equal(wq, wq_ref), name
    d = R.dequant_w4(wq, s)
    assert torch.equal(d.to(torch.bfloat16).float(), d)          # every value exact in bf16


def test_rule_cases_cover_what_they_claim():
    c = rule_cases()
    assert len(torch.unique(R.quant_mxfp4(c["randn_pow2"])[1])) > 8        # many different scales
    # tie points 0.25 .75 1.25 1.75 2.5 3.5 5 -> 0 1 1 2 2 4 4, at every scale, both signs
    wq, s = R.quant_mxfp4(c["ties"])
    d = R.dequant_w4(wq, s) / torch.exp2(s.float() - 127).repeat_interleave(32, -1)
    want = torch.tensor([0, 1, 1, 2, 2, 4, 4.0])
    assert torch.equal(d[:, :7], want.expand(d.shape[0], 7))
    assert torch.equal(d[:, 8:15], -want.expand(d.shape[0], 7))
    wq, s = R.quant_mxfp4(c["zeros_and_negative_zero"])
    assert torch.equal(s, torch.full_like(s, 127))
    assert wq[0].eq(0).all() and wq[1, 0] == 0x08 and wq[1, 1] == 0x80 and wq[1, 2:].eq(0).all()
    # amax exactly 6 * 2^e keeps e; one bf16 ulp above moves to e + 1
    s_at, s_above = R.quant_mxfp4(c["amax_6"])[1], R.quant_mxfp4(c["amax_6_plus_ulp"])[1]
    assert torch.equal(s_above.int(), s_at.int() + 1)
    assert R.quant_mxfp4(c["amax_6"])[0][:, 0].eq(0x07).all()              # 6 * 2^e is code 7 ...
    assert R.quant_mxfp4(c["amax_6_plus_ulp"])[0][:, 0].eq(0x05).all()     # ... 3.01 * 2^(e+1) is code 5 (3)


def test_quant_mxfp4_is_idempotent():
    """The image of a dequantised image is the same image. Two blocks keep their VALUES but not their bytes
    the first time round, by the rule itself: a block whose amax rounded down to 3 * 2^e is re-scaled to
    6 * 2^(e - 1) (the smallest e with amax <= 6 * 2^e, every code's value doubling exactly), and a block
    that rounded to all zeros takes the zero block's scale. So: the dequantised values are a fixed point
    at once, bitwise; blocks whose largest magnitude is 4 or 6 keep their bytes at once; and every image of
    a dequantised image is a fixed point in its bytes."""
    for name, W in rule_cases().items():
        wq, s = R.quant_mxfp4(W)
        d = R.dequant_w4(wq, s)
        wq2, s2 = R.quant_mxfp4(d.to(torch.bfloat16))
        d2 = R.dequant_w4(wq2, s2)
        assert torch.equal(d2.view(torch.int32), d.view(torch.int32)), name       # signed zeros included
        top = (d.reshape(*s.shape, 32).abs() / torch.exp2(s.float() - 127)[..., None]).amax(-1)
        keep = top >= 4
        assert keep.any() or name in ("zeros_and_negative_zero", "amax_6_plus_ulp")   # 3.0156 rounds to 3
        assert torch.equal(s2[keep], s[keep]), name
        assert torch.equal(wq2.reshape(*s.shape, 16)[keep], wq.reshape(*s.shape, 16)[keep]), name
        wq3, s3 = R.quant_mxfp4(d2.to(torch.bfloat16))
        assert torch.equal(wq3, wq2) and torch.equal(s3, s2), name


def test_byte_layout():
    W = torch.zeros(2, 64, dtype=torch.bfloat16)
    W[0, 0], W[0, 1], W[0, 2], W[0, 5] = 6.0, -0.5, 1.5, -4.0    # block amax 6: scale 2^0
    W[1, 32], W[1, 33], W[1, 63] = -12.0, 2.0, 3.0               # block amax 12: scale 2^1
    wq, s = R.quant_mxfp4(W)
    assert s.tolist() == [[127, 127], [127, 128]]
    assert wq[0, 0] == (0x7 | 0x9 << 4)       # k = 0 in the low nibble, k = 1 (sign in bit 3) in the high
    assert wq[0, 1] == 0x3 and wq[0, 2] == 0xe << 4
    assert wq[1, 16] == (0xf | 0x2 << 4)      # -12 / 2 = -6 -> 0xf; 2 / 2 = 1 -> 0x2
    assert wq[1, 31] == 0x3 << 4              # 3 / 2 = 1.5 -> 0x3
    d = R.dequant_w4(wq, s)
    assert d.shape == (2, 64) and d.dtype == torch.float32
    assert d[0, :6].tolist() == [6.0, -0.5, 1.5, 0.0, 0.0, -4.0] and d[1, 32:34].tolist() == [-12.0, 2.0]
    assert d[1, 63] == 3.0


@pytest.mark.parametrize("make", [_llama, _dsv3])
def test_report_and_images(make):
    m = make()
    keys = list(m.state_dict().keys())
    rep8 = quantize_decode_weights(m)                               # the default: fp8, as before
    assert rep8["format"] == "fp8-e4m3 128x128 E8M0"
    params = dict(m.named_parameters())
    assert all(hasattr(params[n], "_spa_w8") for n in rep8["quantized"])
    assert not any(hasattr(p, "_spa_w4") for p in params.values())
    assert rep8["image_bytes"] == sum(params[n].numel() + params[n].numel() // 16384 for n in rep8["quantized"])
    rep = quantize_decode_weights(m, fmt="mxfp4")                   # switching formats swaps the attribute
    assert rep["format"] == "mxfp4-e2m1 1x32 E8M0"
    assert rep["quantized"] == rep8["quantized"] and rep["bf16"] == rep8["bf16"]
    assert sorted(rep["quantized"]) == sorted(n for n, p in params.items() if _eligible(p))
    assert not any(hasattr(p, "_spa_w8") for p in params.values())
    nbytes = 0
    for n in rep["quantized"]:
        p = params[n]
        wq, s, version, ptr, name = p._spa_w4
        wq_ref, s_ref = R.quant_mxfp4(p.detach())
        assert wq.dtype == torch.uint8 and s.dtype == torch.uint8
        assert wq.shape == (*p.shape[:-1], p.shape[-1] // 2) and s.shape == (*p.shape[:-1], p.shape[-1] // 32)
        assert torch.equal(wq, wq_ref) and torch.equal(s, s_ref)
        assert (version, ptr, name) == (p._version, p.data_ptr(), n)
        N, K = p.shape[-2:]
        nbytes += (p.numel() // (N * K)) * (N * K // 2 + N * K // 32)
    assert rep["image_bytes"] == nbytes
    assert list(m.state_dict().keys()) == keys
    assert quantize_decode_weights(m, skip=("layers.0.*",), fmt="mxfp4")["bf16"].get("layers.0.ffn_norm") is not None
    assert not any(hasattr(p, "_spa_w4") for n, p in params.items() if n.startswith("layers.0."))
    quantize_decode_weights(m)                                      # and back
    assert all(hasattr(params[n], "_spa_w8") for n in rep8["quantized"])
    assert not any(hasattr(p, "_spa_w4") for p in params.values())
    quantize_decode_weights(m, skip=("layers.0.*",), fmt="mxfp4")
    clear_decode_weights(m)
    assert not any(hasattr(p, "_spa_w8") or hasattr(p, "_spa_w4") for p in m.parameters())
    with pytest.raises(ValueError):
        quantize_decode_weights(m, fmt="int4")
    assert not any(hasattr(p, "_spa_w8") or hasattr(p, "_spa_w4") for p in m.parameters())


def test_stale_image_raises_and_clear_restores():
    from solvingpapers_amd.ops.linear import linear
    m = _llama()
    w = m.layers[0].wo
    x = torch.randn(2, 1, w.shape[1])
    with torch.no_grad():
        y0 = linear(x, w)
    quantize_decode_weights(m, fmt="mxfp4")
    with torch.no_grad():
        y4 = linear(x, w)
        assert torch.equal(y4.view(2, -1), R.gemv_w4(x.view(2, -1), *w._spa_w4[:2]))
        assert not torch.equal(y4, y0)
        x8 = torch.randn(8, w.shape[1])                  # more rows than a decode step: the master weights
        assert torch.allclose(linear(x8, w), x8 @ w.t(), rtol=1e-4, atol=1e-5)
    assert torch.allclose(linear(x, w), x @ w.t(), rtol=1e-4, atol=1e-5)   # autograd on the weight: the masters
    with torch.no_grad():
        w.add_(1e-3)
        with pytest.raises(RuntimeError, match=r"layers\.0\.wo.*quantize_decode_weights"):
            linear(x, w)
        with pytest.raises(RuntimeError, match=r"layers\.0\.wo"):
            m.step(torch.zeros(1, 1, dtype=torch.long), m.new_cache(1, 4), 0)
        quantize_decode_weights(m, fmt="mxfp4")          # requantise: valid again
        linear(x, w)
        w.data = w.data.clone()                          # moved storage is stale too
        with pytest.raises(RuntimeError, match="stale"):
            linear(x, w)
        clear_decode_weights(m)
        assert torch.allclose(linear(x, w), x @ w.t(), rtol=1e-4, atol=1e-5)


def _teacher_forced(m, ids):
    with torch.no_grad():
        cache = m.new_cache(ids.shape[0], ids.shape[1])
        return torch.stack([m.step(ids[:, t:t + 1], cache, t) for t in range(ids.shape[1])], 1)


def _mxfp4_exact_lookup_table_(m):
    """The token table is also read by index, from the master rows, while the dequantised copy looks
    its rows up in the dequantised table: so the table alone starts from values that are their own
    image (tests/test_quant_decode_cpu.py does the same for fp8)."""
    p = getattr(m, "tok_embeddings", None)
    p = p if p is not None else m.embed
    with torch.no_grad():
        p.copy_(R.dequant_w4(*R.quant_mxfp4(p.detach())))
        assert torch.equal(R.dequant_w4(*R.quant_mxfp4(p.detach())).to(p.dtype), p)


def _dequantised_copy(make, model, report):
    ref = make()
    ref.load_state_dict(model.state_dict())
    params = dict(model.named_parameters())
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name in report["quantized"]:
                p.copy_(R.dequant_w4(*params[name]._spa_w4[:2]))
    return ref


@pytest.mark.parametrize("make", [_llama, _dsv3])
def test_cpu_decode_matches_dequantised_full_forward(make):
    """16 teacher-forced steps on the mxfp4 images against the full forward of a copy holding the
    dequantised weights: fp32, the same weights, another summation order -- the 1e-4 of
    tests/test_quant_decode_cpu.py for the same comparison."""
    torch.manual_seed(0)
    m = make()
    _mxfp4_exact_lookup_table_(m)
    ids = torch.randint(0, m.c.vocab_size, (2, 16))
    with torch.no_grad():
        master = m(ids)
    rep = quantize_decode_weights(m, fmt="mxfp4")
    if make is _dsv3:
        experts = [n for n, p in m.named_parameters() if p.dim() == 3]
        assert experts and all(n in rep["quantized"] for n in experts)       # the grouped route is covered
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
