"""fp8 KV cache on the GPU: the quantising cache writers (csrc/kernels/rope.hip) bitwise against the
torch formula, attn_decode_q8 (csrc/kernels/decode.hip) against the oracle on the same dequantised
rows, the helpers' routing, and LLaMA3 / Gemma decoding from an fp8 cache, eager and HIP-graph."""
import math

import pytest
import torch

from solvingpapers_amd.ops import _ext, reference as R
from solvingpapers_amd.ops.attention import KV8, flash_attention, kv_cache_attend, kv_cache_write
from solvingpapers_amd.ops.rope import RopeCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

# E_ref: fp8-cache vs bf16-cache teacher-forced logits (rel L2) on the CPU oracle path in bf16, as
# printed by tests/test_kv8_cpu.py::test_print_e_ref and recorded in profiles/fp8_kv_cache.txt
E_REF = {"llama3_tiny": 3.5657e-2, "gemma_tiny": 7.7602e-3}


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def u8(t):
    return t.view(torch.uint8)


def kv_rows(shape, lo, hi, gen):
    """randn * 2^e with e random in [lo, hi] per head row (last dim): many distinct row scales."""
    e = torch.randint(lo, hi + 1, (*shape[:-1], 1), device=DEV, generator=gen)
    return (torch.randn(*shape, device=DEV, generator=gen) * torch.exp2(e.float())).to(BF)


def packed_qkv(B, T, H, Hkv, hd, gen):
    """[B, T, H + 2 Hkv, hd] with K rows scaled by 2^[-3, 0] and V rows by 2^[-6, 6]."""
    x = torch.randn(B, T, H + 2 * Hkv, hd, device=DEV, generator=gen).to(BF)
    x[:, :, H:H + Hkv] = kv_rows((B, T, Hkv, hd), -3, 0, gen)
    x[:, :, H + Hkv:] = kv_rows((B, T, Hkv, hd), -6, 6, gen)
    return x


def canary_cache(B, Tmax, Hkv, hd):
    c = KV8.zeros(B, Tmax, Hkv, hd, device=DEV, dtype=BF)
    for t in (c.kq, c.vq):
        u8(t).fill_(0x5A)
    for t in (c.ks, c.vs):
        t.fill_(0xA5)
    return c


def assert_rows(c, kref, vref, pos, T):
    """cache rows [pos, pos+T) == quant_kv8 of the bf16 rows, everything else still canary."""
    for q, s, ref in ((c.kq, c.ks, kref), (c.vq, c.vs, vref)):
        rq, rs = R.quant_kv8(ref)
        assert rs.unique().numel() > 1
        assert torch.equal(u8(q)[:, pos:pos + T], u8(rq))
        assert torch.equal(s[:, :, pos:pos + T], rs)
        keep = torch.ones(q.shape[1], dtype=torch.bool, device=DEV)
        keep[pos:pos + T] = False
        assert (u8(q)[:, keep] == 0x5A).all() and (s[:, :, keep] == 0xA5).all()


@pytest.mark.parametrize("hd", [64, 128, 256])
@pytest.mark.parametrize("T,pos", [(1, 0), (1, 6), (5, 0), (5, 6)])
def test_kv_quant_write_bitwise(hd, T, pos):
    B, H, Hkv, Tmax = 2, 4, 2, 12
    g = torch.Generator(device=DEV).manual_seed(hd + 10 * T + pos)
    x = packed_qkv(B, T, H, Hkv, hd, g)
    k, v = x[:, :, H:H + Hkv], x[:, :, H + Hkv:]
    c = canary_cache(B, Tmax, Hkv, hd)
    _ext.ops().kv_quant_write_(k, v, c.kq, c.ks, c.vq, c.vs, pos)
    assert_rows(c, k, v, pos, T)
    # the write helper takes the same kernel
    c2 = canary_cache(B, Tmax, Hkv, hd)
    kv_cache_write(c2, k, v, pos)
    assert torch.equal(u8(c2.kq), u8(c.kq)) and torch.equal(c2.vs, c.vs)


@pytest.mark.parametrize("mode,hd", [(0, 128), (1, 64), (0, 64), (1, 256)])
def test_rope_kv_write_q8_bitwise(mode, hd):
    B, T, H, Hkv, Tmax = 2, 1, 4, 2, 12
    g = torch.Generator(device=DEV).manual_seed(mode + hd)
    x = packed_qkv(B, T, H, Hkv, hd, g)
    cos, sin = RopeCache.get(Tmax, hd, 500000.0, DEV)
    for row in (0, 7, Tmax):
        index = torch.tensor([row], device=DEV)
        posn = torch.full((B, T), min(row, Tmax - 1), device=DEV, dtype=torch.int32)
        xa, xb = x.clone(), x.clone()
        kc = torch.zeros(B, Tmax, Hkv, hd, device=DEV, dtype=BF)
        vc = torch.zeros_like(kc)
        _ext.ops().rope_kv_write_(xa, cos, sin, posn, index, kc, vc, H, Hkv, mode)
        c = canary_cache(B, Tmax, Hkv, hd)
        _ext.ops().rope_kv_write_q8_(xb, cos, sin, posn, index, c.kq, c.ks, c.vq, c.vs, H, Hkv, mode)
        assert torch.equal(xa[:, :, :H], xb[:, :, :H])        # q heads rotated in place, bitwise
        assert not torch.equal(xb[:, :, :H], x[:, :, :H]) or row == 0
        assert torch.equal(xb[:, :, H:], x[:, :, H:])         # k / v heads of the buffer untouched
        if row == Tmax:                                       # past the cache end: nothing written
            for q, s in ((c.kq, c.ks), (c.vq, c.vs)):
                assert (u8(q) == 0x5A).all() and (s == 0xA5).all()
        else:
            assert_rows(c, kc[:, row:row + T], vc[:, row:row + T], row, T)


def quant_cache(k, v, pad=37):
    """KV8 views [:, :Tk] of a longer cache holding quant_kv8(k), quant_kv8(v)."""
    B, Tk, Hkv, hd = k.shape
    full = canary_cache(B, Tk + pad, Hkv, hd)
    for x, q, s in ((k, full.kq, full.ks), (v, full.vq, full.vs)):
        xq, xs = R.quant_kv8(x)
        assert xs.unique().numel() > 1 or Tk == 1
        u8(q)[:, :Tk] = u8(xq)
        s[:, :, :Tk] = xs
    return full


CASES = [
    # B, Tq, Tk, H, Hkv, hd, nsplit
    (1, 1, 300, 8, 2, 128, 0),       # R = 4, ragged last batch
    (2, 4, 77, 8, 2, 64, 0),         # R = 16, causal rows inside the cache
    (1, 1, 200, 16, 1, 256, 0),      # MQA, R = 16
    (2, 2, 50, 4, 4, 128, 1),        # single split
    (1, 1, 1, 4, 2, 64, 0),          # first token
    (2, 3, 130, 6, 3, 128, 7),       # R = 8, odd split count
]


@pytest.mark.parametrize("B,Tq,Tk,H,Hkv,hd,ns", CASES)
def test_attn_decode_q8_matches_oracle(B, Tq, Tk, H, Hkv, hd, ns):
    g = torch.Generator(device=DEV).manual_seed(0)
    q = torch.randn(B, Tq, H, hd, device=DEV, generator=g).to(BF)
    c = quant_cache(kv_rows((B, Tk, Hkv, hd), -3, 0, g), kv_rows((B, Tk, Hkv, hd), -6, 6, g))
    kq, ks, vq, vs = c.kq[:, :Tk], c.ks[:, :, :Tk], c.vq[:, :Tk], c.vs[:, :, :Tk]
    sc = 1 / math.sqrt(hd)
    out, lse = _ext.ops().attn_decode_q8(q, kq, ks, vq, vs, sc, True, ns)
    of, lf = R.attn_decode_q8(q, kq, ks, vq, vs, True, sc)
    print(f"rel L2 {rel(out, of):.3e}  max |dlse| {(lse - lf).abs().max().item():.3e}")
    assert rel(out, of) < 1e-2, rel(out, of)
    assert (lse - lf).abs().max().item() < 1e-2
    # the attend helper routes here
    assert torch.equal(kv_cache_attend(q, c, Tk, causal=True, nsplit=ns), out)


def test_attn_decode_q8_device_kv_len_twice():
    """A device kv_len shorter than the buffers leaves trailing splits empty; two launches back to back."""
    B, Tk, H, Hkv, hd, n = 2, 700, 8, 2, 128, 300
    g = torch.Generator(device=DEV).manual_seed(2)
    q = torch.randn(B, 1, H, hd, device=DEV, generator=g).to(BF)
    c = quant_cache(kv_rows((B, Tk, Hkv, hd), -3, 0, g), kv_rows((B, Tk, Hkv, hd), -6, 6, g), pad=0)
    kv_len = torch.tensor([n], device=DEV, dtype=torch.int32)
    sc = 1 / math.sqrt(hd)
    o1, l1 = _ext.ops().attn_decode_q8(q, c.kq, c.ks, c.vq, c.vs, sc, True, 0, kv_len)
    o2, l2 = _ext.ops().attn_decode_q8(q, c.kq, c.ks, c.vq, c.vs, sc, True, 9, kv_len)
    of, lf = R.attn_decode_q8(q, c.kq[:, :n], c.ks[:, :, :n], c.vq[:, :n], c.vs[:, :, :n], True, sc)
    for o, l in ((o1, l1), (o2, l2)):
        assert rel(o, of) < 1e-2, rel(o, of)
        assert (l - lf).abs().max().item() < 1e-2
    assert torch.equal(kv_cache_attend(q, c, causal=True, kv_len=kv_len), o1)


def test_bad_calls_raise():
    B, Tk, H, Hkv, hd = 1, 40, 8, 2, 128
    g = torch.Generator(device=DEV).manual_seed(3)
    q = torch.randn(B, 1, H, hd, device=DEV, generator=g).to(BF)
    k, v = kv_rows((B, Tk, Hkv, hd), -3, 0, g), kv_rows((B, Tk, Hkv, hd), -6, 6, g)
    c = quant_cache(k, v, pad=0)
    op = _ext.ops().attn_decode_q8
    sc = 1 / math.sqrt(hd)
    op(q, c.kq, c.ks, c.vq, c.vs, sc, True, 0)                                    # the good call
    with pytest.raises(RuntimeError):                                             # bf16 cache tensors
        op(q, k, c.ks, v, c.vs, sc, True, 0)
    with pytest.raises(RuntimeError):                                             # scales [B, Tk, Hkv]
        op(q, c.kq, c.ks.transpose(1, 2).contiguous(), c.vq, c.vs, sc, True, 0)
    with pytest.raises(RuntimeError):                                             # right shape, token-strided
        op(q, c.kq, c.ks.transpose(1, 2).contiguous().transpose(1, 2), c.vq, c.vs, sc, True, 0)
    with pytest.raises(RuntimeError):                                             # scales of another length
        op(q, c.kq, c.ks[:, :, :Tk - 1], c.vq, c.vs, sc, True, 0)
    with pytest.raises(RuntimeError):                                             # 5 tokens x 4 heads = 20 rows
        op(torch.randn(B, 5, H, hd, device=DEV).to(BF), c.kq, c.ks, c.vq, c.vs, sc, True, 0)
    c96 = KV8.zeros(B, Tk, Hkv, 96, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError):                                             # hd 96
        op(torch.randn(B, 1, H, 96, device=DEV).to(BF), c96.kq, c96.ks, c96.vq, c96.vs, sc, True, 0)
    with pytest.raises(RuntimeError):                                             # write past the cache end
        _ext.ops().kv_quant_write_(k[:, :2], v[:, :2], c.kq, c.ks, c.vq, c.vs, Tk - 1)
    with pytest.raises(ValueError):                                               # kv_len without the kernel
        kv_cache_attend(torch.randn(B, 8, H, hd, device=DEV).to(BF), c, causal=True,
                        kv_len=torch.tensor([Tk], device=DEV, dtype=torch.int32))


def test_attend_helper_falls_back_to_flash_on_dequantised_rows():
    B, Tq, Tk, H, Hkv, hd = 1, 8, 48, 8, 2, 128                                  # 8 x 4 = 32 rows > 16
    g = torch.Generator(device=DEV).manual_seed(4)
    q = torch.randn(B, Tq, H, hd, device=DEV, generator=g).to(BF)
    c = quant_cache(kv_rows((B, Tk, Hkv, hd), -3, 0, g), kv_rows((B, Tk, Hkv, hd), -6, 6, g))
    k, v = c.dequantized(Tk)
    assert k.dtype == BF and k.shape == (B, Tk, Hkv, hd)
    assert torch.equal(kv_cache_attend(q, c, Tk, causal=True), flash_attention(q, k, v, True))
    # a bf16 pair takes today's route
    assert torch.equal(kv_cache_attend(q, (k, v), Tk, causal=True), flash_attention(q, k, v, True))


# ------------------------------------------------------------------ models
def _model(name):
    if name == "llama3_tiny":
        from solvingpapers_amd.models import llama3
        return llama3.Llama3(llama3.config(name), device=DEV, dtype=BF, seed=1).eval()
    from solvingpapers_amd.models import gemma
    return gemma.Gemma(gemma.config(name), device=DEV, dtype=BF, seed=1).eval()


def _ids(m):
    torch.manual_seed(0)
    return torch.randint(0, m.c.vocab_size, (2, 16)).to(DEV)


def _eager(m, ids, kv_cache):
    cache = m.new_cache(2, 16, kv_cache=kv_cache)
    with torch.no_grad():
        lg = [m.step(ids[:, t:t + 1], cache, t) for t in range(16)]
    return torch.stack(lg, 1), cache


def _graph(m, ids, kv_cache):
    from solvingpapers_amd.infer import GraphDecoder
    dec = GraphDecoder(m, 2, 20, kv_cache=kv_cache)
    dec.state.set(0)
    lg = []
    for t in range(16):
        dec.ids.copy_(ids[:, t:t + 1])
        dec.graph.replay()
        lg.append(dec.logits.clone())
    return torch.stack(lg, 1), dec


def _check(name, l8, c8, l16, c16, path):
    k, v = c16[0]
    for q, s, ref in ((c8[0].kq, c8[0].ks, k), (c8[0].vq, c8[0].vs, v)):      # (a) layer 0, bitwise
        rq, rs = R.quant_kv8(ref[:, :16])
        assert torch.equal(u8(q)[:, :16], u8(rq)) and torch.equal(s[:, :, :16], rs)
    e = rel(l8, l16)                                                              # (b)
    print(f"{name} {path}: fp8-cache vs bf16-cache logits rel L2 {e:.4e} (E_ref {E_REF[name]:.4e})")
    assert torch.isfinite(l8).all()
    assert e < 2 * E_REF[name], (e, E_REF[name])


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_model_eager_steps_from_fp8_cache(name):
    m = _model(name)
    ids = _ids(m)
    l8, c8 = _eager(m, ids, "fp8")
    l16, c16 = _eager(m, ids, None)
    _check(name, l8, c8, l16, c16, "eager")


@pytest.mark.parametrize("name", ["llama3_tiny", "gemma_tiny"])
def test_model_graph_replays_from_fp8_cache(name):
    m = _model(name)
    ids = _ids(m)
    l8, d8 = _graph(m, ids, "fp8")
    l16, d16 = _graph(m, ids, None)
    _check(name, l8, d8.cache, l16, d16.cache, "graph")
    out = d8.generate(ids[:, :10], 6)                                             # (c)
    assert out.shape == (2, 16) and torch.equal(out[:, :10], ids[:, :10])
    first = m.generate(ids[:, :10], 1, greedy=True, kv_cache="fp8")
    assert torch.equal(out[:, 10], first[:, 10])
