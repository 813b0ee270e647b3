"""fp8 weight-only decode on the GPU: gemv_w8 / grouped_gemv_w8 (csrc/kernels/gemv.hip)
against the fp32 oracle on the dequantised image, their routing from linear / grouped_linear,
and quantised models decoding token by token against the full forward of a copy that holds the
dequantised weights.

Test weights carry a different power-of-two magnitude in every 128 x 128 block, so every block
gets its own scale and a wrong scale index cannot pass (with plain randn all scales are equal)."""
import pytest
import torch

from solvingpapers_amd.infer import GraphDecoder, clear_decode_weights, quantize_decode_weights
from solvingpapers_amd.ops import _ext, reference as R
from solvingpapers_amd.ops.moe import quant_weight_fp8_blk_uncached

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def block_weights(shape, seed):
    """randn * 2^e with e random in [-6, 6] per 128 x 128 block, bf16 on the device"""
    g = torch.Generator().manual_seed(seed)
    *lead, N, K = shape
    e = torch.randint(-6, 7, (*lead, N // 128, 1, K // 128, 1), generator=g).float()
    w = torch.randn(*lead, N // 128, 128, K // 128, 128, generator=g) * torch.exp2(e)
    return w.view(*shape).to(DEV, torch.bfloat16)


def image(w):
    wq, _, s, _ = quant_weight_fp8_blk_uncached(w if w.dim() == 3 else w[None])
    return (wq, s) if w.dim() == 3 else (wq[0], s[0])


@pytest.mark.parametrize("M,N,K", [
    (1, 128, 128),        # one block, 8 live lanes
    (3, 384, 1152),       # one full 1 KB pass plus a 128 tail, several scale rows
    (4, 256, 5248),       # unrolled main loop, single-pass remainder and a partial pass
    (2, 8192, 256),       # the RW = 4 path
    (1, 4096, 4096),      # a real shape (LLaMA3-8B o-proj)
])
def test_gemv_w8_matches_fp32_oracle(M, N, K):
    wq, s = image(block_weights((N, K), 0))
    assert len(torch.unique(s)) > 1 or s.numel() == 1
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, generator=torch.Generator(DEV).manual_seed(1))
    y = _ext.ops().gemv_w8(x, wq, s)
    ref = R.gemv_w8(x, wq, s)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    print(f"gemv_w8 M={M} N={N} K={K}: rel {rel(y, ref):.3e}")
    assert rel(y, ref) < 1e-2, rel(y, ref)


def test_gemv_w8_strided_rows():
    wq, s = image(block_weights((384, 1152), 2))
    xb = torch.randn(3, 1152 + 64, device=DEV, dtype=torch.bfloat16, generator=torch.Generator(DEV).manual_seed(3))
    x = xb[:, :1152]
    assert rel(_ext.ops().gemv_w8(x, wq, s), R.gemv_w8(x, wq, s)) < 1e-2


def test_gemv_w8_rejects_bad_calls():
    ops = _ext.ops()
    wq, s = image(block_weights((256, 384), 4))
    x = torch.randn(2, 384, device=DEV, dtype=torch.bfloat16)
    ops.gemv_w8(x, wq, s)
    with pytest.raises(RuntimeError):      # K % 128 != 0
        ops.gemv_w8(x[:, :320].contiguous(), wq[:, :320].contiguous(), s)
    with pytest.raises(RuntimeError):      # s of the wrong shape
        ops.gemv_w8(x, wq, s[:, :2].contiguous())
    with pytest.raises(RuntimeError):
        ops.gemv_w8(x, wq, s.t().contiguous())
    with pytest.raises(RuntimeError):      # more than 4 rows
        ops.gemv_w8(torch.randn(5, 384, device=DEV, dtype=torch.bfloat16), wq, s)
    with pytest.raises(RuntimeError):      # bf16 weights are not an image
        ops.gemv_w8(x, wq.to(torch.bfloat16), s)
    with pytest.raises(RuntimeError):      # x and wq disagree on K
        ops.gemv_w8(x[:, :256].contiguous(), wq, s)
    off = torch.tensor([0, 2], device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError):      # 2-D image to the grouped op
        ops.grouped_gemv_w8(x, wq, s, off)
    with pytest.raises(RuntimeError):      # offsets of the wrong length
        ops.grouped_gemv_w8(x, wq[None], s[None], torch.zeros(3, device=DEV, dtype=torch.int32))


def test_grouped_gemv_w8_matches_fp32_oracle():
    E, N, K = 8, 256, 384
    counts = [0, 1, 0, 5, 2, 0, 4, 0]      # empty experts, a row group that loops, an empty last expert
    wq, s = image(block_weights((E, N, K), 5))
    assert len(torch.unique(s)) > 1
    off = torch.tensor([0] + counts, dtype=torch.int32).cumsum(0).to(DEV, torch.int32)
    x = torch.randn(sum(counts), K, device=DEV, dtype=torch.bfloat16, generator=torch.Generator(DEV).manual_seed(6))
    y = _ext.ops().grouped_gemv_w8(x, wq, s, off)
    ref = R.grouped_gemv_w8(x, wq, s, off)
    assert y.shape == (sum(counts), N) and y.dtype == torch.bfloat16
    print(f"grouped_gemv_w8: rel {rel(y, ref):.3e}")
    assert rel(y, ref) < 1e-2, rel(y, ref)


@pytest.mark.parametrize("N,K", [
    (128, 128),           # one block, 8 live lanes
    (256, 5248),          # unrolled main loop, single-pass remainder and a partial pass
    (8192, 256),          # dense on RW = 4, grouped on RW = 2
])
def test_grouped_gemv_w8_one_expert_is_gemv_w8_bitwise(N, K):
    # dense and grouped are the same accumulation: same per-lane order, same reduction
    wq, s = image(block_weights((N, K), 8))
    assert len(torch.unique(s)) > 1 or s.numel() == 1
    g = torch.Generator(DEV).manual_seed(9)
    for M in (1, 2, 3, 4):
        x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, generator=g)
        off = torch.tensor([0, M], device=DEV, dtype=torch.int32)
        assert torch.equal(_ext.ops().grouped_gemv_w8(x, wq[None], s[None], off), _ext.ops().gemv_w8(x, wq, s)), M


def test_grouped_gemv_w8_row_groups_are_gemv_w8_bitwise():
    # every expert's rows, in groups of at most 4 from its first row, against gemv_w8 on that expert's image
    E, N, K = 8, 256, 384
    counts = [0, 1, 0, 5, 2, 0, 4, 0]
    wq, s = image(block_weights((E, N, K), 10))
    assert len(torch.unique(s)) > 1
    off = torch.tensor([0] + counts, dtype=torch.int32).cumsum(0)
    x = torch.randn(sum(counts), K, device=DEV, dtype=torch.bfloat16, generator=torch.Generator(DEV).manual_seed(11))
    y = _ext.ops().grouped_gemv_w8(x, wq, s, off.to(DEV, torch.int32))
    for e, c in enumerate(counts):
        for a in range(int(off[e]), int(off[e]) + c, 4):
            b = min(a + 4, int(off[e + 1]))
            assert torch.equal(y[a:b], _ext.ops().gemv_w8(x[a:b], wq[e], s[e])), (e, a, b)


def test_linear_routes_decode_rows_to_gemv_w8():
    from solvingpapers_amd.ops.linear import linear

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(block_weights((256, 384), 7), requires_grad=False)

    h = Holder()
    w = h.w
    x = torch.randn(2, 1, 384, device=DEV, dtype=torch.bfloat16)
    x8 = torch.randn(8, 384, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        y_bf16, y8_bf16 = linear(x, w), linear(x8, w)
    rep = quantize_decode_weights(h)
    assert rep["quantized"] == ["w"] and rep["image_bytes"] == 256 * 384 + 2 * 3
    wq, s = w._spa_w8[:2]
    with torch.no_grad():
        y = linear(x, w)
        assert y.shape == (2, 1, 256)
        assert torch.equal(y.view(2, 256), _ext.ops().gemv_w8(x.view(2, 384), wq, s))
        assert not torch.equal(y, y_bf16)                 # fp8 weights: a different product
        assert torch.equal(linear(x8, w), y8_bf16)        # 8 rows: the bf16 GEMM as before
    # autograd on the weight: the bf16 path
    w.requires_grad_(True)
    assert torch.equal(linear(x, w).detach(), linear(x, w.detach().clone().requires_grad_()).detach())
    assert rel(linear(x, w), y_bf16) < 1e-2 and rel(linear(x, w), y_bf16) < rel(y, y_bf16)
    w.requires_grad_(False)
    # an in-place update makes the image stale: an error that names the parameter
    with torch.no_grad():
        w.mul_(2)
        with pytest.raises(RuntimeError, match=r"'w'.*quantize_decode_weights"):
            linear(x, w)
        w.mul_(0.5)                                       # exact: the bf16 weights are back
        clear_decode_weights(h)
        assert not hasattr(w, "_spa_w8")
        assert torch.equal(linear(x, w), y_bf16)


def _fp8_exact_lookup_table_(m):
    """The token table is also READ BY INDEX, and a lookup takes the master rows (a few rows per
    step: nothing to save there), while the dequantised copy looks its rows up in the dequantised
    table. So the table alone starts from fp8-representable values (quantising is idempotent:
    they are their own image); every product still runs on weights that differ from their images."""
    p = getattr(m, "tok_embeddings", None)
    p = p if p is not None else m.embed
    with torch.no_grad():
        p.copy_(R.dequant_w8(*image(p.detach())))
        assert torch.equal(R.dequant_w8(*image(p.detach())).to(p.dtype), p)


def _dequantised_copy(make, model, report):
    """a second model with ``model``'s weights, every quantised one overwritten with its dequantised
    image (exact in bf16)"""
    ref = make()
    ref.load_state_dict(model.state_dict())
    params = dict(model.named_parameters())
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name in report["quantized"]:
                wq, s = params[name]._spa_w8[:2]
                w = R.dequant_w8(wq, s)
                assert torch.equal(w.to(p.dtype).float(), w)
                p.copy_(w)
    return ref.eval()


def _teacher_forced(m, ids):
    with torch.no_grad():
        cache = m.new_cache(ids.shape[0], ids.shape[1])
        return torch.stack([m.step(ids[:, t:t + 1], cache, t) for t in range(ids.shape[1])], 1)


def _llama():
    from solvingpapers_amd.models import llama3
    return llama3.Llama3(llama3.config("llama3_tiny"), device=DEV, dtype=torch.bfloat16, seed=1)


def _dsv3():
    from solvingpapers_amd.models import deepseekv3 as ds
    return ds.DeepSeekV3(ds.config("dsv3_tiny"), device=DEV, dtype=torch.bfloat16, seed=1)


@pytest.fixture(scope="module")
def llama_case():
    torch.manual_seed(0)
    m = _llama().eval()
    _fp8_exact_lookup_table_(m)
    ids = torch.randint(0, m.c.vocab_size, (2, 16), device=DEV)
    with torch.no_grad():
        master = m(ids).float()
    rep = quantize_decode_weights(m)
    ref = _dequantised_copy(_llama, m, rep)
    with torch.no_grad():
        full = ref(ids).float()
    return m, ids, rep, full, master


def test_llama_fp8_decode_matches_dequantised_full_forward(llama_case):
    m, ids, rep, full, master = llama_case
    expect = ["tok_embeddings", "output"] + [f"layers.{i}.{w}" for i in range(m.c.n_layers)
                                             for w in ("wqkv", "wo", "w13", "w2")]
    assert sorted(rep["quantized"]) == sorted(expect)
    got = _teacher_forced(m, ids)
    print(f"llama3_tiny fp8 decode vs dequantised full forward: rel {rel(got, full):.3e}; "
          f"vs the bf16 master's logits (recorded, not asserted): {rel(got, master):.3e}")
    assert rel(got, full) < 2e-2, rel(got, full)


def test_llama_fp8_graph_decoder_matches_dequantised_full_forward(llama_case):
    m, ids, rep, full, _ = llama_case
    with torch.no_grad():
        dec = GraphDecoder(m, 2, 24)
        lg = []
        for t in range(16):                 # replays only, from an empty cache
            dec.ids.copy_(ids[:, t:t + 1])
            dec.graph.replay()
            lg.append(dec.logits.clone())
    got = torch.stack(lg, 1)
    print(f"llama3_tiny fp8 graph decode: rel {rel(got, full):.3e}")
    assert rel(got, full) < 2e-2, rel(got, full)


def test_dsv3_fp8_decode_matches_dequantised_full_forward():
    torch.manual_seed(0)
    m = _dsv3().eval()
    _fp8_exact_lookup_table_(m)
    ids = torch.randint(0, m.c.vocab_size, (2, 16), device=DEV)
    rep = quantize_decode_weights(m)
    experts = [n for n, p in m.named_parameters() if p.dim() == 3]
    assert experts and all(n in rep["quantized"] for n in experts)   # the grouped route is covered
    ref = _dequantised_copy(_dsv3, m, rep)
    with torch.no_grad():
        full = ref(ids).float()
    got = _teacher_forced(m, ids)
    print(f"dsv3_tiny fp8 decode: rel {rel(got, full):.3e}")
    assert rel(got, full) < 2e-2, rel(got, full)
