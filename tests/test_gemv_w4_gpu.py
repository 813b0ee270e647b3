"""MXFP4 weight-only decode on the GPU: gemv_w4 / grouped_gemv_w4 (csrc/kernels/gemv.hip, policy
WMxfp4) exactly where the arithmetic is exact and against the fp32 oracle on the dequantised image
elsewhere, the HIP quantizer (csrc/kernels/quant_mxfp4.hip) bit for bit against ops/reference.py
quant_mxfp4, the routing from linear / grouped_linear, and quantised models decoding token by token
against the full forward of a copy that holds the dequantised weights.

Test weights carry a different power-of-two magnitude in [-6, 6] in every 1 x 32 block, and
vertically adjacent blocks differ too: a wave that applies row r's scale to row r + 1, or block b's to
block b + 1, cannot pass."""
import pytest
import torch

from mxfp4_cases import rule_cases
from solvingpapers_amd.infer import GraphDecoder, clear_decode_weights, quantize_decode_weights
from solvingpapers_amd.ops import _ext, reference as R
from solvingpapers_amd.ops.moe import MoEPlan, grouped_linear

pytestmark = pytest.mark.gpu
DEV = "cuda"
# U is a copy of WMxfp4::U (csrc/kernels/gemv.hip), the dense kernel's passes in flight: change both together, or
# the "U * PASS + PASS + 96" shapes stop reaching the U-pass loop. The grouped kernel has UG = 1 (no U-pass loop of
# its own to cover); PASS: weights per wave and pass.
U, PASS = 8, 64 * 32


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def block_exponents(*shape):
    """[N, K/32] or [E, N, K/32] exponents in [-6, 6]: horizontal neighbours differ by 3, vertical ones by 5,
    the same block of consecutive experts by 7 (all mod 13)"""
    *lead, N, KB = shape
    e = 5 * torch.arange(N)[:, None] + 3 * torch.arange(KB)[None, :]
    if lead:
        e = e[None] + 7 * torch.arange(lead[0])[:, None, None]
    return e % 13 - 6


def block_weights(shape, seed):
    """randn * 2^e, e by block_exponents per 1 x 32 block, bf16 on the device"""
    g = torch.Generator().manual_seed(seed)
    *lead, N, K = shape
    e = block_exponents(*lead, N, K // 32).float()
    w = torch.randn(*lead, N, K // 32, 32, generator=g) * torch.exp2(e)[..., None]
    return w.view(*shape).to(DEV, torch.bfloat16)


def image(w):
    """the image by the torch formula (the kernel tests do not lean on the HIP quantizer)"""
    wq, s = R.quant_mxfp4(w)
    assert len(torch.unique(s)) > 1 or s.numel() == 1
    return wq, s


def random_image(shape, seed, lo, hi):
    """an image built directly: every code, scale exponents in [lo, hi]"""
    g = torch.Generator().manual_seed(seed)
    *lead, N, K = shape
    wq = torch.randint(0, 256, (*lead, N, K // 2), generator=g).to(torch.uint8)
    s = (127 + torch.randint(lo, hi + 1, (*lead, N, K // 32), generator=g)).to(torch.uint8)
    assert len(torch.unique(s)) > 1
    return wq.to(DEV), s.to(DEV)


def test_ordering_exact():
    """Row r's only non-zero weight sits at k = r, so y[r] = x[r] * w[r, r]: a nibble, byte, dword or
    scale taken from the wrong place gives another number. (1..64) times (0.5 .. 6) has at most 8
    significant bits: exact in fp32 and in bf16, so y is the fp64 product bit for bit."""
    N = K = 64
    r = torch.arange(N)
    code = (1 + r % 7) | ((r // 7) % 2) << 3                      # the seven magnitudes, both signs
    wq = torch.zeros(N, K // 2, dtype=torch.int64)
    wq[r, r // 2] = code << (4 * (r % 2))
    s = (127 + block_exponents(N, K // 32)).to(torch.uint8)
    assert len(torch.unique(s)) > 1 and not torch.equal(s[:, 0], s[:, 1]) and not torch.equal(s[0], s[1])
    wq, s = wq.to(torch.uint8).to(DEV), s.to(DEV)
    x1 = torch.arange(1, K + 1, dtype=torch.float64)
    x = torch.stack([x1, 2 * x1, -x1, x1 / 2]).to(DEV)            # still 8 significant bits a product
    w = R.dequant_w4(wq, s).double()
    assert (w != 0).sum() == N and (w.diagonal() != 0).all()
    for M in (1, 4):
        y = _ext.ops().gemv_w4(x[:M].to(torch.bfloat16), wq, s)
        ref = x[:M] * w.diagonal()[None, :]                       # fp64: the one product of each output
        assert torch.equal(y.double(), ref), M


def test_exact_sums():
    """Integer x with |x| <= 8, on-grid weights with scale exponents in [-2, 2], K one full pass plus one
    32-wide chunk: every product and partial sum is a multiple of 2^-3 below 2^24 of those units
    (2080 * 8 * 6 * 4 * 8 < 2^24), so the fp32 accumulation is exact in any order and y is bf16(fp64 sum)."""
    N, K = 256, PASS + 32
    wq, s = random_image((N, K), 20, -2, 2)
    w = R.dequant_w4(wq, s).double()
    x = torch.randint(-8, 9, (4, K), generator=torch.Generator().manual_seed(21)).to(DEV)
    for M in (1, 2, 3, 4):
        y = _ext.ops().gemv_w4(x[:M].to(torch.bfloat16), wq, s)
        ref = (x[:M].double() @ w.t()).to(torch.bfloat16)
        assert torch.equal(y, ref), M


SHAPES = [
    (1, 4, 32),                          # one chunk, one live lane
    (3, 384, PASS + 32),                 # a full pass and a one-chunk tail
    (4, 256, U * PASS + PASS + 96),      # the U-pass loop, a single-pass remainder, a partial pass
    (2, 8192, 256),                      # the RW = 4 path
    (1, 4096, 4096),                     # a real shape (LLaMA3-8B o-proj)
]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemv_w4_matches_fp32_oracle(M, N, K):
    wq, s = image(block_weights((N, K), 0))
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, generator=torch.Generator(DEV).manual_seed(1))
    y = _ext.ops().gemv_w4(x, wq, s)
    ref = R.gemv_w4(x, wq, s)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    print(f"gemv_w4 M={M} N={N} K={K}: rel {rel(y, ref):.3e}")
    assert rel(y, ref) < 1e-2, rel(y, ref)


def test_gemv_w4_strided_rows():
    K = PASS + 32
    wq, s = image(block_weights((384, K), 2))
    xb = torch.randn(3, K + 64, device=DEV, dtype=torch.bfloat16, generator=torch.Generator(DEV).manual_seed(3))
    x = xb[:, :K]
    assert not x.is_contiguous()
    y = _ext.ops().gemv_w4(x, wq, s)
    print(f"gemv_w4 strided x: rel {rel(y, R.gemv_w4(x, wq, s)):.3e}")
    assert rel(y, R.gemv_w4(x, wq, s)) < 1e-2
    assert torch.equal(y, _ext.ops().gemv_w4(x.contiguous(), wq, s))


@pytest.mark.parametrize("N,K", [(4, 32), (256, U * PASS + PASS + 96), (8192, 256)])
def test_grouped_gemv_w4_one_expert_is_gemv_w4_bitwise(N, K):
    # dense and grouped are the same accumulation: same per-lane order, same reduction
    wq, s = image(block_weights((N, K), 8))
    g = torch.Generator(DEV).manual_seed(9)
    for M in (1, 2, 3, 4):
        x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16, generator=g)
        off = torch.tensor([0, M], device=DEV, dtype=torch.int32)
        assert torch.equal(_ext.ops().grouped_gemv_w4(x, wq[None], s[None], off), _ext.ops().gemv_w4(x, wq, s)), M


def test_grouped_gemv_w4_row_groups_are_gemv_w4_bitwise():
    # every expert's rows, in groups of at most 4 from its first row, against gemv_w4 on that expert's image
    E, N, K = 8, 256, 384
    counts = [0, 1, 0, 5, 2, 0, 4, 0]      # empty experts, a row group that loops, an empty last expert
    wq, s = image(block_weights((E, N, K), 10))
    assert not torch.equal(s[3], s[4])
    off = torch.tensor([0] + counts, dtype=torch.int32).cumsum(0)
    x = torch.randn(sum(counts), K, device=DEV, dtype=torch.bfloat16, generator=torch.Generator(DEV).manual_seed(11))
    y = _ext.ops().grouped_gemv_w4(x, wq, s, off.to(DEV, torch.int32))
    ref = R.grouped_gemv_w4(x, wq, s, off)
    print(f"grouped_gemv_w4: rel {rel(y, ref):.3e}")
    assert y.shape == (sum(counts), N) and y.dtype == torch.bfloat16 and rel(y, ref) < 1e-2
    for e, c in enumerate(counts):
        for a in range(int(off[e]), int(off[e]) + c, 4):
            b = min(a + 4, int(off[e + 1]))
            assert torch.equal(y[a:b], _ext.ops().gemv_w4(x[a:b], wq[e], s[e])), (e, a, b)


@pytest.mark.parametrize("name", list(rule_cases()))
def test_quant_weight_mxfp4_is_the_reference_bitwise_on_the_rule_cases(name):
    W = rule_cases()[name]
    wq, s = _ext.ops().quant_weight_mxfp4(W.to(DEV)[None])
    wq_ref, s_ref = R.quant_mxfp4(W)
    assert wq.dtype == torch.uint8 and s.dtype == torch.uint8
    assert torch.equal(s[0].cpu(), s_ref) and torch.equal(wq[0].cpu(), wq_ref)


def test_quant_weight_mxfp4_is_the_reference_bitwise():
    W = block_weights((3, 128, 160), 12)
    wq, s = _ext.ops().quant_weight_mxfp4(W)
    wq_ref, s_ref = R.quant_mxfp4(W.cpu())
    assert wq.shape == (3, 128, 80) and s.shape == (3, 128, 5) and len(torch.unique(s)) > 1
    assert torch.equal(s.cpu(), s_ref) and torch.equal(wq.cpu(), wq_ref)
    with pytest.raises(RuntimeError):      # K % 32 != 0
        _ext.ops().quant_weight_mxfp4(W[:, :, :144])
    with pytest.raises(RuntimeError):      # 2-D
        _ext.ops().quant_weight_mxfp4(W[0])


def test_gemv_w4_rejects_bad_calls():
    ops = _ext.ops()
    wq, s = image(block_weights((256, 384), 4))
    x = torch.randn(2, 384, device=DEV, dtype=torch.bfloat16)
    ops.gemv_w4(x, wq, s)
    with pytest.raises(RuntimeError):      # K % 32 != 0
        ops.gemv_w4(x[:, :368].contiguous(), wq[:, :184].contiguous(), s)
    with pytest.raises(RuntimeError):      # N % 4 != 0
        ops.gemv_w4(x, wq[:254].contiguous(), s[:254].contiguous())
    with pytest.raises(RuntimeError):      # s of the wrong shape
        ops.gemv_w4(x, wq, s[:, :11].contiguous())
    with pytest.raises(RuntimeError):      # s transposed
        ops.gemv_w4(x, wq, s.t().contiguous())
    with pytest.raises(RuntimeError):
        ops.gemv_w4(x, wq, s.t().contiguous().t())
    with pytest.raises(RuntimeError):      # more than 4 rows
        ops.gemv_w4(torch.randn(5, 384, device=DEV, dtype=torch.bfloat16), wq, s)
    with pytest.raises(RuntimeError):      # bf16 weights are not an image
        ops.gemv_w4(x, wq.to(torch.bfloat16), s)
    with pytest.raises(RuntimeError):      # nor are fp8 ones
        ops.gemv_w4(x, wq.view(torch.float8_e4m3fn), s)
    with pytest.raises(RuntimeError):      # x and wq disagree on K
        ops.gemv_w4(x[:, :256].contiguous(), wq, s)
    off = torch.tensor([0, 2], device=DEV, dtype=torch.int32)
    with pytest.raises(RuntimeError):      # 2-D image to the grouped op
        ops.grouped_gemv_w4(x, wq, s, off)
    with pytest.raises(RuntimeError):      # offsets of the wrong length
        ops.grouped_gemv_w4(x, wq[None], s[None], torch.zeros(3, device=DEV, dtype=torch.int32))
    ops.grouped_gemv_w4(x, wq[None], s[None], off)


class Holder(torch.nn.Module):
    def __init__(self, shape, seed):
        super().__init__()
        self.w = torch.nn.Parameter(block_weights(shape, seed), requires_grad=False)


def test_linear_routes_decode_rows_to_gemv_w4():
    from solvingpapers_amd.ops.linear import linear
    h = Holder((256, 384), 7)
    w = h.w
    x = torch.randn(2, 1, 384, device=DEV, dtype=torch.bfloat16)
    x8 = torch.randn(8, 384, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        y_bf16, y8_bf16 = linear(x, w), linear(x8, w)
    rep = quantize_decode_weights(h, fmt="mxfp4")
    assert rep["quantized"] == ["w"] and rep["image_bytes"] == 256 * 384 // 2 + 256 * 384 // 32
    wq, s = w._spa_w4[:2]
    assert torch.equal(wq, R.quant_mxfp4(w.detach())[0]) and torch.equal(s, R.quant_mxfp4(w.detach())[1])
    with torch.no_grad():
        y = linear(x, w)
        assert y.shape == (2, 1, 256)
        assert torch.equal(y.view(2, 256), _ext.ops().gemv_w4(x.view(2, 384), wq, s))
        assert not torch.equal(y, y_bf16)                 # 4-bit weights: a different product
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
        assert not hasattr(w, "_spa_w4")
        assert torch.equal(linear(x, w), y_bf16)


def test_grouped_linear_routes_decode_rows_to_grouped_gemv_w4():
    E, N, K = 4, 256, 384
    h = Holder((E, N, K), 13)
    W = h.w
    counts = [2, 0, 5, 1]
    off = torch.tensor([0] + counts, dtype=torch.int32).cumsum(0).to(DEV, torch.int32)
    plan = MoEPlan(None, None, off, off[1:] - off[:-1], 1, sum(counts))
    x = torch.randn(sum(counts), K, device=DEV, dtype=torch.bfloat16)
    big = [20, 30, 10, 20]                                # 80 rows: past the decode route
    off_big = torch.tensor([0] + big, dtype=torch.int32).cumsum(0).to(DEV, torch.int32)
    plan_big = MoEPlan(None, None, off_big, off_big[1:] - off_big[:-1], 1, sum(big))
    xb = torch.randn(sum(big), K, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        y_bf16, yb_bf16 = grouped_linear(x, W, plan), grouped_linear(xb, W, plan_big)
    quantize_decode_weights(h, fmt="mxfp4")
    wq, s = W._spa_w4[:2]
    with torch.no_grad():
        y = grouped_linear(x, W, plan)
        assert torch.equal(y, _ext.ops().grouped_gemv_w4(x, wq, s, off))
        assert not torch.equal(y, y_bf16)
        assert torch.equal(grouped_linear(xb, W, plan_big), yb_bf16)      # many rows: the bf16 GEMM as before
    W.requires_grad_(True)                                # autograd: the bf16 masters
    assert rel(grouped_linear(x, W, plan), y_bf16) < 1e-2
    W.requires_grad_(False)
    with torch.no_grad():
        W.mul_(2)
        with pytest.raises(RuntimeError, match=r"'w'.*quantize_decode_weights"):
            grouped_linear(x, W, plan)
        W.mul_(0.5)
        clear_decode_weights(h)
        assert torch.equal(grouped_linear(x, W, plan), y_bf16)


def _exact_lookup_table_(m):
    """The token table is also read by index, from the master rows, while the dequantised copy looks its
    rows up in the dequantised table: so the table alone starts from values that are their own image
    (tests/test_gemv_w8_gpu.py does the same for fp8)."""
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
                w = R.dequant_w4(*params[name]._spa_w4[:2])
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
    _exact_lookup_table_(m)
    ids = torch.randint(0, m.c.vocab_size, (2, 16), device=DEV)
    with torch.no_grad():
        master = m(ids).float()
    rep = quantize_decode_weights(m, fmt="mxfp4")
    ref = _dequantised_copy(_llama, m, rep)
    with torch.no_grad():
        full = ref(ids).float()
    return m, ids, rep, full, master


def test_llama_mxfp4_decode_matches_dequantised_full_forward(llama_case):
    m, ids, rep, full, master = llama_case
    expect = ["tok_embeddings", "output"] + [f"layers.{i}.{w}" for i in range(m.c.n_layers)
                                             for w in ("wqkv", "wo", "w13", "w2")]
    assert sorted(rep["quantized"]) == sorted(expect) and rep["format"] == "mxfp4-e2m1 1x32 E8M0"
    got = _teacher_forced(m, ids)
    print(f"llama3_tiny mxfp4 decode vs dequantised full forward: rel {rel(got, full):.3e}; "
          f"vs the bf16 master's logits (recorded, not asserted): {rel(got, master):.3e}")
    assert rel(got, full) < 2e-2, rel(got, full)


def test_llama_mxfp4_graph_decoder_matches_dequantised_full_forward(llama_case):
    m, ids, rep, full, master = llama_case
    with torch.no_grad():
        dec = GraphDecoder(m, 2, 24)
        lg = []
        for t in range(16):                 # replays only, from an empty cache
            dec.ids.copy_(ids[:, t:t + 1])
            dec.graph.replay()
            lg.append(dec.logits.clone())
    got = torch.stack(lg, 1)
    print(f"llama3_tiny mxfp4 graph decode: rel {rel(got, full):.3e}; "
          f"vs the bf16 master's logits (recorded, not asserted): {rel(got, master):.3e}")
    assert rel(got, full) < 2e-2, rel(got, full)


def test_dsv3_mxfp4_decode_matches_dequantised_full_forward():
    torch.manual_seed(0)
    m = _dsv3().eval()
    _exact_lookup_table_(m)
    ids = torch.randint(0, m.c.vocab_size, (2, 16), device=DEV)
    with torch.no_grad():
        master = m(ids).float()
    rep = quantize_decode_weights(m, fmt="mxfp4")
    experts = [n for n, p in m.named_parameters() if p.dim() == 3]
    assert experts and all(n in rep["quantized"] for n in experts)   # the grouped route is covered
    ref = _dequantised_copy(_dsv3, m, rep)
    with torch.no_grad():
        full = ref(ids).float()
    got = _teacher_forced(m, ids)
    print(f"dsv3_tiny mxfp4 decode: rel {rel(got, full):.3e}; "
          f"vs the bf16 master's logits (recorded, not asserted): {rel(got, master):.3e}")
    assert rel(got, full) < 2e-2, rel(got, full)
