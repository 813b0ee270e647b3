"""``quantize_decode_weights(max_rows=)`` on the CPU (solvingpapers_amd/infer/quant.py, ops/linear.py): the argument's
validation, the ``_spa_wrows`` attribute beside the images, the routing of 5..max_rows-row inference products to the
dequantised oracle product, and a quantised llama3_tiny generating a ragged batch of 8 from its images."""
import pytest
import torch

from solvingpapers_amd.infer import clear_decode_weights, generate, quantize_decode_weights
from solvingpapers_amd.models import llama3
from solvingpapers_amd.ops import moe as M, reference as R
from solvingpapers_amd.ops.linear import linear

FMTS = ("fp8", "mxfp4")
ATTR = {"fp8": "_spa_w8", "mxfp4": "_spa_w4"}


def _llama():
    return llama3.Llama3(llama3.config("llama3_tiny"), seed=1).eval()


def _eligible(p):
    return p.dim() in (2, 3) and p.shape[-1] % 128 == 0 and p.shape[-2] % 128 == 0


@pytest.mark.parametrize("bad", [3, 17, 4.0, "8", None, True])
def test_max_rows_is_validated(bad):
    m = _llama()
    with pytest.raises(ValueError, match="max_rows"):
        quantize_decode_weights(m, max_rows=bad)
    assert not any(hasattr(p, "_spa_w8") or hasattr(p, "_spa_wrows") for p in m.parameters())


@pytest.mark.parametrize("fmt", FMTS)
def test_attribute_lives_and_dies_with_the_image(fmt):
    m = _llama()
    params = dict(m.named_parameters())
    assert quantize_decode_weights(m, fmt=fmt)["max_rows"] == 4
    assert all(p._spa_wrows == 4 for p in params.values() if _eligible(p))
    plain = {n: getattr(p, ATTR[fmt]) for n, p in params.items() if _eligible(p)}
    for rows in (4, 16, 9):
        rep = quantize_decode_weights(m, fmt=fmt, max_rows=rows)
        assert rep["max_rows"] == rows
        for n, p in params.items():                           # set on exactly the quantised parameters
            assert (n in rep["quantized"]) == _eligible(p) == hasattr(p, "_spa_wrows") == hasattr(p, ATTR[fmt])
            if _eligible(p):
                assert p._spa_wrows == rows and type(p._spa_wrows) is int
                im = getattr(p, ATTR[fmt])                    # the 5-tuple is what it was
                assert len(im) == 5 and im[2:] == (p._version, p.data_ptr(), n) == plain[n][2:]
                assert torch.equal(im[0].view(torch.uint8), plain[n][0].view(torch.uint8)) and torch.equal(im[1], plain[n][1])
    quantize_decode_weights(m, fmt=fmt, max_rows=16, skip=("layers.0.*",))
    for n, p in params.items():
        assert hasattr(p, "_spa_wrows") == (_eligible(p) and not n.startswith("layers.0."))
    other = "mxfp4" if fmt == "fp8" else "fp8"
    assert quantize_decode_weights(m, fmt=other)["max_rows"] == 4      # another format: its own max_rows
    for p in params.values():
        assert not hasattr(p, ATTR[fmt]) and hasattr(p, "_spa_wrows") == hasattr(p, ATTR[other]) == _eligible(p)
        assert getattr(p, "_spa_wrows", 4) == 4
    quantize_decode_weights(m, fmt=fmt, max_rows=16)
    clear_decode_weights(m)
    assert not any(hasattr(p, a) for p in m.parameters() for a in ("_spa_w8", "_spa_w4", "_spa_wrows"))


@pytest.mark.parametrize("fmt", FMTS)
def test_linear_reads_the_image_up_to_max_rows(fmt):
    m = _llama()
    w = m.layers[0].wo
    oracle = R.gemv_w8 if fmt == "fp8" else R.gemv_w4
    g = torch.Generator().manual_seed(0)
    x2, x8, x16, x17 = (torch.randn(r, w.shape[1], generator=g) for r in (2, 8, 16, 17))
    with torch.no_grad():
        master = {r: linear(x, w) for r, x in ((8, x8), (16, x16), (17, x17))}
        quantize_decode_weights(m, fmt=fmt)                            # the default: 8 rows run on the master
        assert torch.equal(linear(x8, w), master[8])
        y2 = linear(x2, w)
        quantize_decode_weights(m, fmt=fmt, max_rows=16)
        im = getattr(w, ATTR[fmt])[:2]
        assert torch.equal(linear(x8, w), oracle(x8, *im)) and not torch.equal(linear(x8, w), master[8])
        assert torch.equal(linear(x16.view(4, 4, -1), w).view(16, -1), oracle(x16, *im))
        assert torch.equal(linear(x2, w), y2) and torch.equal(y2, oracle(x2, *im))
        assert torch.equal(linear(x17, w), master[17])                 # 17 rows: the master
        quantize_decode_weights(m, fmt=fmt, max_rows=8)
        assert torch.equal(linear(x8, w), oracle(x8, *im)) and torch.equal(linear(x16, w), master[16])
    assert torch.equal(linear(x8, w).detach(), master[8])              # autograd on the weight: the master
    with torch.no_grad():
        w.add_(1e-3)
        with pytest.raises(RuntimeError, match=r"layers\.0\.wo.*quantize_decode_weights"):
            linear(x8, w)                                              # the stale-image check, as for the GEMV


def _dequantised_copy(model, report, fmt):
    ref = _llama()
    ref.load_state_dict(model.state_dict())
    params = dict(model.named_parameters())
    deq = R.dequant_w8 if fmt == "fp8" else R.dequant_w4
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name in report["quantized"]:
                p.copy_(deq(*getattr(params[name], ATTR[fmt])[:2]))
    return ref


@pytest.mark.parametrize("fmt", FMTS)
def test_llama_generates_a_ragged_batch_of_8_from_the_images(fmt):
    """generate(..., prompt_lens=) at batch 8 with max_rows=16 picks, token by token, the greedy tokens of the
    dequantised copy's full forward over the same sequence; its decode-step logits are more than 1e-3 relative L2
    from the master's, so the images ran."""
    torch.manual_seed(0)
    m = _llama()
    p = m.tok_embeddings
    with torch.no_grad():            # the table is also read by index from the masters: start it on its own grid
        if fmt == "fp8":
            wq, _, s, _ = M.quant_weight_fp8_blk_uncached(p.detach()[None])
            p.copy_(R.dequant_w8(wq[0], s[0]))
        else:
            p.copy_(R.dequant_w4(*R.quant_mxfp4(p.detach())))
    # prompts of 1 and 2 tokens: the ragged prefill is a 16-row product and every decode step an 8-row one, so all
    # of the generation reads the images (a longer prefill runs on the masters, as it does at the default)
    lens = [1, 2, 2, 1, 2, 1, 1, 2]
    new = 8
    ids = torch.randint(1, m.c.vocab_size, (8, 2))
    rep = quantize_decode_weights(m, fmt=fmt, max_rows=16)
    with torch.no_grad():
        out = generate(m, ids, new, greedy=True, prompt_lens=lens)
        ref = _dequantised_copy(m, rep, fmt)
        for b, n in enumerate(lens):
            seq = out[b:b + 1, :n + new]
            assert torch.equal(seq[0, :n], ids[b, :n])
            full = ref(seq)[0]
            assert torch.equal(full[n - 1:n + new - 1].argmax(-1), seq[0, n:]), (fmt, b)
        # a one-token step of all 8 rows at once (8-row products), against the master's logits
        cache = m.new_cache(8, 4)
        step8 = m.step(ids[:, :1], cache, 0)
        clear_decode_weights(m)
        cache = m.new_cache(8, 4)
        master = m.step(ids[:, :1], cache, 0)
        moved = ((step8 - master).norm() / master.norm()).item()
    assert moved > 1e-3, moved
