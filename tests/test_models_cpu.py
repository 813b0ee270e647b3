"""Model parity against the reference's own code (its recorded results, tests/refgolden.py)
and CPU training smoke tests for the catalogue (SURVEY §4.2 tiers T2/T3)."""
import math

import pytest
import torch

import refgolden


def test_gemma_ref_parity():
    from solvingpapers_amd.models import gemma
    d = refgolden.load("gemma")  # small config, reference semantics (gemma.ipynb:27-43)
    c = gemma.GemmaRefConfig(block_size=16, embeddings_dims=64, no_of_heads=4, no_kv_heads=2, vocab_size=30,
                             no_of_decoder_layers=2)
    ours = gemma.GemmaRef(c).eval()
    ours.load_state_dict(refgolden.get_state(d, "", 100))
    assert torch.allclose(ours(d["x0"]), d["y0"], atol=1e-4, rtol=1e-4)
    assert d["x1"].shape == (2, 11)  # T < block_size
    assert torch.allclose(ours(d["x1"]), d["y1"], atol=1e-4, rtol=1e-4)


def test_gemma_ref_param_count():
    from solvingpapers_amd.models import gemma
    assert sum(p.numel() for p in gemma.GemmaRef().parameters()) == 127_521_089  # gemma.ipynb:495


def test_vit_parity():
    from solvingpapers_amd.models import vit
    d = refgolden.load("vit")
    ours = vit.ViT(vit.config("vit_mnist_ref")).eval()
    ours.load_state_dict(refgolden.get_state(d, "", 101))
    assert torch.allclose(ours(d["x"]), d["y"], atol=1e-4, rtol=1e-4)


def test_ae_vae_parity():
    from solvingpapers_amd.models import autoencoder as A
    d = refgolden.load("ae_vae")
    ours = A.AutoEncoder()
    ours.load_state_dict(refgolden.get_state(d, "ae/", 102))
    x = d["x"]
    assert torch.allclose(ours(x), d["ae/y"], atol=1e-6)
    ours = A.VAE()
    ours.load_state_dict(refgolden.get_state(d, "vae/", 103))
    from solvingpapers_amd.ops.misc import vae_loss
    # fp32 against values recorded on another machine: dot products of up to 784 fp32 terms summed in
    # that machine's order, so 1e-6 absolute for mu / logvar too (as for the reconstruction) ...
    r1, mu1, lv1 = d["vae/r"], d["vae/mu"], d["vae/lv"]
    torch.manual_seed(3)
    r2, mu2, lv2 = ours(x)
    assert torch.allclose(r1, r2, atol=1e-6) and torch.allclose(mu1, mu2, atol=1e-6) and torch.allclose(lv1, lv2, atol=1e-6)
    assert torch.allclose(vae_loss(r2, x, mu2, lv2), d["vae/loss"], rtol=1e-5)
    # ... and in fp64, where the summation order does not show, at the tolerances of the in-process comparison
    ours, x = ours.double(), x.double()
    r1, mu1, lv1 = d["vae64/r"], d["vae64/mu"], d["vae64/lv"]
    torch.manual_seed(3)
    r2, mu2, lv2 = ours(x)
    assert r2.dtype == torch.float64
    assert torch.allclose(r1, r2, atol=1e-6) and torch.allclose(mu1, mu2) and torch.allclose(lv1, lv2)
    assert torch.allclose(vae_loss(r2, x, mu2, lv2), d["vae64/loss"], rtol=1e-5)


def test_kd_alexnet_luong_parity():
    from solvingpapers_amd.models import alexnet, kd, luong
    d = refgolden.load("kd_alexnet_luong")
    os_, ot = kd.Student(), kd.Teacher()
    os_.load_state_dict(refgolden.get_state(d, "student/", 104))
    ot.load_state_dict(refgolden.get_state(d, "teacher/", 105))
    x, y = d["kd/x"], d["kd/y"]
    assert torch.allclose(os_(x), d["kd/s"], atol=1e-5) and torch.allclose(ot(x), d["kd/t"], atol=1e-5)
    # in fp64 (so recorded): the soft loss is a small KL, a cancellation, times T^2 = 49
    b = kd.distillation_loss(d["kd/s"].double(), d["kd/t"].double(), y, 7, 0.3)
    assert len(b) == 3
    for i, v in enumerate(b):
        assert torch.allclose(d[f"kd/loss{i}"], v, atol=1e-6)
    oa = alexnet.AlexNet(10).eval()
    oa.load_state_dict(refgolden.get_state(d, "alexnet/", 106))
    x = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(107))
    assert torch.allclose(oa(x), d["alexnet/y"], atol=1e-4)
    assert sum(p.numel() for p in oa.parameters()) == 46_787_978
    la = luong.LuongAttention(8)
    la.load_state_dict(refgolden.get_state(d, "luong/", 108))
    c2, w2 = la(d["luong/st"], d["luong/hs"])
    assert torch.allclose(d["luong/c"], c2, atol=1e-6) and torch.allclose(d["luong/w"], w2, atol=1e-6)


def test_activation_value_table_matches_numpy_reference():
    import numpy as np
    from solvingpapers_amd.models import activations as A
    t = A.value_table()
    ref = A.numpy_reference()
    x = t["x"].numpy()
    assert np.allclose(t["relu"].numpy(), ref["relu"](x))
    assert np.allclose(t["leakyrelu"].numpy(), ref["leakyrelu"](x))
    assert np.allclose(t["prelu"].numpy(), ref["prelu"](x, 0.3))
    assert np.allclose(t["elu"].numpy(), ref["elu"](x, 0.4), atol=1e-6)
    assert np.allclose(t["gelu"].numpy(), ref["gelu"](x), atol=1e-5)


def test_gpt_counts_and_training():
    from solvingpapers_amd.models import gpt
    assert gpt.GPT(gpt.config("gpt_ref")).num_params() == 6_411_264
    from solvingpapers_amd.train.optim import FlatAdamW
    from solvingpapers_amd.utils.flat import FlatParams
    from solvingpapers_amd.data import CharTokenizer, get_batch, synthetic_corpus
    text = synthetic_corpus(20000)
    tok = CharTokenizer(text)
    data = torch.tensor(tok.encode(text))
    c = gpt.config("gpt_tiny_cpu", vocab_size=tok.vocab_size)
    m = gpt.GPT(c)
    flat = FlatParams(m, groups=m.param_groups())
    opt = FlatAdamW(flat, lr=3e-3, weight_decay=0.01)
    g = torch.Generator().manual_seed(0)
    losses = []
    for _ in range(60):
        x, y = get_batch(data, c.batch_size, c.block_size, g)
        opt.zero_grad()
        loss = m(x, y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0] - 1.0, (losses[0], losses[-1])
    out = m.generate(torch.tensor([tok.encode("ROMEO:\n")]), 20)
    assert len(tok.decode(out[0].tolist())) == 27


def test_gpt_flax_layout_round_trip():
    from solvingpapers_amd.models import gpt
    a = gpt.GPT(gpt.config("gpt_tiny_cpu"), seed=1)
    b = gpt.GPT(gpt.config("gpt_tiny_cpu"), seed=2).from_reference_params(a.to_reference_params())
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)
    d = a.to_reference_params()
    assert d["layers_0/attn/qkv/kernel"].shape == (128, 384) and d["lm_head/kernel"].shape == (128, 65)


def test_gpt_matches_flax_reference_math_fp64():
    """Numeric parity with gpt/gpt-jax.ipynb:321-472 (restated in fp64, tests/refimpl.py gpt_forward:
    fused QKV (in, out) kernel split q|k|v, -1e4 causal fill, tanh GELU, flax LayerNorm eps 1e-6,
    learned pos_embed, untied bias-free head) and its loss (:499-503), at gpt_ref widths (D256, one
    256-wide head, V65, T256) with 2 layers: the same Flax pytree loaded into models/gpt.py through
    from_reference_params gives equal logits and loss (rel <= 1e-10) and equal gradients."""
    from refimpl import gpt_forward, gpt_loss
    from solvingpapers_amd.models import gpt
    c = gpt.config("gpt_ref", num_layers=2)
    src = gpt.GPT(c, dtype=torch.float64, seed=3)
    d = src.to_reference_params(dtype=None)
    m = gpt.GPT(c, dtype=torch.float64, seed=9).from_reference_params(d).eval()
    ids = torch.randint(0, c.vocab_size, (2, c.block_size + 1), generator=torch.Generator().manual_seed(1))
    x, y = ids[:, :-1], ids[:, 1:]
    dr = {k: v.clone().requires_grad_(True) for k, v in d.items()}
    ref_logits = gpt_forward(dr, x, c.num_heads, c.num_layers)
    ref_loss = gpt_loss(ref_logits, y)
    ref_loss.backward()
    with torch.no_grad():
        logits = m(x)
    rel = ((logits - ref_logits.detach()).norm() / ref_logits.detach().norm()).item()
    assert logits.dtype == torch.float64 and rel <= 1e-10, rel
    loss = m(x, y)
    assert abs(loss.item() - ref_loss.item()) <= 1e-10 * abs(ref_loss.item()), (loss.item(), ref_loss.item())
    loss.backward()
    saved = {n: p.detach().clone() for n, p in m.named_parameters()}
    with torch.no_grad():                       # the gradients in the pytree layout
        for p in m.parameters():
            p.copy_(p.grad)
        grads = m.to_reference_params(dtype=None)
        for n, p in m.named_parameters():
            p.copy_(saved[n])
    for k, g in grads.items():
        want = dr[k].grad
        r = ((g - want).norm() / want.norm().clamp_min(1e-300)).item()
        assert r <= 1e-9, (k, r)


@pytest.mark.parametrize("kind", ["ae", "vae"])
def test_autoencoder_training_cpu(kind):
    from solvingpapers_amd.models import autoencoder as A
    _, hist = A.train(A.AEConfig(kind=kind, epochs=2, n_train=512, batch_size=64, device="cpu"), log=lambda *a: None)
    assert hist[-1] < hist[0]


def test_kd_and_vit_training_cpu():
    from solvingpapers_amd.models import kd, vit
    _, _, hist = kd.train(kd.KDConfig(epochs=2, teacher_epochs=1, n_train=1024, n_test=256, device="cpu"),
                          log=lambda *a: None)
    assert hist[-1][1] > 50.0  # synthetic MNIST-like digits are learnable
    _, accs = vit.train(vit.config("vit_mnist_ref"), epochs=2, device="cpu", n_train=1024, n_test=256,
                        log=lambda *a: None)
    assert accs[-1] > 30.0


def test_reference_named_api(tmp_path):
    """Reference entry-point names (solvingpapers_amd/api.py): pickle-free LLaMA pytree I/O,
    DSV3 get_lr / compute_mtp_loss / topk_sampling / checkpoint, estimate_loss."""
    import torch.nn.functional as F
    from solvingpapers_amd import api
    from solvingpapers_amd.models import deepseekv3 as ds, llama3
    m = llama3.Llama3(llama3.config("llama3_ref", vocab_size=64, dim=32, n_heads=4, n_kv_heads=2, ffn_hidden=64))
    tree = m.to_reference_params()
    p = str(tmp_path / "params.safetensors")
    api.save_params(tree, p)
    back = api.load_params(p)
    m2 = llama3.Llama3(llama3.config("llama3_ref", vocab_size=64, dim=32, n_heads=4, n_kv_heads=2, ffn_hidden=64), seed=3)
    m2.from_reference_params(back)
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    assert abs(api.get_lr(0) - 6e-4 / 401) < 1e-12 and abs(api.get_lr(20000) - 6e-5) < 1e-12
    # compute_mtp_loss vs the notebook's double loop
    B, T, D, C = 2, 5, 2, 7
    lg = torch.randn(B, T, D, C)
    tg = torch.randint(0, C, (B, T))
    idx = [min(i + k + 1, T - 1) for i in range(T) for k in range(D)]
    ref = F.cross_entropy(lg.reshape(-1, C), tg[:, idx].reshape(-1))
    assert torch.allclose(api.compute_mtp_loss(lg, tg), ref)
    dm = ds.DeepSeekV3(ds.config("dsv3_tiny", vocab_size=64, n_layers=1))
    out = api.topk_sampling(dm, torch.zeros(1, 3, dtype=torch.long), max_length=8, top_k=5,
                            generator=torch.Generator().manual_seed(0))
    assert out.shape == (1, 8)
    data = torch.randint(0, 64, (500,))
    est = api.estimate_loss(m, {"train": data, "val": data}, 2, 4, 16)
    assert set(est) == {"train", "val"} and all(v > 0 for v in est.values())
