#!/usr/bin/env python
"""Record the goldens of the reference-parity tests (tests/golden/, read through tests/refgolden.py).

Usage: ``python oracle/make_golden.py REFERENCE_DIR`` with a checkout of the reference project.
Its notebooks' own PyTorch class / function cells (picked by the names they define) and its two
plain scripts are executed on CPU, with the small configs of tests/test_models_cpu.py and
tests/test_deepseek_cpu.py; what is stored is data only: the state dicts those models were built
with (or their key -> shape lists), the inputs, and the outputs, losses, gradients and updated
buffers the tests compare against. Nothing of the reference's code is copied. Re-run only when a
test's config or inputs change; the run is deterministic (CPU, seeded)."""
import json
import math
import os
import re
import sys
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refgolden as G  # noqa: E402

REF = None


def cells(rel, names):
    nb = json.load(open(os.path.join(REF, rel)))
    out = []
    for c in nb["cells"]:
        if c["cell_type"] != "code":
            continue
        src = "".join(c["source"])
        if any(re.search(rf"^(class|def) {n}\b", src, re.M) for n in names):
            out.append(src)
    return out


def exec_cells(rel, names, ns=None):
    g = {"torch": torch, "nn": nn, "F": F, "math": math}
    g.update(ns or {})
    for src in cells(rel, names):
        exec(compile(src, f"{rel}", "exec"), g)
    return g


def use_state(d, prefix, ref, seed):
    """Record the reference model's state dict (or, if too large, its shapes: the model then takes
    the seeded fill both sides can rebuild)."""
    ref.load_state_dict(G.put_state(d, prefix, ref.state_dict(), seed))
    return ref


def gemma():
    class args:  # small config, reference semantics (gemma.ipynb:27-43)
        block_size = 16; batch_size = 2; embeddings_dims = 64; attn_dropout = 0.1; no_of_heads = 4
        dropout = 0.1; epochs = 1; max_lr = 2.5e-4; no_of_decoder_layers = 2; weight_decay_optim = 0.1
        beta_1 = 0.9; beta_2 = 0.95; device = "cpu"; no_kv_heads = 2; vocab_size = 30
    ns = exec_cells("gemma/gemma.ipynb", ["RMSNorm", "RotaryEmbeddings", "MQA", "GeGLU", "FFN",
                                          "DecoderLayer", "Gemma"], {"args": args})
    torch.manual_seed(0)
    ref = ns["Gemma"](embeddings_dims=64, block_size=16, vocab_size=30, dropout=0.1).eval()
    d = {}
    use_state(d, "", ref, 100)
    d["x0"] = torch.randint(0, 30, (2, 16))
    d["x1"] = torch.randint(0, 30, (2, 11))  # T < block_size
    with torch.no_grad():
        d["y0"], d["y1"] = ref(d["x0"]), ref(d["x1"])
    return d


def vit():
    g = dict(num_classes=10, batch_size=4, num_channels=1, image_size=28, patch_size=7, num_patches=16,
             embedding_dim=64, attention_heads=4, transformer_blocks=4, learning_rate=1e-3, epochs=1,
             mlp_hidden_nodes=128)
    ns = exec_cells("vision transformer/ViT.ipynb", ["PatchEmbedding", "TransformerEncoder", "MLPHead", "ViT"], g)
    torch.manual_seed(0)
    ref = ns["ViT"]().eval()
    d = {}
    use_state(d, "", ref, 101)
    d["x"] = torch.rand(3, 1, 28, 28)
    with torch.no_grad():
        d["y"] = ref(d["x"])
    return d


def ae_vae():
    d = {}
    ns = exec_cells("autoencoder/autoencoder.ipynb", ["AutoEncoder"])
    torch.manual_seed(0)
    ref = use_state(d, "ae/", ns["AutoEncoder"](), 102)
    x = d["x"] = torch.rand(5, 784)
    with torch.no_grad():
        d["ae/y"] = ref(x)
    ns = exec_cells("autoencoder/variational autoencoder.ipynb", ["VAE", "vae_loss"])
    ref = use_state(d, "vae/", ns["VAE"](), 103)
    with torch.no_grad():
        torch.manual_seed(3)
        d["vae/r"], d["vae/mu"], d["vae/lv"] = ref(x)
        d["vae/loss"] = ns["vae_loss"](d["vae/r"], x, d["vae/mu"], d["vae/lv"])
        # the same in fp64, where the recorded values do not depend on the machine's fp32 summation
        # order: what the test holds to the tight tolerances
        ref, x = ref.double(), x.double()
        torch.manual_seed(3)
        d["vae64/r"], d["vae64/mu"], d["vae64/lv"] = ref(x)
        d["vae64/loss"] = ns["vae_loss"](d["vae64/r"], x, d["vae64/mu"], d["vae64/lv"])
    return d


def kd_alexnet_luong():
    d = {}
    path = os.path.join(REF, "knowledge distillation/kd.py")
    src = open(path).read()
    src = src.split("# data")[0].replace("from torchvision import datasets, transforms", "")
    ns = {}
    exec(compile(src, path, "exec"), ns)
    torch.manual_seed(0)
    s, t = use_state(d, "student/", ns["Student"](), 104), use_state(d, "teacher/", ns["Teacher"](), 105)
    x = d["kd/x"] = torch.rand(4, 1, 28, 28)
    y = d["kd/y"] = torch.randint(0, 10, (4,))
    with torch.no_grad():
        d["kd/s"], d["kd/t"] = s(x), t(x)
        # in fp64: the soft loss is a small KL (cancellation) times T^2 = 49, machine-dependent in fp32
        for i, v in enumerate(ns["distillation_loss"](s(x).double(), t(x).double(), y, 7, 0.3)):
            d[f"kd/loss{i}"] = v
    asrc = open(os.path.join(REF, "alexnet/alexnet.py")).read()
    ans = {}
    exec(compile(asrc, "alexnet.py", "exec"), ans)
    ra = use_state(d, "alexnet/", ans["AlexNet"](10).eval(), 106)
    x = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(107))   # the test redraws it
    with torch.no_grad():
        d["alexnet/y"] = ra(x)
    lns = exec_cells("attention/luong.ipynb", ["LuongAttention"])
    la = use_state(d, "luong/", lns["LuongAttention"](8), 108)
    d["luong/st"], d["luong/hs"] = torch.randn(3, 8), torch.randn(3, 5, 8)
    with torch.no_grad():
        d["luong/c"], d["luong/w"] = la(d["luong/st"], d["luong/hs"])
    return d


NB = "deepseekv3/deepseekv3.ipynb"


class _Args:
    block_size = 16
    batch_size = 2
    embeddings_dim = 64
    attn_dropout = 0.0
    vocab_size = 97
    heads = 4
    dropout = 0.0
    decoder_layers = 2
    experts = 4
    top_experts = 2
    use_shared_experts = True
    noisy_topk = False
    use_aux_free_load_balancing = True
    aux_free_bias_update_rate = 0.001
    mtp_heads = 0
    latent_dim = 16
    device = "cpu"
    ignore_pad_token_in_loss = False


def _dsv3_model(noisy):
    from torch.nn import RMSNorm
    args = type("_NoisyArgs", (_Args,), {"noisy_topk": True}) if noisy else _Args
    ns = exec_cells(NB, ["precompute_pos_embeddings", "apply_pos_embeddings", "Normalization", "swish",
                         "SWiGLUExpert", "MoeLayer", "LatentAttention", "MHLA", "DecoderLayer", "Block",
                         "DeepSeekV3"], {"modelargs": args, "RMSNorm": RMSNorm, "dataclass": dataclass})
    torch.manual_seed(0)
    ref = ns["DeepSeekV3"](embeddings_dim=64, vocab_size=97, dropout=0.0, mtp_heads=0, device="cpu")
    with torch.no_grad():
        for l in ref.decoder.decoder:
            l.moe_block.routing_bias.uniform_(-0.01, 0.01)
    return ref


def _dsv3_train_record(d, ref, x, y, noisy):
    """One training forward + backward of the reference: loss, updated routing biases, and the
    gradients the tests compare, under the tests' own names (L<layer>/...)."""
    logits = ref(x)                               # training path: MTP loop inert -> plain decoder
    loss = F.cross_entropy(logits.view(-1, 97), y.view(-1))
    loss.backward()
    d["train/loss"] = loss.detach()
    d["train/embed.grad"] = ref.decoder.embeddings.weight.grad
    for i, l in enumerate(ref.decoder.decoder):
        p = f"train/L{i}/"
        d[p + "routing_bias"] = l.moe_block.routing_bias
        d[p + "gate.grad"] = l.moe_block.gate.weight.grad
        if noisy:
            d[p + "noise.grad"] = l.moe_block.noise.weight.grad
        for h in range(4):
            rh = l.mhla.heads[h]
            d[p + f"h{h}/query.grad"] = rh.query.weight.grad
            d[p + f"h{h}/W_k.grad"] = rh.W_k.weight.grad
            d[p + f"h{h}/W_v.grad"] = rh.W_v.weight.grad
            if i == 0 and h == 0:
                d[p + f"h{h}/W_dkv.grad"] = rh.W_dkv.weight.grad
        for e in range(4):
            ex = l.moe_block.experts[e]
            if ex.w1.weight.grad is None:         # an expert no token was routed to
                continue
            for w in ("w1", "w2", "w3"):
                d[p + f"e{e}/{w}.grad"] = getattr(ex, w).weight.grad
        d[p + "shared/w1.grad"] = l.moe_block.shared_expert.w1.weight.grad


def dsv3():
    d = {}
    ref = _dsv3_model(False)
    for k, v in ref.state_dict().items():
        d["sd/" + k] = v.detach().clone()     # the training step below updates buffers in place
    x = d["x"] = torch.randint(0, 97, (2, 16), generator=torch.Generator().manual_seed(1))
    ref.eval()
    with torch.no_grad():
        d["logits"] = ref(x, inference=True)
    ref.train()
    g = torch.Generator().manual_seed(3)
    d["train/x"] = torch.randint(0, 97, (2, 16), generator=g)
    d["train/y"] = torch.randint(0, 97, (2, 16), generator=g)
    _dsv3_train_record(d, ref, d["train/x"], d["train/y"], False)
    return d


def dsv3_noisy():
    d = {}
    ref = _dsv3_model(True)
    for k, v in ref.state_dict().items():
        d["sd/" + k] = v.detach().clone()     # the training step below updates buffers in place
    g = torch.Generator().manual_seed(3)
    x = d["x"] = torch.randint(0, 97, (2, 16), generator=g)
    y = d["y"] = torch.randint(0, 97, (2, 16), generator=g)
    ref.eval()
    with torch.no_grad():
        torch.manual_seed(11)
        d["logits"] = ref(x, inference=True)
    ref.train()
    torch.manual_seed(13)
    _dsv3_train_record(d, ref, x, y, True)
    return d


def main():
    global REF
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    REF = sys.argv[1]
    torch.set_num_threads(1)
    for name, fn in [("gemma", gemma), ("vit", vit), ("ae_vae", ae_vae), ("kd_alexnet_luong", kd_alexnet_luong),
                     ("dsv3", dsv3), ("dsv3_noisy", dsv3_noisy)]:
        d = fn()
        n = G.save(name, d)
        size = sum(v.numel() * v.element_size() for v in d.values())
        print(f"{name}: {len(d)} tensors, {size / 1e6:.2f} MB in {n} part(s)")


if __name__ == "__main__":
    main()
