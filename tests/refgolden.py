"""Recorded results of the reference's own PyTorch code, so the parity tests run
without the reference mounted.

``oracle/make_golden.py`` executes the reference notebooks' class/function cells on CPU with the
small configs of the tests and stores, under ``tests/golden/``, the state dict the reference model
was built with, the inputs and everything the test compares (outputs, losses, gradients, updated
buffers). A golden is a flat ``{name: tensor}`` dict, split over ``<name>.pNN.pt`` files of under
1 MiB each. Where a reference state dict is too large to store (AlexNet, the KD teacher) only its
key -> shape list is stored and both sides fill it from the same seeded generator (synth_state)."""
import glob
import math
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 1000 * 1000


def load(name):
    parts = sorted(glob.glob(os.path.join(GOLDEN, f"{name}.p[0-9][0-9].pt")))
    assert parts, f"golden {name!r} missing under {GOLDEN} (python oracle/make_golden.py REFERENCE_DIR)"
    d = {}
    for p in parts:
        d.update(torch.load(p, map_location="cpu", weights_only=True))
    return d


def save(name, d):
    """Greedy, order-preserving split into parts of at most PART_BYTES of tensor data."""
    os.makedirs(GOLDEN, exist_ok=True)
    for old in glob.glob(os.path.join(GOLDEN, f"{name}.p[0-9][0-9].pt")):
        os.remove(old)
    parts, cur, size = [], {}, 0
    for k, v in d.items():
        v = v.detach().clone().contiguous()
        n = v.numel() * v.element_size()
        assert n <= PART_BYTES, (name, k, n)
        if cur and size + n > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    parts.append(cur)
    for i, p in enumerate(parts):
        torch.save(p, os.path.join(GOLDEN, f"{name}.p{i:02d}.pt"))
    return len(parts)


def sub(d, prefix):
    return {k[len(prefix):]: v for k, v in d.items() if k.startswith(prefix)}


def synth_state(shapes, seed):
    """A state dict for ``{key: shape}`` from one seeded generator: uniform in +-1/sqrt(fan_in) for
    matrices and filters, +-0.05 for vectors (no zero biases). Float32 entries only."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in shapes.items():
        shape = tuple(int(s) for s in shape)
        bound = 1.0 / math.sqrt(math.prod(shape[1:])) if len(shape) >= 2 else 0.05
        sd[k] = (torch.rand(shape, generator=g) * 2 - 1) * bound
    return sd


def put_state(d, prefix, sd, seed):
    """Record ``sd`` under ``prefix`` (generator side): the tensors themselves if they fit in one
    part, else the shapes only; returns the state dict the reference model must then use."""
    d[f"{prefix}n_state"] = torch.tensor(len(sd))
    total = sum(v.numel() * v.element_size() for v in sd.values())
    if total <= PART_BYTES:
        for k, v in sd.items():
            d[f"{prefix}sd/{k}"] = v.detach().clone()
        return dict(sd)
    assert all(v.dtype == torch.float32 for v in sd.values()), prefix
    for k, v in sd.items():
        d[f"{prefix}shape/{k}"] = torch.tensor(list(v.shape), dtype=torch.int64)
    return synth_state({k: v.shape for k, v in sd.items()}, seed)


def get_state(d, prefix, seed):
    """The state dict recorded by put_state (test side)."""
    sd = sub(d, f"{prefix}sd/")
    if not sd:
        sd = synth_state({k: v.tolist() for k, v in sub(d, f"{prefix}shape/").items()}, seed)
    assert len(sd) == int(d[f"{prefix}n_state"]), prefix      # 0: a module without parameters
    return sd
