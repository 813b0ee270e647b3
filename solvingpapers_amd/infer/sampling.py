"""Token sampling: greedy / categorical / top-k / top-p, with temperature.

Covers every sampler of the reference: greedy argmax (gpt/gpt-jax.ipynb:827), categorical
at T = 1 (llama3/LLaMA-jax.ipynb:508), softmax + multinomial (gemma/gemma.ipynb:620-622)
and top-k + temperature (deepseekv3/deepseekv3.ipynb:1861-1866); nucleus (top-p) is an
addition. Everything stays on the device: no ``.item()`` per token.
"""
from __future__ import annotations

from typing import Optional

import torch


def sample(logits: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None,
           greedy: bool = False, generator: Optional[torch.Generator] = None,
           top_p: Optional[float] = None) -> torch.Tensor:
    """logits [B, V] -> next ids [B, 1]."""
    if greedy:
        return logits.argmax(-1, keepdim=True)
    logits = logits.float() / max(temperature, 1e-6)
    if top_k is not None:
        v, ix = torch.topk(logits, min(int(top_k), logits.shape[-1]), dim=-1)
        if top_p is not None:
            v = _nucleus(v, top_p)
        p = torch.softmax(v, dim=-1)
        j = torch.multinomial(p, 1, generator=generator)
        return ix.gather(-1, j)
    if top_p is not None:
        v, ix = torch.sort(logits, dim=-1, descending=True)
        p = torch.softmax(_nucleus(v, top_p), dim=-1)
        return ix.gather(-1, torch.multinomial(p, 1, generator=generator))
    p = torch.softmax(logits, dim=-1)
    return torch.multinomial(p, 1, generator=generator)


def _nucleus(sorted_logits: torch.Tensor, top_p: float) -> torch.Tensor:
    """Mask (to -inf) the tail of descending-sorted logits beyond cumulative mass top_p;
    the first token is always kept."""
    p = torch.softmax(sorted_logits, dim=-1)
    cum = p.cumsum(-1)
    drop = (cum - p) > top_p
    return sorted_logits.masked_fill(drop, float("-inf"))


class Sampler:
    """Device-resident sampler: temperature / top-k / top-p with a counter RNG, one launch per call
    (csrc/kernels/sample.hip on the GPU, the fp64 oracle ops.reference.sample_logits on the CPU).

    Row b of the n-th call after ``reseed(seed)`` draws with ``u01(seed, n * B + b)``
    (ops.sampling.u01), whatever the device: sampled generation is reproducible, and the call makes no
    host sync, so it can be captured in a HIP graph (``GraphDecoder(..., sampler=...)``): ``seed`` and
    ``offset`` live in int64 [1] tensors that the kernel reads and ``__call__`` advances on the device.
    Semantics of the filters: ops.reference.sample_probs. ``u`` has 24 bits: a token with less than
    2^-24 of the kept mass may never be drawn."""

    def __init__(self, temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                 seed: int = 0, device=None):
        if top_p is not None and not top_p > 0:
            raise ValueError("Sampler: top_p must be > 0")
        self.temperature, self.top_k, self.top_p = float(temperature), top_k, top_p
        self.seed = torch.full((1,), int(seed), dtype=torch.int64, device=device)
        self.offset = torch.zeros(1, dtype=torch.int64, device=device)

    def to(self, device) -> "Sampler":
        """Move the counters (host-side; outside a graph)."""
        self.seed, self.offset = self.seed.to(device), self.offset.to(device)
        return self

    def reseed(self, seed: int, offset: int = 0) -> "Sampler":
        """Host-side restart of the stream (outside a graph): the tensors a captured graph reads
        are refilled in place."""
        self.seed.fill_(int(seed))
        self.offset.fill_(int(offset))
        return self

    def __call__(self, logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """logits [B, V] -> ids [B, 1] (into ``out`` when given); then offset += 1 on the device."""
        from ..ops.sampling import sample_logits
        if self.seed.device != logits.device:
            self.to(logits.device)
        ids = sample_logits(logits.contiguous(), self.temperature, self.top_k, self.top_p,
                            seed=self.seed, offset=self.offset, out=out)
        self.offset.add_(1)
        return ids
