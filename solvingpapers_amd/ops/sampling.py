"""Wrapper for csrc/kernels/sample.hip: one launch from a row of logits to a token id
(temperature, top-k, top-p, counter RNG). CPU tensors run the fp64 oracle of ops/reference.py on
the same uniforms, so a (seed, offset) pair names the same draw on either device."""
from __future__ import annotations

from typing import Optional

import torch

from . import _ext, reference

_M64 = (1 << 64) - 1


def mix32(k: int) -> int:
    """Host twin of mix32 (csrc/include/spa_rng.h)."""
    k &= _M64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _M64
    k ^= k >> 33
    return k & 0xFFFFFFFF


def u01(seed: int, i: int) -> float:
    """Host twin of u01 (csrc/include/spa_rng.h): a 24-bit uniform in (0, 1], exact in fp32."""
    return ((mix32((seed & _M64) * 0x9E3779B97F4A7C15 + i) >> 8) + 1) / float(1 << 24)


def sample_logits(logits: torch.Tensor, temperature: float = 1.0, top_k: Optional[int] = None,
                  top_p: Optional[float] = None, u: Optional[torch.Tensor] = None,
                  seed: Optional[torch.Tensor] = None, offset: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits [B, V] (fp32 / bf16, contiguous) -> ids [B, 1] int64, written into ``out`` when given.

    The uniform of row b is ``u[b]`` (fp32 [B], in (0, 1]) or ``u01(seed, offset * B + b)`` with
    ``seed`` / ``offset`` int64 [1] tensors on the logits' device: pass exactly one of the two.
    Semantics: :func:`reference.sample_logits`. ``u`` has 24 bits, so a token with less than 2^-24
    of the kept mass may never be drawn. No host sync on the GPU path (graph-capturable)."""
    if top_p is not None and not top_p > 0:
        raise ValueError("sample_logits: top_p must be > 0")
    if (u is None) == (seed is None or offset is None) or (seed is None) != (offset is None):
        raise ValueError("sample_logits: pass exactly one of u or (seed and offset)")
    if logits.is_cuda:
        return _ext.ops().sample_logits(logits, float(temperature), int(top_k or 0),
                                        1.0 if top_p is None else float(top_p), u, seed, offset, out)
    B = logits.shape[0]
    if u is None:
        s, o = int(seed.item()), int(offset.item())
        u = torch.tensor([u01(s, o * B + b) for b in range(B)], dtype=torch.float32)
    ids = reference.sample_logits(logits, temperature, top_k, top_p, u)
    if out is None:
        return ids
    out.copy_(ids.view_as(out))
    return out
