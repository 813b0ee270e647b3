"""Preallocated per-layer KV cache for GQA / MQA decoding.

One [B, Tmax, Hkv, hd] buffer per layer for K and for V, allocated once for the whole
generation (HBM is 288 GB per MI355X: a LLaMA3-8B cache at 8K tokens is 1 GB per
sequence), written in place at the current position and read as strided views by the
decode kernel -- no concatenation per token (the reference's unused cache path,
llama3/LLaMA-jax.ipynb:816-819, concatenates).

``quant="fp8"`` (opt-in) keeps K and V as OCP e4m3 bytes in the same [B, Tmax, Hkv, hd] layout
plus one E8M0 power-of-two scale byte per (batch, kv head, token) in [B, Hkv, Tmax]: half the
bytes a decode step streams and half the memory (plus 1 / hd for the scales). What is quantised is
the value the bf16 cache would hold (RoPE'd K rounded to the model dtype, raw V), so the fp8 cache
is bitwise ``reference.quant_kv8`` of the bf16 cache; ``cache[layer]`` is then an
``ops.attention.KV8`` handle, which ``kv_cache_write`` / ``kv_cache_attend`` take in place of the
``(k, v)`` pair.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from ..ops.attention import KV8, kv_cache_write

KV_CACHE_FORMATS = (None, "bf16", "fp8")


def kv_cache_quant(kv_cache: Optional[str]) -> Optional[str]:
    """The ``kv_cache=`` argument of the drivers (None / "bf16": the model-dtype cache; "fp8") as
    KVCache's ``quant``."""
    if kv_cache not in KV_CACHE_FORMATS:
        raise ValueError(f"kv_cache must be one of {KV_CACHE_FORMATS}, got {kv_cache!r}")
    return "fp8" if kv_cache == "fp8" else None


class KVCache(list):
    """``list`` of (k, v) pairs so models can index ``cache[layer]`` directly (``quant="fp8"``: of
    KV8 handles)."""

    def __init__(self, n_layers: int, batch: int, max_len: int, n_kv_heads: int, head_dim: int,
                 device=None, dtype=torch.bfloat16, quant: Optional[str] = None):
        if quant not in (None, "fp8"):
            raise ValueError(f"KVCache: quant must be None or 'fp8', got {quant!r}")
        if quant == "fp8":
            super().__init__(KV8.zeros(batch, max_len, n_kv_heads, head_dim, device=device, dtype=dtype)
                             for _ in range(n_layers))
        else:
            super().__init__(
                (torch.zeros(batch, max_len, n_kv_heads, head_dim, device=device, dtype=dtype),
                 torch.zeros(batch, max_len, n_kv_heads, head_dim, device=device, dtype=dtype))
                for _ in range(n_layers))
        self.max_len = max_len
        self.pos = 0
        self.quant = quant

    def write(self, layer: int, k: torch.Tensor, v: torch.Tensor, pos: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Store k/v [B, T, Hkv, hd] at [pos, pos+T) and return the [0, pos+T) views (fp8: the
        dequantised rows)."""
        T = k.shape[1]
        if pos + T > self.max_len:
            raise ValueError(f"KV cache overflow: {pos + T} > {self.max_len}")
        if self.quant:
            kv_cache_write(self[layer], k, v, pos)
            return self.dequantized(layer, pos + T)
        kc, vc = self[layer]
        kc[:, pos:pos + T] = k
        vc[:, pos:pos + T] = v
        return kc[:, :pos + T], vc[:, :pos + T]

    def dequantized(self, layer: int, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(k, v) rows [0, n) of ``layer`` in the model dtype."""
        if self.quant:
            return self[layer].dequantized(n)
        kc, vc = self[layer]
        return kc[:, :n], vc[:, :n]

    def rows(self, b0: int, b1: int) -> "KVCache":
        """A cache of views of batch rows [b0, b1) (per layer the ``(k, v)`` slices, or a KV8 of the
        data and scale slices): what ``model.step`` writes through it lands in this cache, so one slot
        of a running batch can be prefilled alone."""
        if not 0 <= b0 < b1 <= (self[0].kq if self.quant else self[0][0]).shape[0]:
            raise IndexError(f"KVCache.rows: [{b0}, {b1}) outside the batch")
        sub = KVCache.__new__(KVCache)
        if self.quant:
            list.__init__(sub, (KV8(l.kq[b0:b1], l.ks[b0:b1], l.vq[b0:b1], l.vs[b0:b1], l.dtype) for l in self))
        else:
            list.__init__(sub, ((k[b0:b1], v[b0:b1]) for k, v in self))
        sub.max_len, sub.pos, sub.quant = self.max_len, self.pos, self.quant
        return sub

    def nbytes(self) -> int:
        if self.quant:
            return sum(l.nbytes() for l in self)
        return sum(k.numel() * k.element_size() * 2 for k, _ in self)

    @staticmethod
    def layers(cache) -> List:
        return list(cache)
