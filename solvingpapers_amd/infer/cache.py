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

``PagedKVCache`` (opt-in, ``page_size=`` on the drivers) replaces the [B, Tmax] rows by a pool of
fixed-size pages per layer and one block table: memory follows the tokens held. ``cache[layer]`` is then
an ``ops.attention.PagedKV`` handle.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from ..ops.attention import KV8, PagedKV, check_page_size, kv_cache_write

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


class CacheFull(RuntimeError):
    """The page pool of a :class:`PagedKVCache` cannot back the rows asked for."""


class PagedKVCache(list):
    """Paged KV cache (PagedAttention, Kwon et al., SOSP 2023): a ``list`` of ``ops.attention.PagedKV``
    layers, like :class:`KVCache`. Every layer owns two bf16 page pools [num_pages, page_size, Hkv, hd];
    ONE int32 block table [B, NP] (``NP = ceil(max_len / page_size)``), shared by all layers, maps logical
    row r of sequence b to pool row ``block_table[b, r >> lg] * page_size + (r & (page_size - 1))``, so
    memory scales with the tokens held, not with ``batch * max_len``.

    Page 0 is the null page: the allocator never hands it out and every unassigned entry is 0. A write
    to a row a slot has not reserved (an inactive row, the pad rows of a right-padded prefill) lands
    there, a read past a reservation (a contract violation) reads it; neither can fault.

    The allocator is host-side: a free list plus ``table``, a host mirror of the device table. A table
    update is a plain copy into the static device tensor outside any graph, so a captured step sees it at
    its next replay -- and does no host work itself: whatever a run of replays will write must be
    reserved before it. ``num_pages=None`` sizes the pool to ``batch * NP + 1``: nothing can run out and
    the memory is the contiguous cache's plus the null page."""

    def __init__(self, n_layers: int, batch: int, max_len: int, n_kv_heads: int, head_dim: int,
                 page_size: int = 64, num_pages: Optional[int] = None, device=None, dtype=torch.bfloat16):
        ps = check_page_size(page_size)
        if max_len < 1 or batch < 1:
            raise ValueError(f"PagedKVCache: batch {batch} and max_len {max_len} must be positive")
        NP = -(-max_len // ps)
        num_pages = batch * NP + 1 if num_pages is None else int(num_pages)
        if num_pages < 2:
            raise ValueError(f"PagedKVCache: num_pages must be at least 2 (the null page and one more), got {num_pages}")
        self.page_size, self.num_pages, self.pages_per_seq = ps, num_pages, NP
        self.batch, self.max_len, self.pos, self.quant = batch, max_len, 0, None
        self.block_table = torch.zeros(batch, NP, dtype=torch.int32, device=device)
        self.table = torch.zeros(batch, NP, dtype=torch.int32)    # host mirror
        self._held = [0] * batch                                 # pages backing each slot
        self._free = list(range(num_pages - 1, 0, -1))           # pop() hands out 1, 2, ...; never 0
        self._parent, self._b0 = None, 0
        super().__init__(
            PagedKV(torch.zeros(num_pages, ps, n_kv_heads, head_dim, device=device, dtype=dtype),
                    torch.zeros(num_pages, ps, n_kv_heads, head_dim, device=device, dtype=dtype),
                    self.block_table, ps, max_len)
            for _ in range(n_layers))

    # ---------------------------------------------------------------- allocator
    def pages_for(self, n_rows: int) -> int:
        """Pages that back rows [0, n_rows)."""
        return -(-max(int(n_rows), 0) // self.page_size)

    def held(self, b: int) -> int:
        """Pages slot ``b`` holds."""
        if self._parent is not None:
            return self._parent.held(self._slot(b))
        return self._held[self._slot(b)]

    def _slot(self, b: int) -> int:
        if not 0 <= b < self.batch:
            raise IndexError(f"slot {b} of {self.batch}")
        return b + self._b0

    def reserve(self, b: int, n_rows: int) -> None:
        """Back rows [0, n_rows) of slot ``b``. Idempotent, only ever adds pages, and copies the changed
        table row to the device. Raises :class:`CacheFull`, changing nothing, if the pool is short."""
        if self._parent is not None:
            return self._parent.reserve(self._slot(b), n_rows)
        b = self._slot(b)
        need = self.pages_for(n_rows)
        if need > self.pages_per_seq:
            raise ValueError(f"PagedKVCache.reserve: {n_rows} rows exceed the table's "
                             f"{self.pages_per_seq * self.page_size}")
        have = self._held[b]
        if need <= have:
            return
        if need - have > len(self._free):
            raise CacheFull(f"slot {b} needs {need - have} more page(s) of {self.page_size} rows for {n_rows} rows; "
                            f"{len(self._free)} of {self.num_pages - 1} are free")
        for i in range(have, need):
            self.table[b, i] = self._free.pop()
        self._held[b] = need
        self.block_table[b].copy_(self.table[b])

    def free(self, b: int) -> None:
        """Return slot ``b``'s pages to the pool and zero its table row (host and device)."""
        if self._parent is not None:
            return self._parent.free(self._slot(b))
        b = self._slot(b)
        have = self._held[b]
        if have == 0:
            return
        # pushed back in reverse, so the next reserve hands the same pages out in the same order
        self._free.extend(reversed(self.table[b, :have].tolist()))
        self.table[b].zero_()
        self._held[b] = 0
        self.block_table[b].copy_(self.table[b])

    def free_all(self) -> None:
        for b in range(self.batch):
            self.free(b)

    @property
    def pages_free(self) -> int:
        return len(self._parent._free if self._parent is not None else self._free)

    @property
    def pages_used(self) -> int:
        """Pages handed out (the null page is not counted)."""
        return self.num_pages - 1 - self.pages_free

    def nbytes(self) -> int:
        """Pools of every layer plus the device block table."""
        return sum(l.nbytes() for l in self) + self.block_table.numel() * self.block_table.element_size()

    # ---------------------------------------------------------------- KVCache's surface
    def gathered(self, layer: int, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(k, v) rows [0, n) of ``layer`` as contiguous [B, n, Hkv, hd] tensors."""
        return self[layer].gathered(n)

    def write(self, layer: int, k: torch.Tensor, v: torch.Tensor, pos: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """Store k/v [B, T, Hkv, hd] at rows [pos, pos+T) and return rows [0, pos+T), gathered."""
        T = k.shape[1]
        if pos + T > self.max_len:
            raise ValueError(f"KV cache overflow: {pos + T} > {self.max_len}")
        kv_cache_write(self[layer], k, v, pos)
        return self.gathered(layer, pos + T)

    def rows(self, b0: int, b1: int) -> "PagedKVCache":
        """A cache of views of batch rows [b0, b1): the same pools and ``block_table[b0:b1]`` (a
        contiguous slice), so one slot of a running batch can be prefilled alone. Its allocator calls go
        to this cache's, slot ``b`` of the view being slot ``b0 + b`` here."""
        if not 0 <= b0 < b1 <= self.batch:
            raise IndexError(f"PagedKVCache.rows: [{b0}, {b1}) outside the batch")
        sub = PagedKVCache.__new__(PagedKVCache)
        bt = self.block_table[b0:b1]
        list.__init__(sub, (PagedKV(l.k, l.v, bt, self.page_size, self.max_len) for l in self))
        sub.page_size, sub.num_pages, sub.pages_per_seq = self.page_size, self.num_pages, self.pages_per_seq
        sub.batch, sub.max_len, sub.pos, sub.quant = b1 - b0, self.max_len, self.pos, None
        sub.block_table, sub.table = bt, self.table[b0:b1]
        root = self._parent if self._parent is not None else self
        sub._parent, sub._b0 = root, self._b0 + b0
        sub._held = sub._free = None
        return sub


def new_kv_cache(n_layers: int, batch: int, max_len: int, n_kv_heads: int, head_dim: int, device=None,
                 dtype=torch.bfloat16, kv_cache: Optional[str] = None, page_size: Optional[int] = None,
                 num_pages: Optional[int] = None):
    """The cache behind a GQA / MQA model's ``new_cache``: a :class:`KVCache` (``kv_cache`` None / "bf16" /
    "fp8"), or with ``page_size`` a :class:`PagedKVCache` of bf16 pages (``num_pages`` None: enough for
    every slot's ``max_len``)."""
    quant = kv_cache_quant(kv_cache)
    if page_size is None:
        if num_pages is not None:
            raise ValueError("num_pages sizes a paged KV cache: pass page_size too")
        return KVCache(n_layers, batch, max_len, n_kv_heads, head_dim, device=device, dtype=dtype, quant=quant)
    check_page_size(page_size)
    if quant:
        raise NotImplementedError("only the bf16 KV cache is paged: page_size with kv_cache='fp8' (fp8 pages) is "
                                  "not implemented")
    return PagedKVCache(n_layers, batch, max_len, n_kv_heads, head_dim, page_size, num_pages, device=device,
                        dtype=dtype)
