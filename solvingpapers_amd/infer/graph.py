"""HIP-graph decode: one captured launch per generated token.

A KV-cached decode step of LLaMA3-8B is ~450 short kernels (32 layers x norms, four
projections, RoPE, cache writes, decode attention, GLU) whose launch cost exceeds their
run time at batch 1. ``GraphDecoder`` captures one step with every position-dependent
value on the device:

* ``DecodeState.index``     -- the cache row written this step (long [1]);
* ``DecodeState.positions`` -- RoPE positions (int32 [B, 1]);
* ``DecodeState.kv_len``    -- valid cache rows (int32 [1]) read by the decode kernel.

The captured step ends by advancing that state on the device, and greedy sampling
(argmax into the static token buffer) is captured too, so ``n`` tokens are ``n`` graph
replays with no host work in between. With a ``Sampler`` (infer/sampling.py) the captured step
ends in the fused sampling kernel instead (temperature / top-k / top-p from a device-resident
counter RNG, written into the same token buffer): non-greedy generation is ``n`` replays too.
Without one, non-greedy sampling runs eagerly on the replay's logits between replays
(torch.multinomial).

``GraphDecoder(ragged=True)`` captures the same step over a ``RaggedDecodeState``: the three
tensors hold one entry per sequence (``index`` long [B], ``kv_len`` int32 [B]), the kernels read
entry b for sequence b, so right-padded prompts of different lengths decode together and
``prefill_row`` puts a new prompt into one slot while the others continue.

``GraphDecoder(page_size=N)`` decodes from a paged KV cache (infer/cache.py PagedKVCache): the captured
step writes and reads cache rows through a block table that lives in one static device tensor.
``reserve`` / ``free`` change it from the host between replays; a replay does no host work, so every row
a run of replays will write must be reserved before the run.

Protocol a model implements: ``new_cache(B, max_len)``, ``step(ids, cache, pos)`` (eager
prefill; ``last=`` for a ragged one) and ``step_graph(ids, cache, state)`` (graph-safe decode
step: no host syncs).
"""
from __future__ import annotations

from typing import Optional

import torch

from .sampling import sample


class DecodeState:
    """Device-resident position state of a captured decode step (batch-uniform positions)."""

    per_row = False   # one position for the whole batch; RaggedDecodeState: one per sequence

    def __init__(self, batch: int, max_len: int, device):
        self.batch, self.max_len = batch, max_len
        self.index = torch.zeros(1, dtype=torch.long, device=device)
        self.positions = torch.zeros(batch, 1, dtype=torch.int32, device=device)
        self.kv_len = torch.ones(1, dtype=torch.int32, device=device)

    def set(self, pos: int):
        """Host-side (re)position, outside the graph: the next step writes cache row ``pos``."""
        self.index.fill_(pos)
        self.positions.fill_(pos)
        self.kv_len.fill_(pos + 1)

    def advance(self):
        """Device-side increment (captured at the end of the step)."""
        self.index.add_(1)
        self.positions.add_(1)
        self.kv_len.add_(1)


class RaggedDecodeState(DecodeState):
    """Per-sequence positions (ragged batch: prompts of different lengths, slot reuse): ``index`` long
    [B], ``positions`` int32 [B, 1], ``kv_len`` int32 [B]; the kernels read entry b for sequence b
    (``per_row``). ``active`` int32 [B] (ones) is what ``advance`` adds: a row with ``active[b] = 0``
    stays where it is and recomputes its current position at every step -- its logits are unspecified
    (finite), it rewrites only its own cache row, and it never touches another row's cache."""

    per_row = True

    def __init__(self, batch: int, max_len: int, device):
        self.batch, self.max_len = batch, max_len
        self.index = torch.zeros(batch, dtype=torch.long, device=device)
        self.positions = torch.zeros(batch, 1, dtype=torch.int32, device=device)
        self.kv_len = torch.ones(batch, dtype=torch.int32, device=device)
        self.active = torch.ones(batch, dtype=torch.int32, device=device)

    def set(self, pos):
        """Host-side (re)position of every row: an int, or one position per sequence (tensor / sequence
        of length B). Row b's next step writes cache row ``pos[b]``."""
        if isinstance(pos, int):
            return super().set(pos)
        p = torch.as_tensor(pos, device=self.index.device).reshape(-1).long()
        if p.numel() != self.batch:
            raise ValueError(f"RaggedDecodeState.set: {p.numel()} positions for a batch of {self.batch}")
        self.index.copy_(p)
        self.positions.copy_(p[:, None])
        self.kv_len.copy_(p + 1)

    def set_row(self, b: int, pos: int):
        """(Re)position sequence ``b`` alone (a new prompt in a freed slot); the others keep theirs."""
        self.index[b:b + 1].fill_(pos)
        self.positions[b:b + 1].fill_(pos)
        self.kv_len[b:b + 1].fill_(pos + 1)

    def advance(self):
        """Device-side increment of the active rows (captured at the end of the step)."""
        self.index.add_(self.active)
        self.positions.add_(self.active[:, None])
        self.kv_len.add_(self.active)


class ExtendState(RaggedDecodeState):
    """A :class:`RaggedDecodeState` for ONE multi-token step (``model.extend``): sequence b's ``T`` tokens
    take cache rows [starts[b], starts[b] + T). ``index`` long [B] = starts, ``positions`` int32 [B, T] =
    starts[:, None] + arange(T), ``kv_len`` int32 [B] = starts + T. ``starts`` (host list or tensor) is
    checked on the host: 0 <= starts[b] and starts[b] + T <= max_len, so kv_len[b] never exceeds the
    cache's rows and every token sits at the position stated."""

    def __init__(self, starts, T: int, max_len: int, device):
        s = torch.as_tensor(starts).reshape(-1).long().cpu()
        T = int(T)
        if T < 1:
            raise ValueError(f"ExtendState: a step of {T} tokens")
        if s.numel() < 1:
            raise ValueError("ExtendState: starts is empty")
        if int(s.min()) < 0 or int(s.max()) + T > max_len:
            raise ValueError(f"ExtendState: rows [start, start + {T}) must lie in [0, {max_len}], got starts "
                             f"{s.tolist()}")
        self.batch, self.max_len, self.T = s.numel(), max_len, T
        self.index = s.to(device)
        self.positions = (self.index[:, None] + torch.arange(T, device=device)[None]).int()
        self.kv_len = (self.index + T).int()
        self.active = torch.ones(self.batch, dtype=torch.int32, device=device)


EXTEND_UNSUPPORTED = ("multi-token steps behind a live cache (extend, extend_row, chunked prefill) cover LLaMA3 and "
                      "Gemma; {} has no extend()")


def _need_extend(model):
    if not hasattr(model, "extend"):
        raise NotImplementedError(EXTEND_UNSUPPORTED.format(type(model).__name__))


def check_chunk(chunk) -> int:
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"chunk must be a positive int, got {chunk!r}")
    return chunk


def chunked_prefill(model, cache, ids: torch.Tensor, lens: torch.Tensor, chunk: int) -> torch.Tensor:
    """Right-padded prompts ``ids`` [B, T0] (``lens`` long [B] real tokens each) into rows [0, T0) of
    ``cache`` in blocks of ``chunk`` columns: the first through ``model.step`` at position 0, each later
    one through ``model.extend`` at ``starts = [chunk * i] * B``. Returns logits [B, V], sequence b's
    taken from the chunk that holds its last real token; chunks wholly past every length are skipped."""
    chunk = check_chunk(chunk)
    _need_extend(model)
    B, T0 = ids.shape
    out = None
    for c0 in range(0, int(lens.max()), chunk):
        c1 = min(c0 + chunk, T0)
        last = (lens - 1 - c0).clamp(0, c1 - c0 - 1)
        if c0 == 0:
            lg = model.step(ids[:, :c1], cache, 0, last=last)
        else:
            lg = model.extend(ids[:, c0:c1], cache, [c0] * B, last=last)
        here = (lens > c0) & (lens <= c1)
        out = lg if out is None else torch.where(here[:, None], lg, out)
    return out


def extend_row(model, cache, state, b: int, ids: torch.Tensor, reserve: Optional[int] = None) -> torch.Tensor:
    """Append ``ids`` (1-D) behind slot ``b``'s current position (read on the host from ``state.index[b]``,
    a synchronisation) through the batch-row views ``cache.rows(b, b + 1)`` and ``model.extend``, then
    position the slot behind them; the other slots keep their rows and positions. Returns the logits [V]
    of the last appended token. Paged cache: ``max(pos + len(ids), reserve)`` rows are reserved first
    (only ever adds pages); ``CacheFull`` is raised before anything changes."""
    if not getattr(state, "per_row", False):
        raise ValueError("extend_row needs per-sequence positions (GraphDecoder(ragged=True)): the uniform state "
                         "holds one position")
    _need_extend(model)
    if not 0 <= b < state.batch:
        raise IndexError(f"slot {b} of {state.batch}")
    ids = ids.reshape(1, -1)
    T = ids.shape[1]
    pos = int(state.index[b])
    if T < 1 or pos + T >= state.max_len:
        raise ValueError(f"{T} tokens behind position {pos} do not fit a {state.max_len}-token cache")
    if hasattr(cache, "block_table"):
        cache.reserve(b, max(pos + T, int(reserve or 0)))
    lg = model.extend(ids, cache.rows(b, b + 1), [pos])
    state.set_row(b, pos + T)
    return lg[0]


def ragged_layout(ids: torch.Tensor, lens: torch.Tensor, new: torch.Tensor, pad_token_id: int) -> torch.Tensor:
    """[B, T0 + n]: row b = its prompt ids[b, :lens[b]], its n new tokens from column lens[b], then
    ``pad_token_id`` (the output layout of ragged generation)."""
    B, T0 = ids.shape
    n = new.shape[1]
    out = torch.full((B, T0 + n), pad_token_id, dtype=ids.dtype, device=ids.device)
    out[:, :T0] = torch.where(torch.arange(T0, device=ids.device)[None] < lens[:, None], ids, out[:, :T0])
    return out.scatter_(1, lens[:, None] + torch.arange(n, device=ids.device)[None], new.to(ids.dtype))


def check_prompt_lens(prompt_lens, B: int, T0: int, device) -> torch.Tensor:
    """``prompt_lens`` (tensor or sequence) as a long [B] tensor on ``device``, 1 <= len_b <= T0."""
    lens = torch.as_tensor(prompt_lens).reshape(-1).long()
    if lens.numel() != B:
        raise ValueError(f"prompt_lens: {lens.numel()} lengths for a batch of {B}")
    if int(lens.min()) < 1 or int(lens.max()) > T0:
        raise ValueError(f"prompt_lens must lie in [1, {T0}] (ids are right-padded to {T0}), got {lens.tolist()}")
    return lens.to(device)


RAGGED_UNSUPPORTED = ("ragged batches (per-sequence positions) cover the RoPE models with a (k, v) cache, LLaMA3 and "
                      "Gemma; {} is not covered")


class GraphDecoder:
    def __init__(self, model, batch: int, max_len: int, greedy: bool = True, warmup: int = 2, sampler=None,
                 kv_cache: Optional[str] = None, ragged: bool = False, page_size: Optional[int] = None,
                 num_pages: Optional[int] = None):
        """``ragged=True`` captures the step over a :class:`RaggedDecodeState`: every sequence at its own
        position (prompts of different lengths, ``prefill_row`` to refill one slot mid-stream).

        ``page_size`` (with or without ``ragged``): a paged KV cache of ``num_pages`` pages per layer
        (None: enough for every slot's ``max_len``). ``prefill`` / ``prefill_row`` / ``generate`` reserve
        the rows they are about to write; a caller that replays the graph itself reserves with
        :meth:`reserve` BEFORE the replays -- a replay does no host work, and a row written without a
        reservation lands in the null page and is lost."""
        self.model, self.batch, self.max_len, self.greedy = model, batch, max_len, greedy
        self.ragged = ragged
        dev = next(model.parameters()).device
        self.sampler = sampler.to(dev) if sampler is not None else None
        # kv_cache="fp8": the captured step quantises its K/V row and attends over e4m3 rows
        kw = {} if kv_cache is None else {"kv_cache": kv_cache}
        if page_size is not None or num_pages is not None:
            kw.update(page_size=page_size, num_pages=num_pages)
        self.cache = model.new_cache(batch, max_len, **kw)
        self.paged = page_size is not None
        self.state = RaggedDecodeState(batch, max_len, dev) if ragged else DecodeState(batch, max_len, dev)
        self.ids = torch.zeros(batch, 1, dtype=torch.long, device=dev)
        self.logits: Optional[torch.Tensor] = None
        self._capture(warmup)

    def _body(self):
        lg = self.model.step_graph(self.ids, self.cache, self.state)
        if self.sampler is not None:
            self.sampler(lg, out=self.ids)
        elif self.greedy:
            self.ids.copy_(lg.argmax(-1, keepdim=True))
        self.state.advance()
        return lg

    @torch.no_grad()
    def _capture(self, warmup):
        # warm-up outside the capture (lazy allocations, library handles, RoPE tables); it
        # scribbles on the first cache rows and advances the state, both reset by prefill()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._body()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.state.set(0)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.logits = self._body()
        self.state.set(0)
        if self.sampler is not None:   # the warm-up calls consumed offsets; the stream starts at 0
            self.sampler.offset.zero_()

    # ---------------------------------------------------------------- paged cache
    def reserve(self, b: int, n_rows: int) -> None:
        """Back rows [0, n_rows) of slot ``b`` (paged cache): idempotent, only adds pages; ``CacheFull``
        changes nothing. Whatever the coming replays write must be reserved before them."""
        self._paged_only("reserve")
        self.cache.reserve(b, n_rows)

    def free(self, b: int) -> None:
        """Return slot ``b``'s pages to the pool (paged cache). The slot's position is the caller's: park
        it with ``state.active[b] = 0`` or refill it with ``prefill_row``."""
        self._paged_only("free")
        self.cache.free(b)

    def _paged_only(self, what):
        if not self.paged:
            raise ValueError(f"GraphDecoder.{what}: the decoder was built without page_size")

    def _reserve_all(self, rows) -> None:
        """Free every slot and back ``rows[b]`` rows of each; all or nothing (CacheFull before any change)."""
        from .cache import CacheFull
        need = sum(self.cache.pages_for(r) for r in rows)
        if need > self.cache.num_pages - 1:
            raise CacheFull(f"{len(rows)} sequences of {list(rows)} rows need {need} pages of "
                            f"{self.cache.page_size} rows; the pool holds {self.cache.num_pages - 1}")
        self.cache.free_all()
        for b, r in enumerate(rows):
            self.cache.reserve(b, r)

    @torch.no_grad()
    def prefill(self, ids: torch.Tensor, prompt_lens=None, reserve=None, chunk: Optional[int] = None) -> torch.Tensor:
        """Eager prompt pass: fills cache rows [0, T0), positions the state at T0 and returns
        the last position's logits. ``prompt_lens`` (``ragged=True`` only): ``ids`` is right-padded,
        sequence b has ``prompt_lens[b]`` real tokens; its logits are those of its last real token and
        its state is positioned at ``prompt_lens[b]`` (the pad rows the pass wrote into the cache lie
        beyond kv_len and are overwritten as the sequence grows). Paged cache: every slot is freed and
        each prompt's rows are reserved (``reserve``: that many rows per slot instead, a list, for the
        tokens to come); a short prompt's pad rows go to the null page.

        ``chunk=C`` (with ``prompt_lens``): the prompt runs in blocks of C columns, the first at position
        0 as without it, each later one through ``model.extend`` (:func:`chunked_prefill`), which bounds
        the activation memory of a long prompt. None: one pass."""
        T0 = ids.shape[1]
        if chunk is not None:
            check_chunk(chunk)
            if prompt_lens is None:
                raise ValueError("GraphDecoder.prefill: chunk needs prompt_lens (and ragged=True): a chunk behind the "
                                 "first is a per-sequence multi-token step")
            _need_extend(self.model)
        if T0 >= self.max_len:
            raise ValueError(f"prompt of {T0} tokens leaves no room in a {self.max_len}-token cache")
        if prompt_lens is not None and not self.ragged:
            raise ValueError("GraphDecoder: prompt_lens needs ragged=True (the uniform state holds one position)")
        lens = None if prompt_lens is None else check_prompt_lens(prompt_lens, self.batch, T0, ids.device)
        if self.paged:
            held = [T0] * self.batch if lens is None else lens.tolist()
            self._reserve_all(held if reserve is None else [max(h, int(r)) for h, r in zip(held, reserve)])
        if self.ragged:
            self.state.active.fill_(1)   # a batch prefill restarts every slot
        if prompt_lens is None:
            lg = self.model.step(ids, self.cache, 0)
            self.state.set(T0)
            return lg
        if chunk is not None:
            lg = chunked_prefill(self.model, self.cache, ids, lens, chunk)
        else:
            lg = self.model.step(ids, self.cache, 0, last=lens - 1)
        self.state.set(lens)
        return lg

    @torch.no_grad()
    def prefill_row(self, b: int, ids: torch.Tensor, reserve: Optional[int] = None,
                    chunk: Optional[int] = None) -> torch.Tensor:
        """Prefill one sequence (``ids`` 1-D) into slot ``b`` while the other slots keep their cache
        rows and positions (``ragged=True``): the prompt runs through the batch-row views
        ``cache.rows(b, b + 1)`` and ``state.set_row`` positions the slot behind it. Returns the
        prompt's last-position logits [V]; feeding the next token (``self.ids[b]``) and
        ``state.active[b]`` are the caller's. Paged cache: slot ``b`` is freed and ``max(len(ids),
        reserve)`` rows are reserved for it (``reserve``: the prompt plus the tokens the coming replays
        will add); ``CacheFull`` leaves the slot as it was. ``chunk``: as :meth:`prefill`."""
        if not self.ragged:
            raise ValueError("GraphDecoder: prefill_row needs ragged=True")
        if chunk is not None:
            check_chunk(chunk)
            _need_extend(self.model)
        if not 0 <= b < self.batch:
            raise IndexError(f"slot {b} of {self.batch}")
        ids = ids.reshape(1, -1)
        T = ids.shape[1]
        if not 1 <= T < self.max_len:
            raise ValueError(f"prompt of {T} tokens does not fit a {self.max_len}-token cache")
        if self.paged:
            from .cache import CacheFull
            rows = max(T, int(reserve or 0))
            if self.cache.pages_for(rows) > self.cache.pages_free + self.cache.held(b):
                raise CacheFull(f"slot {b} needs {self.cache.pages_for(rows)} pages for {rows} rows; "
                                f"{self.cache.pages_free} are free and it holds {self.cache.held(b)}")
            self.cache.free(b)
            self.cache.reserve(b, rows)
        if chunk is not None:
            lg = chunked_prefill(self.model, self.cache.rows(b, b + 1), ids,
                                 torch.full((1,), T, dtype=torch.long, device=ids.device), chunk)
        else:
            lg = self.model.step(ids, self.cache.rows(b, b + 1), 0)
        self.state.set_row(b, T)
        return lg[0]

    @torch.no_grad()
    def extend_row(self, b: int, ids: torch.Tensor, reserve: Optional[int] = None) -> torch.Tensor:
        """Append ``ids`` (1-D) behind slot ``b``'s current position between replays (a new turn of a live
        sequence) without re-running its history; the other slots keep their rows and positions
        (``ragged=True``). Returns the last appended token's logits [V]; feeding the next token
        (``self.ids[b]``) is the caller's. See :func:`extend_row`."""
        if not self.ragged:
            raise ValueError("GraphDecoder: extend_row needs ragged=True (the uniform state holds one position)")
        return extend_row(self.model, self.cache, self.state, b, ids, reserve)

    @torch.no_grad()
    def generate(self, ids: torch.Tensor, max_new_tokens: int, temperature: float = 1.0, top_k=None,
                 top_p=None, generator=None, stats=None, prompt_lens=None, pad_token_id: int = 0,
                 prefill_chunk: Optional[int] = None) -> torch.Tensor:
        """``prompt_lens`` (``ragged=True``): right-padded prompts of different lengths; returns
        [B, T0 + n] with row b = its prompt, its n new tokens from column ``prompt_lens[b]``, then
        ``pad_token_id``. ``prefill_chunk``: :meth:`prefill`'s ``chunk`` (needs ``prompt_lens``)."""
        import time
        if prefill_chunk is not None and prompt_lens is None:
            raise ValueError("GraphDecoder.generate: prefill_chunk needs prompt_lens (a ragged batch)")
        if self.sampler is not None and (temperature != 1.0 or top_k is not None or top_p is not None
                                         or generator is not None):
            raise ValueError("GraphDecoder: the captured sampler fixes temperature / top_k / top_p and draws from "
                             "its own counter RNG; per-call sampling arguments cannot apply")
        if stats is not None:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        lens = None
        if prompt_lens is not None:
            lens = check_prompt_lens(prompt_lens, self.batch, ids.shape[1], ids.device)
        # the i-th replay writes cache row len + i of every sequence: the longest prompt sets the room
        n = min(max_new_tokens, self.max_len - (ids.shape[1] if lens is None else int(lens.max())) + 1)
        # paged cache: each row's len + n rows are reserved before the replay loop (a pool too small raises
        # CacheFull here, before the cache or the positions change)
        held = [ids.shape[1]] * self.batch if lens is None else lens.tolist()
        lg = self.prefill(ids, lens, reserve=[min(h + n, self.max_len) for h in held] if self.paged else None,
                          chunk=prefill_chunk)
        if stats is not None:
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = torch.empty(self.batch, n, dtype=torch.long, device=ids.device)
        if self.sampler is not None:
            self.sampler(lg, out=self.ids)   # the first token: same kernel, next offset of the stream
        elif self.greedy:
            self.ids.copy_(lg.argmax(-1, keepdim=True))
        else:
            self.ids.copy_(sample(lg, temperature, top_k, False, generator, top_p))
        for i in range(n):
            out[:, i:i + 1].copy_(self.ids)
            if i + 1 == n:
                break
            self.graph.replay()  # feeds the token at row T0 + i; greedy / the sampler leave the next one in self.ids
            if self.sampler is None and not self.greedy:
                self.ids.copy_(sample(self.logits, temperature, top_k, False, generator, top_p))
        if stats is not None:
            torch.cuda.synchronize()
            stats.cached = True
            stats.prompt_tokens += ids.numel() if lens is None else int(lens.sum())
            stats.new_tokens += self.batch * n
            stats.prefill_s += t1 - t0
            stats.decode_s += time.perf_counter() - t1
        if lens is not None:
            return ragged_layout(ids, lens, out, pad_token_id)
        return torch.cat([ids, out], 1)
