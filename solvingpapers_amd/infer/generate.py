"""Generic autoregressive generation driver.

Protocol a model implements for cached decoding:
  ``new_cache(batch, max_len)``  -> cache object (KVCache or the model's latent cache)
  ``step(ids, cache, pos)``      -> logits [B, V] of the LAST position of ``ids``, after
                                    writing ``ids``' keys/values at cache rows [pos, pos+T)
  ``max_context`` (attribute, optional) -> the longest sequence the model accepts
  ragged batches (``prompt_lens=``) also need ``step(..., last=)`` (logits at row last[b] of each
  sequence), ``step_graph(ids, cache, state)`` and the class attribute ``ragged_decode = True``

The first call is the prompt prefill (flash attention over the whole prompt), every later
call feeds one token per sequence (split-K decode attention). Models without the protocol
(the reference-exact GPT / Gemma presets, whose notebooks crop to ``block_size`` and
re-run the window) are driven by re-forwarding the cropped window, as the reference does
(gpt/gpt-jax.ipynb:821-829, gemma/gemma.ipynb:608-630).
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Optional

import torch

from .sampling import sample


@dataclass
class GenerationStats:
    prompt_tokens: int = 0
    new_tokens: int = 0
    prefill_s: float = 0.0
    decode_s: float = 0.0
    cached: bool = False

    @property
    def decode_tok_s(self) -> float:
        """Generated tokens per second over the decode phase (all sequences)."""
        return self.new_tokens / self.decode_s if self.decode_s > 0 else 0.0

    @property
    def prefill_tok_s(self) -> float:
        return self.prompt_tokens / self.prefill_s if self.prefill_s > 0 else 0.0


def _sync(t: torch.Tensor):
    if t.is_cuda:
        torch.cuda.synchronize(t.device)


def _new_cache(model, B, total, kv_cache, page_size, num_pages):
    """The model's cache for ``total`` rows; ``page_size`` / ``num_pages`` only reach models asked for a paged
    one (their ``new_cache`` names itself in a NotImplementedError when it has none)."""
    kw = {}
    if kv_cache is not None:
        kw["kv_cache"] = kv_cache
    if page_size is not None or num_pages is not None:
        kw.update(page_size=page_size, num_pages=num_pages)
    return model.new_cache(B, total, **kw)


def _reserve(cache, rows):
    """Back ``rows[b]`` rows of every slot of a paged cache before the first launch; all or nothing
    (CacheFull with no page taken when the pool cannot hold them all)."""
    from .cache import CacheFull
    need = sum(cache.pages_for(r) for r in rows)
    if need > cache.pages_free + cache.pages_used:
        raise CacheFull(f"{len(rows)} sequences of {list(rows)} rows need {need} pages of {cache.page_size} rows; the "
                        f"pool holds {cache.num_pages - 1} (plus the null page)")
    for b, r in enumerate(rows):
        cache.reserve(b, r)


def _generate_ragged(model, ids, prompt_lens, pad_token_id, max_new_tokens, temperature, top_k, top_p, greedy,
                     eos_token_id, generator, st, timed, sampler, kv_cache, page_size=None, num_pages=None,
                     prefill_chunk=None):
    """Ragged batch: one right-padded prefill whose logits are gathered at each sequence's last real
    token (causal attention keeps real tokens independent of the pads to their right), then
    ``step_graph`` run eagerly on a RaggedDecodeState positioned at ``prompt_lens``: sequence b writes
    cache row len_b + i at step i (over the pad rows the prefill left there) and attends over its own
    kv_len[b] rows."""
    from .graph import (EXTEND_UNSUPPORTED, RAGGED_UNSUPPORTED, RaggedDecodeState, check_chunk, check_prompt_lens,
                        chunked_prefill, ragged_layout)
    if not getattr(model, "ragged_decode", False):
        raise NotImplementedError(RAGGED_UNSUPPORTED.format(type(model).__name__))
    if prefill_chunk is not None:
        check_chunk(prefill_chunk)
        if not hasattr(model, "extend"):
            raise NotImplementedError(EXTEND_UNSUPPORTED.format(type(model).__name__))
    B, T0 = ids.shape
    lens = check_prompt_lens(prompt_lens, B, T0, ids.device)
    longest = int(lens.max())
    total = T0 + max_new_tokens
    limit = getattr(model, "max_context", None)
    if limit is not None:
        if T0 > limit:
            raise ValueError(f"padded prompts of {T0} tokens exceed the model's context of {limit}")
        total = min(total, limit)
    st.cached = True
    cache = _new_cache(model, B, total, kv_cache, page_size, num_pages)
    if page_size is not None:
        # each sequence's own rows; the right-padded prefill writes a short one's pad rows past its
        # reservation into the null page, so padding costs no pages
        _reserve(cache, [min(n + max_new_tokens, total) for n in lens.tolist()])
    if timed:
        _sync(ids)
    t0 = time.perf_counter()
    if prefill_chunk is not None:
        logits = chunked_prefill(model, cache, ids, lens, prefill_chunk)
    else:
        logits = model.step(ids, cache, 0, last=lens - 1)
    state = RaggedDecodeState(B, total, ids.device)
    state.set(lens)
    if timed:
        _sync(ids)
    t1 = time.perf_counter()
    st.prompt_tokens += int(lens.sum())
    st.prefill_s += t1 - t0
    done = torch.zeros(B, dtype=torch.bool, device=ids.device)
    new = []
    while len(new) < max_new_tokens:
        nxt = sampler(logits) if sampler is not None else sample(logits, temperature, top_k, greedy, generator, top_p)
        if eos_token_id is not None:
            nxt = torch.where(done[:, None], torch.full_like(nxt, pad_token_id), nxt)   # a finished row pads
            done |= nxt[:, 0] == eos_token_id
            state.active.copy_(~done)   # ... and stays at its position: its steps touch its own row only
        new.append(nxt)
        n = len(new)
        # the next step feeds token n - 1 of every row at cache row len_b + n - 1
        if n >= max_new_tokens or longest + n - 1 >= total:
            break
        if eos_token_id is not None and n % 16 == 0 and bool(done.all()):
            break
        logits = model.step_graph(nxt, cache, state)
        state.advance()
    if timed:
        _sync(ids)
    st.decode_s += time.perf_counter() - t1
    st.new_tokens += B * len(new)
    return ragged_layout(ids, lens, torch.cat(new, 1) if new else ids.new_zeros(B, 0), pad_token_id)


@torch.no_grad()
def generate(model, ids: torch.Tensor, max_new_tokens: int, temperature: float = 1.0,
             top_k: Optional[int] = None, top_p: Optional[float] = None, greedy: bool = False,
             eos_token_id: Optional[int] = None, generator: Optional[torch.Generator] = None,
             stats: Optional[GenerationStats] = None, timed: bool = False, sampler=None,
             kv_cache: Optional[str] = None, prompt_lens=None, pad_token_id: int = 0,
             page_size: Optional[int] = None, num_pages: Optional[int] = None,
             prefill_chunk: Optional[int] = None) -> torch.Tensor:
    """ids [B, T0] -> [B, T0 + n] (n <= max_new_tokens; stops early once every sequence has
    produced ``eos_token_id``, checked every 16 tokens to keep the host out of the loop).
    ``sampler`` (an infer.Sampler) replaces ``sample(...)``: one fused launch per token on the GPU,
    the fp64 oracle on the CPU, both drawing u01(seed, call * B + row).
    ``kv_cache="fp8"`` decodes from an e4m3 KV cache (infer/cache.py; models with ``new_cache(...,
    kv_cache=)``); None / "bf16": the model-dtype cache.

    ``prompt_lens`` (length-B tensor or list, 1 <= len_b <= T0): a ragged batch. ``ids`` is
    RIGHT-padded (what stands after a row's len_b tokens is ignored), every sequence decodes from
    its own position, and row b of the result holds its prompt, its n new tokens from column len_b,
    then ``pad_token_id`` (also after a row's ``eos_token_id``). Models with ``step_graph`` and a
    (k, v) cache: LLaMA3 and Gemma.

    ``page_size`` (a power of two in [16, 256]): decode from a paged KV cache (infer/cache.py
    PagedKVCache; LLaMA3 and Gemma, bf16 pages) of ``num_pages`` pages per layer (None: enough for every
    slot's full length). Every sequence's rows are reserved before the first launch -- T0 +
    max_new_tokens each, or ``prompt_lens[b] + max_new_tokens`` for a ragged batch -- so a pool too
    small raises ``CacheFull`` with no work done. Pages are not freed when a row reaches EOS.

    ``prefill_chunk=C`` (ragged batches only): the prompts run in blocks of C columns, every block after
    the first as a multi-token step behind the rows already cached (``model.extend``; LLaMA3 and Gemma),
    which bounds the prefill's activation memory. None: one pass."""
    if prefill_chunk is not None and prompt_lens is None:
        raise ValueError("generate: prefill_chunk needs prompt_lens (a ragged batch); a uniform batch prefills in "
                         "one pass")
    was = model.training
    model.eval()
    timed = timed or stats is not None  # stats requested -> device-synchronised phase timings
    st = stats if stats is not None else GenerationStats()
    B, T0 = ids.shape
    limit = getattr(model, "max_context", None)
    out = ids
    done = torch.zeros(B, dtype=torch.bool, device=ids.device)
    try:
        if prompt_lens is not None:
            out = _generate_ragged(model, ids, prompt_lens, pad_token_id, max_new_tokens, temperature, top_k, top_p,
                                   greedy, eos_token_id, generator, st, timed, sampler, kv_cache, page_size, num_pages,
                                   prefill_chunk)
        elif hasattr(model, "new_cache") and hasattr(model, "step"):
            st.cached = True
            total = T0 + max_new_tokens
            if limit is not None:
                total = min(total, limit)
            prompt = ids[:, -total:] if T0 > total else ids
            cache = _new_cache(model, B, total, kv_cache, page_size, num_pages)
            if page_size is not None:
                _reserve(cache, [total] * B)
            if timed:
                _sync(ids)
            t0 = time.perf_counter()
            logits = model.step(prompt, cache, 0)
            pos = prompt.shape[1]
            if timed:
                _sync(ids)
            t1 = time.perf_counter()
            st.prompt_tokens += B * prompt.shape[1]
            st.prefill_s += t1 - t0
            n = 0
            while n < max_new_tokens:
                nxt = sampler(logits) if sampler is not None else \
                    sample(logits, temperature, top_k, greedy, generator, top_p)
                if eos_token_id is not None:
                    nxt = torch.where(done[:, None], torch.full_like(nxt, eos_token_id), nxt)
                    done |= nxt[:, 0] == eos_token_id
                out = torch.cat([out, nxt], 1)
                n += 1
                if pos >= total or n >= max_new_tokens:
                    break
                if eos_token_id is not None and n % 16 == 0 and bool(done.all()):
                    break
                logits = model.step(nxt, cache, pos)
                pos += 1
            if timed:
                _sync(ids)
            st.decode_s += time.perf_counter() - t1
            st.new_tokens += B * n
        else:
            if kv_cache not in (None, "bf16"):
                raise NotImplementedError(f"kv_cache={kv_cache!r} needs a model with the cached-decoding protocol")
            if page_size is not None or num_pages is not None:
                raise NotImplementedError(f"page_size needs a model with the cached-decoding protocol; "
                                          f"{type(model).__name__} has none")
            block = limit or getattr(getattr(model, "c", None), "block_size", None)
            t1 = time.perf_counter()
            for n in range(max_new_tokens):
                window = out[:, -block:] if block else out
                lg = model(window)[:, -1].float()
                nxt = sampler(lg) if sampler is not None else \
                    sample(lg, temperature, top_k, greedy, generator, top_p)
                out = torch.cat([out, nxt], 1)
            if timed:
                _sync(ids)
            st.decode_s += time.perf_counter() - t1
            st.new_tokens += B * max_new_tokens
    finally:
        model.train(was)
    return out
