"""Inference: KV-cached generation for the language models of the catalogue.

* :func:`sample` -- greedy / categorical / top-k / top-p with temperature;
* :class:`Sampler` -- the same filters as one fused launch with a device-resident counter RNG
  (csrc/kernels/sample.hip): reproducible, and capturable in the decode graph;
* :class:`KVCache` -- preallocated per-layer K/V buffers, written in place; ``quant="fp8"`` (the
  drivers' ``kv_cache="fp8"``, one of :data:`KV_CACHE_FORMATS`) keeps them as e4m3 rows with per-row
  E8M0 scales, one :class:`KV8` handle per layer, read by the fp8 decode-attention kernel;
* :class:`PagedKVCache` -- the drivers' ``page_size=``: a pool of fixed-size bf16 pages per layer and one
  block table shared by all layers (one :class:`PagedKV` handle per layer), so memory follows the tokens
  held; ``reserve`` / ``free`` hand pages out and take them back, :class:`CacheFull` when the pool is short;
* :func:`generate` -- prompt prefill (flash attention) + token-by-token decode (split-K
  decode kernel, csrc/kernels/decode.hip) with the model's own cache layout, timing
  prefill and decode separately; ``prompt_lens=`` takes a right-padded batch of prompts of different
  lengths (ragged batch: per-sequence positions in :class:`RaggedDecodeState`; LLaMA3 and Gemma);
  ``prefill_chunk=`` runs such prompts in blocks of columns, every block after the first as a multi-token
  step behind the rows already cached (:class:`ExtendState`, ``model.extend``, the extend-attention
  kernel csrc/kernels/attention_extend.hip); ``GraphDecoder.extend_row`` appends to one live slot;
* :func:`quantize_decode_weights` / :func:`clear_decode_weights` -- fp8 weight-only decode:
  block-scaled e4m3 images of the projection matrices, read by the decode GEMV kernels
  (csrc/kernels/gemv.hip); see infer/quant.py.

Reference entry points (all recompute the whole prefix per token, no cache):
gpt/gpt-jax.ipynb:821-829, llama3/LLaMA-jax.ipynb:499-511, gemma/gemma.ipynb:608-630,
deepseekv3/deepseekv3.ipynb:1849-1873.
"""
from ..ops.attention import KV8, PagedKV
from .cache import KV_CACHE_FORMATS, CacheFull, KVCache, PagedKVCache
from .generate import GenerationStats, generate
from .graph import DecodeState, ExtendState, GraphDecoder, RaggedDecodeState
from .quant import clear_decode_weights, quantize_decode_weights
from .sampling import Sampler, sample

__all__ = ["CacheFull", "KV8", "KV_CACHE_FORMATS", "KVCache", "PagedKV", "PagedKVCache", "DecodeState", "ExtendState", "GenerationStats", "GraphDecoder", "RaggedDecodeState",
           "Sampler", "clear_decode_weights", "generate", "quantize_decode_weights", "sample"]
