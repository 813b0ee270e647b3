#!/usr/bin/env python
"""KV-cached generation throughput (serving-side bench): prompt prefill + N decode steps.

Default: LLaMA3-8B shape, bf16, random-init weights, synthetic prompt. Reports prefill
tok/s and decode tok/s (all sequences); one JSON line. ``--weights fp8`` decodes from the
block-scaled e4m3 images of infer.quantize_decode_weights, ``--weights mxfp4`` from its OCP MXFP4 images
(prefill stays on bf16); ``--weight-rows N`` (4..16, with ``--weights fp8|mxfp4``) builds them with ``max_rows=N``, so a
batch of up to N sequences decodes from the images too (csrc/kernels/skinny_gemm.hip), and adds ``weight_rows`` to the result line;
``--kv-cache fp8`` keeps the KV cache as e4m3 rows with per-row E8M0 scales (infer/cache.py) and
decodes with attn_decode_q8 -- the cache's size is reported as ``kv_cache_bytes`` either way. The
``--sampler`` picks how the next token is drawn: ``greedy`` (argmax, captured with
``--graph``), ``eager`` (infer.sample(): topk / sort / softmax / multinomial launches between the replays) or ``fused``
(infer.Sampler: one kernel, captured in the graph). ``--prompt-lens a,b,c,...`` decodes a ragged batch (one
prompt length per sequence, right-padded; per-sequence positions: GraphDecoder(ragged=True) with ``--graph``) and
adds ``prompt_lens`` to the result line. ``--page-size N`` decodes from a paged KV cache (infer/cache.py PagedKVCache,
bf16 pages of N rows) of ``--pages N`` pages per layer (default: enough for every slot's prompt + new rows);
``kv_cache_bytes`` is then the pools' size. ``--prefill-chunk N`` (with ``--prompt-lens``) runs the prompts in blocks
of N columns, every block after the first as a multi-token step behind the cached rows (model.extend), and adds
``prefill_chunk``, ``prefill_s`` and ``peak_mem_bytes`` (torch.cuda.max_memory_allocated over the timed call) to the
result line; ``--prefill-chunk 0`` reports the same fields for the one-pass prefill. The reference decodes by re-running the whole prefix per token (llama3/LLaMA-jax.ipynb:1629: 20 tokens in 60.6 s on a T4)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from solvingpapers_amd.infer import GenerationStats  # noqa: E402


def build(model, layers, sets=()):
    kw = {} if layers is None else {"n_layers": layers}
    for kv in sets:                      # --set n_experts=32 etc. (int/float/str)
        k, v = kv.split("=", 1)
        for cast in (int, float):
            try:
                v = cast(v)
                break
            except ValueError:
                pass
        kw[k] = v
    if model.startswith("dsv3"):
        # MLA decode attends over the per-layer compressed latent cache (kv_lora + rope values
        # per token) with W_uk absorbed into q and W_uv applied after
        from solvingpapers_amd.models import deepseekv3
        return deepseekv3.DeepSeekV3(deepseekv3.config(model, **kw), device="cuda", dtype=torch.bfloat16, seed=1)
    if model.startswith("llama3"):
        from solvingpapers_amd.models import llama3
        return llama3.Llama3(llama3.config(model, **kw), device="cuda", dtype=torch.bfloat16, seed=1)
    from solvingpapers_amd.models import gemma
    return gemma.Gemma(gemma.config(model, **kw), device="cuda", dtype=torch.bfloat16, seed=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3_8b")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--prompt", type=int, default=1024)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--graph", action="store_true", help="HIP-graph decode (one replay per token)")
    ap.add_argument("--set", action="append", default=[], help="config override key=value")
    ap.add_argument("--weights", choices=["bf16", "fp8", "mxfp4"], default="bf16",
                    help="fp8: decode products read e4m3 weight images (128x128 E8M0 block scales); "
                         "mxfp4: e2m1 images (1x32 E8M0 block scales)")
    ap.add_argument("--weight-rows", type=int, default=None,
                    help="with --weights fp8|mxfp4: quantize_decode_weights(max_rows=N), N in [4, 16]: products of up "
                         "to N token rows read the images (default: 4, the GEMV routes alone)")
    ap.add_argument("--kv-cache", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: e4m3 KV cache with one E8M0 scale per (batch, kv head, token) row")
    ap.add_argument("--sampler", choices=["greedy", "eager", "fused"], default="greedy",
                    help="eager: infer.sample() between the steps; fused: infer.Sampler (one kernel, captured with --graph)")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--top-p", type=float, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--prompt-lens", default=None,
                    help="a,b,c,...: one prompt length per sequence (ragged batch, right-padded to the longest; "
                         "sets --batch and --prompt); with --graph the step is captured over per-sequence positions")
    ap.add_argument("--page-size", type=int, default=None,
                    help="paged KV cache: rows per page (a power of two in [16, 256]); LLaMA3 / Gemma, bf16 cache")
    ap.add_argument("--pages", type=int, default=None,
                    help="pages per layer of the paged cache, the null page included (default: batch * pages per "
                         "sequence + 1)")
    ap.add_argument("--prefill-chunk", type=int, default=None,
                    help="ragged batches (--prompt-lens): prefill in blocks of N columns (model.extend behind the "
                         "first); 0: one pass, but report prefill_s and peak_mem_bytes as the chunked run does")
    a = ap.parse_args(argv)
    if a.prefill_chunk is not None and a.prompt_lens is None:
        ap.error("--prefill-chunk needs --prompt-lens (a ragged batch)")
    if a.pages is not None and a.page_size is None:
        ap.error("--pages needs --page-size")
    if a.weight_rows is not None and a.weights == "bf16":
        ap.error("--weight-rows needs --weights fp8 or mxfp4")
    pkw = {} if a.page_size is None else {"page_size": a.page_size, "num_pages": a.pages}
    lens = None
    if a.prompt_lens is not None:
        lens = [int(x) for x in a.prompt_lens.split(",")]
        a.batch, a.prompt = len(lens), max(lens)
    m = build(a.model, a.layers, a.set).eval()
    extra = {} if lens is None else {"prompt_lens": lens}
    if pkw:
        extra.update(page_size=a.page_size)
    if a.weights != "bf16":
        from solvingpapers_amd.infer import quantize_decode_weights
        qkw = {} if a.weight_rows is None else {"max_rows": a.weight_rows}   # {}: the call as before the option existed
        rep = quantize_decode_weights(m, **qkw) if a.weights == "fp8" else quantize_decode_weights(m, fmt=a.weights, **qkw)
        extra = {"weights": rep["format"], "image_bytes": rep["image_bytes"],
                 "quantized_params": len(rep["quantized"]), "bf16_params": len(rep["bf16"])}
        if a.weight_rows is not None:
            extra["weight_rows"] = rep["max_rows"]
    kvc = None if a.kv_cache == "bf16" else a.kv_cache     # None: every call as before the option existed
    ckw = {} if kvc is None else {"kv_cache": kvc}
    ids = torch.randint(0, m.c.vocab_size, (a.batch, a.prompt), device="cuda")
    st = GenerationStats()
    from solvingpapers_amd.infer import Sampler
    sampler = Sampler(a.temperature, a.top_k, a.top_p, seed=a.seed, device="cuda") if a.sampler == "fused" else None
    # eager: today's sample() path with the same parameters, drawing from a seeded device generator
    kw = {} if a.sampler != "eager" else {"temperature": a.temperature, "top_k": a.top_k, "top_p": a.top_p,
                                          "generator": torch.Generator(device="cuda").manual_seed(a.seed)}
    rkw = {} if lens is None else {"prompt_lens": lens}    # {}: every call as before the option existed
    if a.prefill_chunk:
        rkw["prefill_chunk"] = a.prefill_chunk
    wkw = {} if lens is None else {"prompt_lens": [min(n, 64) for n in lens]}
    if a.sampler != "greedy":
        extra.update(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=a.seed)
    if a.graph:
        from solvingpapers_amd.infer import GraphDecoder
        dec = GraphDecoder(m, a.batch, a.prompt + a.new, greedy=a.sampler == "greedy", sampler=sampler, **ckw,
                           **pkw, **({} if lens is None else {"ragged": True}))
        cache_bytes = dec.cache.nbytes() if hasattr(dec.cache, "nbytes") else None
        if pkw:
            extra.update(num_pages=dec.cache.num_pages)
        dec.generate(ids[:, :64], 4, **kw, **wkw)  # warm-up of the eager prefill path
        if sampler is not None:
            sampler.reseed(a.seed)
        torch.cuda.reset_peak_memory_stats()
        out = dec.generate(ids, a.new, stats=st, **kw, **rkw)
    else:
        kw = dict(kw, greedy=a.sampler == "greedy", sampler=sampler, **ckw)
        gen = m.generate
        if pkw or a.prefill_chunk:   # the models' generate() carries no paging or chunking arguments: the driver itself
            from solvingpapers_amd.infer import generate
            gen = lambda *args, **k: generate(m, *args, **k, **pkw)
        if pkw:
            pool = m.new_cache(a.batch, a.prompt + a.new, **ckw, **pkw)   # what generate() allocates
            cache_bytes = pool.nbytes()
            extra.update(num_pages=pool.num_pages)
            del pool
        else:
            row = m.new_cache(a.batch, 1, **ckw)     # generate() allocates prompt + new rows of this size
            cache_bytes = row.nbytes() * (a.prompt + a.new) if hasattr(row, "nbytes") else None
        gen(ids[:, :64], 4, **kw, **wkw)         # warm-up (kernels, allocator)
        if sampler is not None:
            sampler.reseed(a.seed)
        torch.cuda.reset_peak_memory_stats()
        out = gen(ids, a.new, stats=st, **kw, **rkw)
    torch.cuda.synchronize()
    if a.prefill_chunk is not None:
        extra.update(prefill_chunk=a.prefill_chunk, prefill_s=round(st.prefill_s, 4),
                     peak_mem_bytes=torch.cuda.max_memory_allocated())
    print(json.dumps({"metric": "decode tokens/s", "model": a.model, "graph": a.graph, "batch": a.batch, "prompt": a.prompt,
                      "new_tokens": st.new_tokens, "prefill_tok_s": round(st.prefill_tok_s, 1),
                      "decode_tok_s": round(st.decode_tok_s, 2),
                      "ms_per_token": round(1e3 * st.decode_s / max(1, st.new_tokens // a.batch), 3),
                      "dtype": "bf16", "data": "synthetic prompt, random-init weights", "sampler": a.sampler,
                      "kv_cache": a.kv_cache, "kv_cache_bytes": cache_bytes,
                      "out_len": out.shape[1], **extra}), flush=True)


if __name__ == "__main__":
    main()
