"""Per-kernel timing of the hand-written memory-bound / small-op kernels at the north-star shapes,
as achieved HBM bandwidth (ideal bytes / time). Run under ``rocprofv3 --pmc`` for counters.

usage: python tools/bench_kernels.py [--iters N] [--only name,name]

``--only gemv`` runs just the decode GEMV rows: the fp8 and MXFP4 weight-only kernels (gemv_w8, gemv_w4)
against the bf16 kernel (gemv) at the four LLaMA3-8B projection shapes, M = 1 and 4. ``--only skinny`` runs just
the 5..16-row weight-only rows: skinny_gemm_w8 and skinny_gemm_w4 on the images against torch.mm on the bf16 master
(what such a product runs on today) at those shapes and the LM head, M = 8 and 16. ``--only sample`` runs
just the token-sampler rows: the fused kernel (sample_logits) beside the eager infer.sample() on the same logits.
``--only decode_attn`` runs just the decode-attention rows: attn_decode_q8 over an fp8 KV cache against
attn_decode over the bf16 cache at LLaMA3-8B (H 32/8, hd 128) and Gemma-7B (H 16/1, hd 256) shapes, then
the per_row (ragged batch) form of both kernels at batch 16: equal lengths and lengths spread 1:4, then
attn_decode_paged (paged KV cache, 16- and 64-row pages in shuffled order) against attn_decode on the same
rows (``--only decode_attn_paged``: those rows alone). ``--only attn_extend`` runs just the extend-attention rows:
attn_extend (device per-sequence lengths) against attn_fwd (host length) at the same Tq / Tk, attn_extend_paged
(16- and 64-row pages in shuffled order) against gather + attn_fwd (``attn_extend_kernels``: those rows alone), and
(``attn_extend_e2e``: that alone) a chunked against a one-pass GraphDecoder.prefill of 16 ragged LLaMA3-8B prompts
with its peak memory.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from solvingpapers_amd.ops import _ext  # noqa: E402
from solvingpapers_amd import ops as O  # noqa: E402
from solvingpapers_amd.ops import misc, optim_kernels  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def cases():
    g = torch.Generator(device=DEV).manual_seed(0)

    def rn(*shape, dtype=BF, req=False):
        return torch.randn(*shape, device=DEV, dtype=dtype, generator=g).requires_grad_(req)

    N, D = 8192, 4096                                       # LLaMA3-8B rows x width
    x, w = rn(N, D), torch.ones(D, device=DEV, dtype=BF)
    out = {}
    out["rmsnorm_fwd_8192x4096"] = (lambda: O.rms_norm(x, w, 1e-5), 2 * N * D * 2)
    xr, wr = rn(N, D, req=True), torch.ones(D, device=DEV, dtype=BF, requires_grad=True)
    yr = O.rms_norm(xr, wr, 1e-5)
    dy = rn(N, D)
    out["rmsnorm_bwd_8192x4096"] = (lambda: torch.autograd.grad(yr, (xr, wr), dy, retain_graph=True),
                                    3 * N * D * 2)
    _, hn, rstd, _ = _ext.ops().norm_fwd(x, None, w, None, 1e-5)
    out["rmsnorm_bwd_kernel_8192x4096"] = (lambda: _ext.ops().norm_bwd(dy, x, w, rstd, None, None, None, None),
                                           3 * N * D * 2)
    Nv, Dv = 256 * 197, 768                                 # ViT-B/16 batch 256
    xl, wl, bl = rn(Nv, Dv), torch.ones(Dv, device=DEV, dtype=BF), torch.zeros(Dv, device=DEV, dtype=BF)
    out["layernorm_fwd_50432x768"] = (lambda: O.layer_norm(xl, wl, bl), 2 * Nv * Dv * 2)
    F = 14336
    gu = rn(N, 2 * F)
    out["swiglu_fwd_8192x14336"] = (lambda: O.swiglu(gu), 3 * N * F * 2)
    gug = rn(4096, 2 * 24576)
    out["geglu_fwd_4096x24576"] = (lambda: O.geglu(gug), 3 * 4096 * 24576 * 2)
    qkv = rn(1, N, 48, 128)                                 # 32 q + 8 k + 8 v heads
    out["rope_qk_inplace_8192x40x128"] = (lambda: O.rope_packed_(qkv, 40, 500000.0), 2 * N * 40 * 128 * 2)
    V = 128256
    logits = rn(N, V)
    tgt = torch.randint(0, V, (N,), device=DEV, generator=g)
    out["xent_fwd_8192x128256"] = (lambda: O.cross_entropy(logits, tgt), N * V * 2)
    emb = rn(V, D)
    ids = torch.randint(0, V, (1, N), device=DEV, generator=g)
    out["embedding_fwd_8192x4096"] = (lambda: O.embedding(emb, ids), 2 * N * D * 2)
    n = 1 << 28                                             # 268M-param AdamW slice (bf16 p, fp32 master/m/v, bf16 g)
    p = torch.zeros(n, device=DEV, dtype=BF)
    mst, m, v = (torch.zeros(n, device=DEV) for _ in range(3))
    gr = torch.full((n,), 1e-3, device=DEV, dtype=BF)
    out["adamw_268M"] = (lambda: optim_kernels.adamw_(p, mst, gr, m, v, 3e-4, 0.9, 0.95, 1e-8, 0.1, 1),
                         n * (2 + 2 + 3 * 4 * 2 + 2))
    mb, vb = (torch.zeros(n, device=DEV, dtype=BF) for _ in range(2))   # bf16 moments (DeepSeek benches)
    out["adamw_268M_bf16mom"] = (lambda: optim_kernels.adamw_(p, mst, gr, mb, vb, 3e-4, 0.9, 0.95, 1e-8, 0.1, 1),
                                 n * (2 + 2 + 4 * 2 + 2 * 2 * 2))
    out["sqsum_268M_bf16"] = (lambda: optim_kernels.sqsum(gr),
                              n * 2)
    s, t = rn(16384, 1000, dtype=torch.float32), rn(16384, 1000, dtype=torch.float32)
    y = torch.randint(0, 1000, (16384,), device=DEV, generator=g)
    out["kd_loss_16384x1000"] = (lambda: misc.distillation_loss(s, t, y, 7.0, 0.3), 2 * 16384 * 1000 * 4)
    sb, tb = rn(65536, 10), rn(65536, 10)                   # reference shape: CIFAR-10 logits, big batch
    yb = torch.randint(0, 10, (65536,), device=DEV, generator=g)
    out["kd_loss_grad_65536x10_bf16"] = (lambda: _ext.ops().kd_loss_fwd(sb, tb, yb, 7.0, 0.3, True), 3 * 65536 * 10 * 2)
    out["kd_loss_grad_16384x1000"] = (lambda: _ext.ops().kd_loss_fwd(s, t, y, 7.0, 0.3, True), 3 * 16384 * 1000 * 4)
    xd = rn(N, D)
    out["dropout_8192x4096"] = (lambda: misc.dropout(xd, 0.1, True), 2 * N * D * 2)
    return out


GEMV_SHAPES = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]   # LLaMA3-8B qkv, o, gate|up, down


def _graphed(fn):
    """``fn``'s launches as one HIP-graph replay (as GraphDecoder issues them): a few-microsecond
    kernel is timed on the device, not by how fast the host can enqueue it."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    return lambda g=graph, _outputs=keep: g.replay()


def gemv_rows(iters, rounds=3):
    """gemv_w8 and gemv_w4 next to gemv, same process, arms alternated A B C C B A per round. Every call
    reads another copy of the weight out of a ring larger than the 256 MB last-level cache (all arms: 32
    copies at least, >= 0.5 GB of the smallest format), as a decode step does, where each matrix is read once
    per token; one pass over the ring is one HIP-graph replay. Reported: GB/s of WEIGHT bytes (scales
    included), the fp8 / bf16 and mxfp4 / bf16 time ratios and mxfp4 / fp8 (< 1: the first is faster)."""
    from solvingpapers_amd.ops.moe import quant_weight_fp8_blk_uncached, quant_weight_mxfp4
    ops = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(0)
    for N, K in GEMV_SHAPES:
        ring = max(32, -(-(1 << 30) // (N * K)))             # >= 1 GB of fp8 bytes, 2 GB of bf16, 0.5 GB of mxfp4
        w = torch.randn(N, K, device=DEV, dtype=BF, generator=g)
        wq, _, s, _ = quant_weight_fp8_blk_uncached(w[None])
        w4, s4 = quant_weight_mxfp4(w[None])
        wb = [w.clone() for _ in range(ring)]
        wf = [(wq[0].clone(), s[0].clone()) for _ in range(ring)]
        w4s = [(w4[0].clone(), s4[0].clone()) for _ in range(ring)]
        for M in (1, 4):
            x = torch.randn(M, K, device=DEV, dtype=BF, generator=g)
            arms = {"bf16": _graphed(lambda: [ops.gemv(x, wi) for wi in wb]),
                    "fp8": _graphed(lambda: [ops.gemv_w8(x, q, si) for q, si in wf]),
                    "mxfp4": _graphed(lambda: [ops.gemv_w4(x, q, si) for q, si in w4s])}
            ms = {a: [] for a in arms}
            for _ in range(rounds):
                for arm in ("bf16", "fp8", "mxfp4", "mxfp4", "fp8", "bf16"):
                    ms[arm].append(timed(arms[arm], iters) / ring)
            med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
            for arm, key, nbytes in (("gemv", "bf16", N * K * 2), ("gemv_w8", "fp8", N * K + N * K // 16384),
                                     ("gemv_w4", "mxfp4", N * K // 2 + N * K // 32)):
                ratios = {} if key == "bf16" else {"time_vs_bf16": round(med[key] / med["bf16"], 3)}
                if key == "mxfp4":
                    ratios["time_vs_fp8"] = round(med[key] / med["fp8"], 3)
                print(json.dumps({"kernel": f"{arm}_M{M}_{N}x{K}", "ms": round(med[key], 5), "GB": round(nbytes / 1e9, 4),
                                  "weight_GB_per_s": round(nbytes / med[key] / 1e6, 1),
                                  "min_ms": round(min(ms[key]), 5), "max_ms": round(max(ms[key]), 5), **ratios}),
                      flush=True)
        del wb, wf, w4s


SKINNY_SHAPES = GEMV_SHAPES + [(128256, 4096)]                             # .. and the LM head


def skinny_rows(iters, rounds=3):
    """skinny_gemm_w8 and skinny_gemm_w4 next to torch.mm on the bf16 master (the route of a 5..16-row product
    without ``max_rows``), same process, arms alternated A B C C B A per round, as ``gemv_rows``: every call reads
    another copy of the weight out of a ring larger than the 256 MB last-level cache (>= 0.5 GB of the smallest
    format), one pass over the ring is one HIP-graph replay. Reported: time, GB/s of WEIGHT bytes (scales
    included) and the time ratio to the bf16 product (< 1: the image is faster)."""
    from solvingpapers_amd.ops.moe import quant_weight_fp8_blk_uncached, quant_weight_mxfp4
    ops = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(0)
    for N, K in SKINNY_SHAPES:
        ring = max(32, -(-(1 << 30) // (N * K))) if N * K < (1 << 28) else 3   # the LM head: 3 x 0.28 GB of mxfp4
        w = torch.randn(N, K, device=DEV, dtype=BF, generator=g)
        wq, _, s, _ = quant_weight_fp8_blk_uncached(w[None])
        w4, s4 = quant_weight_mxfp4(w[None])
        wb = [w.clone() for _ in range(ring)]
        wf = [(wq[0].clone(), s[0].clone()) for _ in range(ring)]
        w4s = [(w4[0].clone(), s4[0].clone()) for _ in range(ring)]
        del w, wq, w4
        for M in (8, 16):
            x = torch.randn(M, K, device=DEV, dtype=BF, generator=g)
            arms = {"bf16": _graphed(lambda: [torch.mm(x, wi.t()) for wi in wb]),
                    "fp8": _graphed(lambda: [ops.skinny_gemm_w8(x, q, si) for q, si in wf]),
                    "mxfp4": _graphed(lambda: [ops.skinny_gemm_w4(x, q, si) for q, si in w4s])}
            ms = {a: [] for a in arms}
            for _ in range(rounds):
                for arm in ("bf16", "fp8", "mxfp4", "mxfp4", "fp8", "bf16"):
                    ms[arm].append(timed(arms[arm], iters) / ring)
            med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
            for arm, key, nbytes in (("mm_bf16", "bf16", N * K * 2), ("skinny_gemm_w8", "fp8", N * K + N * K // 16384),
                                     ("skinny_gemm_w4", "mxfp4", N * K // 2 + N * K // 32)):
                ratios = {} if key == "bf16" else {"time_vs_bf16": round(med[key] / med["bf16"], 3)}
                print(json.dumps({"kernel": f"{arm}_M{M}_{N}x{K}", "ms": round(med[key], 5), "GB": round(nbytes / 1e9, 4),
                                  "weight_GB_per_s": round(nbytes / med[key] / 1e6, 1),
                                  "min_ms": round(min(ms[key]), 5), "max_ms": round(max(ms[key]), 5), **ratios}),
                      flush=True)
            del arms
        del wb, wf, w4s


def sample_rows(iters, rounds=3):
    """The fused sampler (csrc/kernels/sample.hip) beside infer.sample() on the same logits: V = 128256,
    fp32 holding bf16-rounded values as step_graph hands them over, arms alternated A B B A per round,
    medians. ``fused_graph_ms`` is one HIP-graph replay of the op plus the offset increment (how
    GraphDecoder runs it); ``fused_ms`` and ``eager_ms`` are host-enqueued, as between two replays."""
    from solvingpapers_amd.infer import Sampler, sample
    V = 128256
    g = torch.Generator(device=DEV).manual_seed(0)
    for B in (1, 4, 16):
        lg = (torch.randn(B, V, device=DEV, generator=g) * 2).bfloat16().float()
        ids = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        for name, k, p in (("plain", None, None), ("top_k50", 50, None), ("top_p0.9", None, 0.9), ("top_k50_p0.9", 50, 0.9)):
            smp = Sampler(0.8, k, p, seed=1, device=DEV)
            gen = torch.Generator(device=DEV).manual_seed(1)
            arms = {"fused_graph": _graphed(lambda: smp(lg, out=ids)),
                    "fused": lambda: smp(lg, out=ids),
                    "eager": lambda: ids.copy_(sample(lg, 0.8, k, False, gen, p))}
            ms = {a: [] for a in arms}
            for _ in range(rounds):
                for arm in ("eager", "fused", "fused_graph", "fused_graph", "fused", "eager"):
                    ms[arm].append(timed(arms[arm], iters))
            med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
            print(json.dumps({"kernel": f"sample_{name}_B{B}_V{V}", "fused_graph_ms": round(med["fused_graph"], 5),
                              "fused_ms": round(med["fused"], 5), "eager_ms": round(med["eager"], 5),
                              "fused_graph_vs_eager": round(med["fused_graph"] / med["eager"], 3),
                              "min_ms": {a: round(min(v), 5) for a, v in ms.items()},
                              "max_ms": {a: round(max(v), 5) for a, v in ms.items()}}), flush=True)


# (H, Hkv, hd, B, Tk): LLaMA3-8B GQA at short / long caches and small / large batch, Gemma-7B MQA
DECODE_ATTN_SHAPES = [(32, 8, 128, 1, 1024), (32, 8, 128, 1, 8192), (32, 8, 128, 16, 1024), (32, 8, 128, 16, 8192),
                      (16, 1, 256, 16, 8192)]


def decode_attn_rows(iters, rounds=3):
    """attn_decode_q8 (fp8 cache) next to attn_decode (bf16 cache), one new token per sequence, same
    process, arms alternated A B B A per round, medians. Every call reads another cache out of a ring
    larger than the 256 MB last-level cache (the fp8 ring too), as a decode step does, where each layer's
    cache is read once per token; one pass over the ring is one HIP-graph replay. Reported: GB/s of K/V
    bytes (fp8: data + scale bytes) and the fp8 / bf16 time ratio (< 1: the fp8 kernel is faster)."""
    from solvingpapers_amd.ops import reference as R
    ops = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(0)
    for H, Hkv, hd, B, Tk in DECODE_ATTN_SHAPES:
        f8_bytes = 2 * B * Tk * Hkv * (hd + 1)
        ring = max(4, -(-(320 << 20) // f8_bytes))           # >= 320 MB of fp8 caches, twice that of bf16
        q = torch.randn(B, 1, H, hd, device=DEV, dtype=BF, generator=g)
        k, v = (torch.randn(B, Tk, Hkv, hd, device=DEV, dtype=BF, generator=g) for _ in range(2))
        (kq, ks), (vq, vs) = R.quant_kv8(k), R.quant_kv8(v)
        cb = [(k.clone(), v.clone()) for _ in range(ring)]
        cf = [tuple(t.clone() for t in (kq, ks, vq, vs)) for _ in range(ring)]
        sc = hd ** -0.5
        arms = {"bf16": _graphed(lambda: [ops.attn_decode(q, ki, vi, sc, True, 0) for ki, vi in cb]),
                "fp8": _graphed(lambda: [ops.attn_decode_q8(q, *c, sc, True, 0) for c in cf])}
        ms = {"bf16": [], "fp8": []}
        for _ in range(rounds):
            for arm in ("bf16", "fp8", "fp8", "bf16"):
                ms[arm].append(timed(arms[arm], iters) / ring)
        mb, mf = (sorted(ms[a])[len(ms[a]) // 2] for a in ("bf16", "fp8"))
        for arm, key, m_, nbytes in (("attn_decode", "bf16", mb, 2 * B * Tk * Hkv * hd * 2),
                                     ("attn_decode_q8", "fp8", mf, f8_bytes)):
            print(json.dumps({"kernel": f"{arm}_B{B}_Tk{Tk}_H{H}kv{Hkv}_hd{hd}", "ms": round(m_, 5),
                              "GB": round(nbytes / 1e9, 4), "kv_GB_per_s": round(nbytes / m_ / 1e6, 1),
                              "min_ms": round(min(ms[key]), 5), "max_ms": round(max(ms[key]), 5), "ring": ring,
                              **({"time_vs_bf16": round(mf / mb, 3)} if key == "fp8" else {})}), flush=True)
        del cb, cf, arms


def decode_attn_per_row_rows(iters, rounds=3):
    """The per_row (ragged batch) form of both decode-attention kernels at the batch-16 LLaMA3-8B shapes:
    ``scalar`` is a one-entry device kv_len (what the uniform graph decode launches), ``equal`` a kv_len
    [B] with every length Tk, ``spread`` lengths spaced evenly from Tk / 4 to Tk (1:4). Ring, A B C C B A
    order and medians as in decode_attn_rows. ``time_vs_scalar`` compares at equal work; the spread rows
    count only the valid rows' bytes in their GB/s (the empty splits of short rows still launch)."""
    from solvingpapers_amd.ops import reference as R
    ops = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(0)
    for H, Hkv, hd, B, Tk in [s for s in DECODE_ATTN_SHAPES if s[3] > 1 and s[2] == 128]:
        ring = max(4, -(-(320 << 20) // (2 * B * Tk * Hkv * (hd + 1))))
        q = torch.randn(B, 1, H, hd, device=DEV, dtype=BF, generator=g)
        k, v = (torch.randn(B, Tk, Hkv, hd, device=DEV, dtype=BF, generator=g) for _ in range(2))
        (kq, ks), (vq, vs) = R.quant_kv8(k), R.quant_kv8(v)
        sc = hd ** -0.5
        lens = {"scalar": torch.tensor([Tk], device=DEV, dtype=torch.int32),
                "equal": torch.full((B,), Tk, device=DEV, dtype=torch.int32),
                "spread": torch.linspace(Tk / 4, Tk, B, device=DEV).round().int()}
        rows = {a: (B * Tk if a != "spread" else int(lens[a].sum())) for a in lens}
        for fmt, row_bytes in (("bf16", Hkv * hd * 2), ("fp8", Hkv * (hd + 1))):
            if fmt == "bf16":
                ringc = [(k.clone(), v.clone()) for _ in range(ring)]
                call = lambda c, a: ops.attn_decode(q, c[0], c[1], sc, True, 0, lens[a], a != "scalar")
            else:
                ringc = [tuple(t.clone() for t in (kq, ks, vq, vs)) for _ in range(ring)]
                call = lambda c, a: ops.attn_decode_q8(q, *c, sc, True, 0, lens[a], a != "scalar")
            arms = {a: _graphed(lambda a=a: [call(c, a) for c in ringc]) for a in lens}
            ms = {a: [] for a in arms}
            for _ in range(rounds):
                for arm in ("scalar", "equal", "spread", "spread", "equal", "scalar"):
                    ms[arm].append(timed(arms[arm], iters) / ring)
            med = {a: sorted(t)[len(t) // 2] for a, t in ms.items()}
            name = "attn_decode" if fmt == "bf16" else "attn_decode_q8"
            for a in arms:
                nbytes = 2 * rows[a] * row_bytes
                print(json.dumps({"kernel": f"{name}_{a}_B{B}_Tk{Tk}_H{H}kv{Hkv}_hd{hd}", "ms": round(med[a], 5),
                                  "GB": round(nbytes / 1e9, 4), "kv_GB_per_s": round(nbytes / med[a] / 1e6, 1),
                                  "min_ms": round(min(ms[a]), 5), "max_ms": round(max(ms[a]), 5), "ring": ring,
                                  **({"time_vs_scalar": round(med[a] / med["scalar"], 3)} if a != "scalar" else {})}),
                      flush=True)
            del ringc, arms


def decode_attn_paged_rows(iters, rounds=3):
    """attn_decode_paged (paged KV cache, pages of 16 and of 64 rows assigned in shuffled order) next to
    attn_decode on the same rows in a contiguous cache, at DECODE_ATTN_SHAPES, one new token per sequence.
    Ring of caches (every arm its own, each larger than the last-level cache), A B C C B A order and
    medians as in decode_attn_rows; all three arms read a device kv_len. ``time_vs_contiguous`` > 1: paging
    is slower."""
    ops = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(0)
    for H, Hkv, hd, B, Tk in DECODE_ATTN_SHAPES:
        nbytes = 2 * B * Tk * Hkv * hd * 2
        ring = max(4, -(-(640 << 20) // nbytes))
        q = torch.randn(B, 1, H, hd, device=DEV, dtype=BF, generator=g)
        k, v = (torch.randn(B, Tk, Hkv, hd, device=DEV, dtype=BF, generator=g) for _ in range(2))
        sc = hd ** -0.5
        kv_len = torch.tensor([Tk], device=DEV, dtype=torch.int32)
        rings = {"contiguous": [(k.clone(), v.clone()) for _ in range(ring)]}
        for page in (16, 64):
            NP = Tk // page
            pools = []
            for i in range(ring):      # every sequence's pages scattered over the pool; page 0 stays the null page
                perm = torch.randperm(B * NP, generator=torch.Generator().manual_seed(page + i)) + 1
                bt = perm.view(B, NP).to(DEV, torch.int32)
                kp, vp = (torch.zeros(B * NP + 1, page, Hkv, hd, device=DEV, dtype=BF) for _ in range(2))
                idx = bt.long().flatten()
                kp[idx] = k.view(B * NP, page, Hkv, hd)
                vp[idx] = v.view(B * NP, page, Hkv, hd)
                pools.append((kp, vp, bt))
            rings[f"page{page}"] = pools
        o0 = ops.attn_decode(q, k, v, sc, True, 0, kv_len)[0]
        for page in (16, 64):          # the same bits through the table, before anything is timed
            kp, vp, bt = rings[f"page{page}"][0]
            assert torch.equal(ops.attn_decode_paged(q, kp, vp, bt, sc, True, 0, Tk, kv_len)[0], o0)
        arms = {"contiguous": _graphed(lambda: [ops.attn_decode(q, ki, vi, sc, True, 0, kv_len)
                                                for ki, vi in rings["contiguous"]])}
        for page in (16, 64):
            arms[f"page{page}"] = _graphed(lambda page=page: [ops.attn_decode_paged(q, kp, vp, bt, sc, True, 0, Tk, kv_len)
                                                              for kp, vp, bt in rings[f"page{page}"]])
        ms = {a: [] for a in arms}
        for _ in range(rounds):
            for arm in ("contiguous", "page16", "page64", "page64", "page16", "contiguous"):
                ms[arm].append(timed(arms[arm], iters) / ring)
        med = {a: sorted(t)[len(t) // 2] for a, t in ms.items()}
        for a in arms:
            name = "attn_decode" if a == "contiguous" else f"attn_decode_paged_{a}"
            print(json.dumps({"kernel": f"{name}_B{B}_Tk{Tk}_H{H}kv{Hkv}_hd{hd}", "ms": round(med[a], 5),
                              "GB": round(nbytes / 1e9, 4), "kv_GB_per_s": round(nbytes / med[a] / 1e6, 1),
                              "min_ms": round(min(ms[a]), 5), "max_ms": round(max(ms[a]), 5), "ring": ring,
                              **({"time_vs_contiguous": round(med[a] / med["contiguous"], 3)}
                                 if a != "contiguous" else {})}), flush=True)
        del rings, arms


# (H, Hkv, hd, B, Tq, Tk): a 512-token chunk against 2K / 8K / 32K cache rows at LLaMA3-8B heads, the same at
# Gemma's MQA hd 256, and a 64-token turn against 8K rows
ATTN_EXTEND_SHAPES = [(32, 8, 128, B, 512, Tk) for Tk in (2048, 8192, 32768) for B in (1, 4)] + \
    [(16, 1, 256, 1, 512, 8192), (16, 1, 256, 4, 512, 8192), (32, 8, 128, 1, 64, 8192), (32, 8, 128, 4, 64, 8192)]


def attn_extend_rows(iters, rounds=3):
    """Arm 1: attn_extend over the contiguous cache (device kv_len [B], every length Tk) against attn_fwd with the
    host length at the same Tq / Tk -- the same MFMA loop, so ``time_vs_fwd`` near 1 is the expectation. Arm 2:
    attn_extend_paged through shuffled 16- and 64-row pages against PagedKV.gathered + attn_fwd, what a paged
    multi-token step at a host length runs (``time_vs_gather_fwd``, the gather included). Each arm is one HIP-graph
    replay, the six arms alternated A B C D E F F E D C B A per round, medians reported with min / max. TFLOP/s counts the causal
    work 4 * hd * H * B * Tq * (Tk - Tq / 2)."""
    from solvingpapers_amd.ops.attention import PagedKV
    ops = _ext.ops()
    g = torch.Generator(device=DEV).manual_seed(0)
    for H, Hkv, hd, B, Tq, Tk in ATTN_EXTEND_SHAPES:
        q = torch.randn(B, Tq, H, hd, device=DEV, dtype=BF, generator=g)
        k, v = (torch.randn(B, Tk, Hkv, hd, device=DEV, dtype=BF, generator=g) for _ in range(2))
        sc = hd ** -0.5
        kv_len = torch.full((B,), Tk, device=DEV, dtype=torch.int32)
        layers = {}
        for page in (16, 64):
            NP = Tk // page
            perm = torch.randperm(B * NP, generator=torch.Generator().manual_seed(page)) + 1
            bt = perm.view(B, NP).to(DEV, torch.int32)
            kp, vp = (torch.zeros(B * NP + 1, page, Hkv, hd, device=DEV, dtype=BF) for _ in range(2))
            kp[bt.long().flatten()] = k.view(B * NP, page, Hkv, hd)
            vp[bt.long().flatten()] = v.view(B * NP, page, Hkv, hd)
            layers[page] = PagedKV(kp, vp, bt, page, Tk)
        o0 = ops.attn_extend(q, k, v, sc, kv_len, True)[0]
        f0 = ops.attn_fwd(q, k, v, sc, True, 0.0, 0, None)[0]
        err = ((o0.float() - f0.float()).norm() / f0.float().norm()).item()
        for page, l in layers.items():     # the same bits through the table, before anything is timed
            assert torch.equal(ops.attn_extend_paged(q, l.k, l.v, l.block_table, sc, Tk, kv_len, True)[0], o0)

        def gather_fwd(l):
            kg, vg = l.gathered(Tk)
            return ops.attn_fwd(q, kg, vg, sc, True, 0.0, 0, None)

        arms = {"fwd": _graphed(lambda: ops.attn_fwd(q, k, v, sc, True, 0.0, 0, None)),
                "extend": _graphed(lambda: ops.attn_extend(q, k, v, sc, kv_len, True))}
        for page, l in layers.items():
            arms[f"paged{page}"] = _graphed(lambda l=l: ops.attn_extend_paged(q, l.k, l.v, l.block_table, sc, Tk,
                                                                              kv_len, True))
            arms[f"gather_fwd{page}"] = _graphed(lambda l=l: gather_fwd(l))
        order = list(arms)
        ms = {a: [] for a in arms}
        for _ in range(rounds):
            for arm in order + order[::-1]:
                ms[arm].append(timed(arms[arm], iters))
        med = {a: sorted(t)[len(t) // 2] for a, t in ms.items()}
        flop = 4.0 * hd * H * B * Tq * (Tk - Tq / 2)
        base = {"extend": ("time_vs_fwd", "fwd"), "paged16": ("time_vs_gather_fwd", "gather_fwd16"),
                "paged64": ("time_vs_gather_fwd", "gather_fwd64")}
        names = {"fwd": "attn_fwd", "extend": "attn_extend", "paged16": "attn_extend_paged_page16",
                 "paged64": "attn_extend_paged_page64", "gather_fwd16": "gather+attn_fwd_page16",
                 "gather_fwd64": "gather+attn_fwd_page64"}
        for a in arms:
            row = {"kernel": f"{names[a]}_B{B}_Tq{Tq}_Tk{Tk}_H{H}kv{Hkv}_hd{hd}", "ms": round(med[a], 5),
                   "TFLOP_per_s": round(flop / med[a] / 1e9, 1), "min_ms": round(min(ms[a]), 5),
                   "max_ms": round(max(ms[a]), 5)}
            if a in base:
                row[base[a][0]] = round(med[a] / med[base[a][1]], 3)
            if a == "paged16" or a == "paged64":
                row["time_vs_extend"] = round(med[a] / med["extend"], 3)
            if a == "extend":
                row["rel_l2_vs_fwd"] = float(f"{err:.3e}")
            print(json.dumps(row), flush=True)
        del arms, layers


def attn_extend_e2e_rows(rounds=2, chunk=512, layers=None):
    """Arm 3: GraphDecoder.prefill of 16 ragged LLaMA3-8B prompts of 2K..8K tokens into a paged cache (64-row
    pages), chunk=512 against chunk=None: one decoder, the two alternated A B B A per round, each timed between
    device synchronisations with its own torch.cuda.max_memory_allocated (the peak is reset before each)."""
    import time
    from solvingpapers_amd.infer import GraphDecoder
    from solvingpapers_amd.models import llama3
    kw = {} if layers is None else {"n_layers": layers}
    m = llama3.Llama3(llama3.config("llama3_8b", **kw), device=DEV, dtype=BF, seed=1).eval()
    lens = [2048 + (6080 * i) // 15 for i in range(16)]     # 2048 .. 8128: the longest plus 64 rows is the 8K context
    ids = torch.randint(0, m.c.vocab_size, (16, max(lens)), device=DEV)
    dec = GraphDecoder(m, 16, max(lens) + 64, ragged=True, page_size=64)
    res = {"chunked": [], "one_pass": []}
    logits = {}

    def run(arm):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        logits[arm] = dec.prefill(ids, lens, chunk=chunk if arm == "chunked" else None)
        torch.cuda.synchronize()
        res[arm].append((time.perf_counter() - t0, torch.cuda.max_memory_allocated()))

    run("one_pass"), run("chunked")            # warm-up of both paths (kernels, allocator, GEMM selection)
    res = {"chunked": [], "one_pass": []}
    for _ in range(rounds):
        for arm in ("chunked", "one_pass", "one_pass", "chunked"):
            run(arm)
    base = torch.cuda.memory_allocated()       # weights, cache, graph pools: held by both arms
    err = ((logits["chunked"] - logits["one_pass"]).norm() / logits["one_pass"].norm()).item()
    med = {a: sorted(t for t, _ in r)[len(r) // 2] for a, r in res.items()}
    for a, r in res.items():
        peak = max(p for _, p in r)
        print(json.dumps({"kernel": f"llama3_8b_prefill_{a}_16x2K..8K_page64" + (f"_chunk{chunk}" if a == "chunked" else ""),
                          "s": round(med[a], 4), "min_s": round(min(t for t, _ in r), 4),
                          "max_s": round(max(t for t, _ in r), 4), "prompt_tokens": sum(lens),
                          "tok_per_s": round(sum(lens) / med[a], 1), "peak_mem_GB": round(peak / 1e9, 3),
                          "peak_above_resident_GB": round((peak - base) / 1e9, 3),
                          **({"time_vs_one_pass": round(med[a] / med["one_pass"], 3),
                              "logits_rel_l2_vs_one_pass": float(f"{err:.3e}")} if a == "chunked" else {})}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    assert _ext.load(), "HIP extension missing"
    only = set(filter(None, a.only.split(",")))
    if not only or "gemv" in only:
        gemv_rows(a.iters)
    if not only or "skinny" in only:
        skinny_rows(a.iters)
    if not only or "sample" in only:
        sample_rows(a.iters)
    if not only or "decode_attn" in only:
        decode_attn_rows(a.iters)
        decode_attn_per_row_rows(a.iters)
    if not only or only & {"decode_attn", "decode_attn_paged"}:
        decode_attn_paged_rows(a.iters)
    if not only or only & {"attn_extend", "attn_extend_kernels"}:
        attn_extend_rows(a.iters)
    if only & {"attn_extend", "attn_extend_e2e"}:      # builds a LLaMA3-8B: never part of a plain run (no --only)
        attn_extend_e2e_rows()
    for name, (fn, nbytes) in ({} if only and only <= {"gemv", "skinny", "sample", "decode_attn", "decode_attn_paged",
                                                       "attn_extend", "attn_extend_kernels", "attn_extend_e2e"}
                               else cases()).items():
        if only and name not in only:
            continue
        ms = timed(fn, a.iters)
        print(json.dumps({"kernel": name, "ms": round(ms, 4), "GB": round(nbytes / 1e9, 3),
                          "TB_per_s": round(nbytes / ms / 1e9, 2)}), flush=True)


if __name__ == "__main__":
    main()
