"""fp8 weight-only decode: block-scaled e4m3 images of a model's projection matrices.

Decode is weight streaming: every token reads every projection matrix once
(csrc/kernels/gemv.hip). :func:`quantize_decode_weights` builds, for each eligible
parameter, the OCP e4m3 image with one E8M0 scale per 128 x 128 block -- the format of the fp8
training path (ops/moe.py ``quant_weight_fp8_blk``) and of DeepSeek-V3 checkpoints -- and
attaches it to the Parameter. From then on decode-shaped inference products
(``ops.linear.linear`` with <= 4 token rows, ``ops.moe.grouped_linear`` with <= 64 expert rows)
read the image through ``gemv_w8`` / ``grouped_gemv_w8`` (csrc/kernels/gemv.hip): half the
bytes per token.

This mode buys decode speed and COSTS memory: the bf16 master weights stay (prefill, training
and every product with more rows run on them exactly as before), so a quantised model holds
+50 % weight bytes. Dropping the masters (a memory-saving mode) is out of scope.

Images are not part of ``state_dict`` and are built eagerly, so a ``GraphDecoder`` constructed
after the call captures the fp8 kernels. An image records its parameter's ``_version`` and
``data_ptr()``; using it after the weight was updated in place or moved raises -- requantise.

    from solvingpapers_amd.infer import quantize_decode_weights, GraphDecoder
    quantize_decode_weights(model); GraphDecoder(model, ...)
"""
from __future__ import annotations

from fnmatch import fnmatch

import torch

ATTR = "_spa_w8"


def _model_dtype(model):
    for p in model.parameters():
        if p.is_floating_point():
            return p.dtype
    return None


def _ineligible(p, dtype):
    """why ``p`` keeps its bf16 product, or None if it can carry an image"""
    if p.dim() not in (2, 3):
        return f"{p.dim()}-D"
    if not p.is_floating_point() or p.dtype != dtype:
        return f"dtype {p.dtype} is not the model's {dtype}"
    if p.is_cuda and p.dtype != torch.bfloat16:
        return f"dtype {p.dtype}: the HIP kernels read bf16 activations"
    N, K = p.shape[-2:]
    if N % 128 or K % 128 or N == 0 or K == 0:
        return f"N = {N}, K = {K} not multiples of 128"
    return None


@torch.no_grad()
def quantize_decode_weights(model, skip=()) -> dict:
    """Attach an fp8 decode image to every eligible parameter of ``model``: 2-D ``[N, K]`` or 3-D
    ``[E, N, K]``, of the model's floating dtype, N and K multiples of 128. ``skip``: parameter
    names (fnmatch patterns) to leave in bf16. Returns a report::

        {"quantized": [names], "bf16": {name: reason}, "image_bytes": int, "format": str}

    See the module docstring for what the images change and what they cost."""
    from ..ops.moe import quant_weight_fp8_blk_uncached
    dtype = _model_dtype(model)
    report = {"quantized": [], "bf16": {}, "image_bytes": 0, "format": "fp8-e4m3 128x128 E8M0"}
    for name, p in model.named_parameters():
        why = "skipped by the caller" if any(fnmatch(name, pat) for pat in skip) else _ineligible(p, dtype)
        if why is not None:
            report["bf16"][name] = why
            if hasattr(p, ATTR):
                delattr(p, ATTR)
            continue
        W = p.detach()
        # the quantizer also writes the transposed image (for training's dX): dropped at once
        wq, _, s, _ = quant_weight_fp8_blk_uncached(W if W.dim() == 3 else W.unsqueeze(0))
        if p.dim() == 2:
            wq, s = wq[0], s[0]
        setattr(p, ATTR, (wq, s, p._version, p.data_ptr(), name))
        report["quantized"].append(name)
        report["image_bytes"] += wq.numel() * wq.element_size() + s.numel() * s.element_size()
    return report


def clear_decode_weights(model) -> None:
    """Remove the images: every product runs on the bf16 weights again."""
    for p in model.parameters():
        if hasattr(p, ATTR):
            delattr(p, ATTR)
