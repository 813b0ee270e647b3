"""Weight-only decode: block-scaled e4m3 (fp8) or MXFP4 images of a model's projection matrices.

Decode is weight streaming: every token reads every projection matrix once
(csrc/kernels/gemv.hip). :func:`quantize_decode_weights` builds, for each eligible
parameter, the OCP e4m3 image with one E8M0 scale per 128 x 128 block -- the format of the fp8
training path (ops/moe.py ``quant_weight_fp8_blk``) and of DeepSeek-V3 checkpoints -- and
attaches it to the Parameter. From then on decode-shaped inference products
(``ops.linear.linear`` with <= 4 token rows, ``ops.moe.grouped_linear`` with <= 64 expert rows)
read the image through ``gemv_w8`` / ``grouped_gemv_w8`` (csrc/kernels/gemv.hip): half the
bytes per token.

This mode buys decode speed and COSTS memory: the bf16 master weights stay (prefill, training
and every product with more rows run on them exactly as before), so a model with fp8 images holds
+50 % weight bytes (with MXFP4 images, below, +27 %). Dropping the masters (a memory-saving mode) is out of scope.

``fmt="mxfp4"`` builds OCP MXFP4 images instead (e2m1 codes, one E8M0 scale per 32 consecutive
weights of a row: 4.25 bits per weight, ops/reference.py ``quant_mxfp4``), read through ``gemv_w4`` /
``grouped_gemv_w4``: a quarter of the bf16 bytes per token and +27 % weight memory over the masters
alone, at the accuracy of 4-bit round-to-nearest (about 0.12 relative L2 on Gaussian weights).
A parameter carries one image at a time.

Images are not part of ``state_dict`` and are built eagerly, so a ``GraphDecoder`` constructed
after the call captures the kernels of the chosen format. An image records its parameter's ``_version`` and
``data_ptr()``; using it after the weight was updated in place or moved raises -- requantise.

    from solvingpapers_amd.infer import quantize_decode_weights, GraphDecoder
    quantize_decode_weights(model); GraphDecoder(model, ...)
    quantize_decode_weights(model, fmt="mxfp4"); GraphDecoder(model, ...)
"""
from __future__ import annotations

from fnmatch import fnmatch

import torch

ATTR = "_spa_w8"
ATTR_W4 = "_spa_w4"
FORMATS = {"fp8": "fp8-e4m3 128x128 E8M0", "mxfp4": "mxfp4-e2m1 1x32 E8M0"}


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
def quantize_decode_weights(model, skip=(), fmt="fp8") -> dict:
    """Attach a decode image to every eligible parameter of ``model``: 2-D ``[N, K]`` or 3-D
    ``[E, N, K]``, of the model's floating dtype, N and K multiples of 128. ``skip``: parameter
    names (fnmatch patterns) to leave in bf16. ``fmt``: ``"fp8"`` (e4m3, 128 x 128 block scales) or
    ``"mxfp4"`` (e2m1, 1 x 32 block scales); an image of the other format is removed. Returns a report::

        {"quantized": [names], "bf16": {name: reason}, "image_bytes": int, "format": str}

    See the module docstring for what the images change and what they cost."""
    from ..ops.moe import quant_weight_fp8_blk_uncached, quant_weight_mxfp4
    if fmt not in FORMATS:
        raise ValueError(f"quantize_decode_weights: fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    attr, other = (ATTR, ATTR_W4) if fmt == "fp8" else (ATTR_W4, ATTR)
    dtype = _model_dtype(model)
    report = {"quantized": [], "bf16": {}, "image_bytes": 0, "format": FORMATS[fmt]}
    for name, p in model.named_parameters():
        why = "skipped by the caller" if any(fnmatch(name, pat) for pat in skip) else _ineligible(p, dtype)
        if why is not None:
            report["bf16"][name] = why
            for a in (ATTR, ATTR_W4):
                if hasattr(p, a):
                    delattr(p, a)
            continue
        if hasattr(p, other):
            delattr(p, other)
        W = p.detach()
        W3 = W if W.dim() == 3 else W.unsqueeze(0)
        if fmt == "fp8":
            # the quantizer also writes the transposed image (for training's dX): dropped at once
            wq, _, s, _ = quant_weight_fp8_blk_uncached(W3)
        else:
            wq, s = quant_weight_mxfp4(W3)
        if p.dim() == 2:
            wq, s = wq[0], s[0]
        setattr(p, attr, (wq, s, p._version, p.data_ptr(), name))
        report["quantized"].append(name)
        report["image_bytes"] += wq.numel() * wq.element_size() + s.numel() * s.element_size()
    return report


def clear_decode_weights(model) -> None:
    """Remove the images: every product runs on the bf16 weights again."""
    for p in model.parameters():
        for a in (ATTR, ATTR_W4):
            if hasattr(p, a):
                delattr(p, a)
