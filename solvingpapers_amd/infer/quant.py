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

``max_rows`` (opt-in, default 4 = the GEMV's limit): with ``max_rows=R``, 5 <= R <= 16, inference products of
5..R token rows on a weight that carries an image ALSO read the image, through the MFMA weight-streaming
kernel ``skinny_gemm_w8`` / ``skinny_gemm_w4`` (csrc/kernels/skinny_gemm.hip; on the CPU the dequantised oracle
product). Contract: ``y = bf16(x . dequant(W)^T)`` with exact products and fp32 accumulation, activations NOT
quantised; each output row is a function of its own input row, the image and (N, K) only -- bitwise the same
whatever the other rows hold and however many there are -- so a slot's logits still do not depend on its
neighbours. It applies to ANY such product, not only a one-token step of a batch of R: a 10-token
``prefill_row`` reads the images too, and so does the 8-row product that runs on the masters at the default.
Products of 1..4 rows and of more than R rows, weights without an image, autograd and biased products take
exactly the routes they take at the default. What it costs: nothing in memory (the same images); accuracy is
that of the image at these batch sizes too (MXFP4: about 0.12 relative L2 on Gaussian weights), where the
default keeps bf16-master accuracy above 4 rows. Measured: profiles/skinny_decode_gemm.txt.
Not covered: more than 16 rows (one MFMA row tile), the grouped (MoE expert) route (``grouped_gemv_*`` already
serves <= 64 expert rows), a bf16-master instantiation or any change of the default route, dropping the
masters, activation quantisation (the block-scaled fp8 / fp4 MFMA), tensor-parallel decode.

Images are not part of ``state_dict`` and are built eagerly, so a ``GraphDecoder`` constructed
after the call captures the kernels of the chosen format. An image records its parameter's ``_version`` and
``data_ptr()``; using it after the weight was updated in place or moved raises -- requantise.

    from solvingpapers_amd.infer import quantize_decode_weights, GraphDecoder
    quantize_decode_weights(model); GraphDecoder(model, ...)
    quantize_decode_weights(model, fmt="mxfp4"); GraphDecoder(model, ...)
    quantize_decode_weights(model, max_rows=16); GraphDecoder(model, 16, ...)   # batch 5..16 reads the images
"""
from __future__ import annotations

from fnmatch import fnmatch

import torch

ATTR = "_spa_w8"
ATTR_W4 = "_spa_w4"
ATTR_ROWS = "_spa_wrows"       # int beside the image: products of up to this many rows read it (ops/linear.py)
MIN_ROWS, MAX_ROWS = 4, 16     # the GEMV's row limit (the default) .. one MFMA row tile
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
def quantize_decode_weights(model, skip=(), fmt="fp8", max_rows=MIN_ROWS) -> dict:
    """Attach a decode image to every eligible parameter of ``model``: 2-D ``[N, K]`` or 3-D
    ``[E, N, K]``, of the model's floating dtype, N and K multiples of 128. ``skip``: parameter
    names (fnmatch patterns) to leave in bf16. ``fmt``: ``"fp8"`` (e4m3, 128 x 128 block scales) or
    ``"mxfp4"`` (e2m1, 1 x 32 block scales); an image of the other format is removed. ``max_rows``: an int
    in [4, 16], kept beside each image (``_spa_wrows``): inference products of up to that many token rows read
    the image (4, the default: the GEMV routes alone, as before the option existed). Returns a report::

        {"quantized": [names], "bf16": {name: reason}, "image_bytes": int, "format": str, "max_rows": int}

    See the module docstring for what the images change and what they cost."""
    from ..ops.moe import quant_weight_fp8_blk_uncached, quant_weight_mxfp4
    if fmt not in FORMATS:
        raise ValueError(f"quantize_decode_weights: fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    if type(max_rows) is not int or not MIN_ROWS <= max_rows <= MAX_ROWS:
        raise ValueError(f"quantize_decode_weights: max_rows must be an int in [{MIN_ROWS}, {MAX_ROWS}], "
                         f"got {max_rows!r}")
    attr, other = (ATTR, ATTR_W4) if fmt == "fp8" else (ATTR_W4, ATTR)
    dtype = _model_dtype(model)
    report = {"quantized": [], "bf16": {}, "image_bytes": 0, "format": FORMATS[fmt],
              "max_rows": max_rows}
    for name, p in model.named_parameters():
        why = "skipped by the caller" if any(fnmatch(name, pat) for pat in skip) else _ineligible(p, dtype)
        if why is not None:
            report["bf16"][name] = why
            for a in (ATTR, ATTR_W4, ATTR_ROWS):
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
        setattr(p, ATTR_ROWS, max_rows)
        report["quantized"].append(name)
        report["image_bytes"] += wq.numel() * wq.element_size() + s.numel() * s.element_size()
    return report


def clear_decode_weights(model) -> None:
    """Remove the images: every product runs on the bf16 weights again."""
    for p in model.parameters():
        for a in (ATTR, ATTR_W4, ATTR_ROWS):
            if hasattr(p, a):
                delattr(p, a)
