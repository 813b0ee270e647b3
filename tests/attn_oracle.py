"""Per-tile error bounds for the attention kernels against an fp64 oracle (pure torch, any device).

``ref64`` is materialised fp64 attention (forward, lse and the three input gradients by explicit
formulas). ``emulate_bf16`` / ``emulate_fp32`` compute the same operation with only the roundings
every flash kernel of that precision has to make, in one of two legitimate orderings: materialised
softmax, or blockwise online softmax over key tiles. ``tile_errors`` measures a result against
``ref64`` per (batch, head, 32-row tile); ``assert_tiles`` bounds the kernel's per-tile error by a
small multiple of the emulation's error on the same inputs -- a self-calibrating bound, no fixed
constants.

Roundings of the bf16 emulation (the least a bf16 flash kernel does): inputs bf16, S fp32, P rounded
to bf16 before P V and before dV = P^T dO, O rounded to bf16, delta = rowsum(dO * O_bf16), dS rounded
to bf16 before dQ = dS K and dK = dS^T Q, GQA group sums in fp32, outputs rounded to bf16. The
blockwise ordering rounds P against the running row maximum and rescales the fp32 accumulator; its
backward reads that forward's O and lse (the fp32 sums of the backward do not depend on the order
beyond fp32 rounding).

Margins in force (kernel tile error <= margin x yardstick tile error):

    bf16:  RMS 2.13, max-abs 4.0  yardstick: ONE emulation, the blockwise ordering over 32-key sub-tiles that
                                  the forward kernel's source shows (tests/test_attention_tiles_gpu.py
                                  bf16_yardstick: with the deferred rescale for attention.hip, without for
                                  attention_wide.hip)
    fp32:  RMS 4.0, max-abs 4.0   yardstick: per tile, the larger of the materialised and the
                                  16-key blockwise fp32 emulation
    lse:   |lse - lse64| <= 4.0 x the yardstick's max |lse error| per (b, h); the yardstick is the
           largest of the two fp32 emulations, the same sum formed in log2 units as the kernels form it
           (lse_log2_fp32) and half an fp32 ulp of the largest |lse| of that (b, h): lse is stored in
           fp32, and at one key (lse = s) both emulations are exact while any stored value rounds

Observed spread between the materialised and the blockwise ordering (tests/test_attn_oracle_cpu.py
asserts it on every shape and input kind of tests/test_attention_tiles_gpu.py; worst per-tile ratio,
either one as the yardstick of the other):

    bf16 O        RMS 1.42   max-abs 2.05     -> RMS margin 1.5 x 1.42 = 2.13 (1.42 exceeds the 1.38 that a
                                                 margin of 2 covers); max-abs 2.05 is below 2.47: margin 4
    fp32 O        RMS 1.37   max-abs 1.97     -> margins 4 / 4
    dQ, dK, dV    not a measurement: the yardstick's backward reads the O and lse of the result it is
                  compared with (``fwd``), and given the same O and lse the backward is the same
                  computation in both orderings, so the ratio is 1.00 by construction.

    With each ordering's backward reading its own forward the dQ / dK spread is up to 6.1x RMS in
    bf16 (ragged tails of 1 and 5 rows at T = 65 / 97 / 197 / 325; up to 2.4x on full tiles of peaked and
    ramped scores) and 10.8x in fp32. The cause is one number per query row: delta = rowsum(dO * O)
    carries the rounding of O, enters dS = P (dP - delta) coherently along the row and is amplified by
    dQ = dS K on peaked rows, so a small tile's error is the ratio of a few random draws. A backward
    kernel reads the O it is given; so does the yardstick, and the draw is common to both. O and lse
    are bounded on their own in the same test. For the same reason the fp32 cases avoid one-row ragged
    tails (a handful of fp32 roundings per element, 16 elements per row at head dim 16).

Kernel-specific steps (each off unless asked for, source cited at the step in _attention):
    ds_p_rounded  paired-wave dK/dV kernels form dS from the bf16 P. Without it their dK and the dQ / dK
                  streamed from their dS measure 1.3 - 2.0x the plain emulation's RMS (up to 3.7x on
                  one-row tiles); with it 1.00 - 1.44.
    defer_log2    the forward's deferred rescale. Against the materialised emulation two one-row tiles
                  measure 2.03x and 2.22x (hd 128, peaked b=1 head=10 row 64 of T = 65; ramp_hi b=0 head=2
                  of Tq 1 x Tk 77: the last 13-key sub-tile raises the maximum by 4.9 < 8 log2 units, so P
                  keeps the stale maximum); against this ordering both measure 1.00. The emulation alone
                  reproduces the 2.22x on the CPU (tests/test_attn_oracle_cpu.py prints it).

A reference tile that is exactly zero (dQ / dK of a one-key softmax) has no relative error: such
tiles are measured absolutely, and the caller passes the fp32 cancellation noise it derives for the
case as ``floor``.
"""
import math

import torch

RMS_MARGIN, MAX_MARGIN = 2.13, 4.0         # bf16 kernels (1.5 x the observed 1.42; see above)
F32_RMS_MARGIN, F32_MAX_MARGIN = 4.0, 4.0  # fp32 kernels
LSE_MARGIN = 4.0
TILE = 32


def visible_mask(Tq, Tk, causal, device):
    """Bool [Tq, Tk], bottom-right aligned causal mask (ops/reference.py attention)."""
    if not causal:
        return torch.ones(Tq, Tk, dtype=torch.bool, device=device)
    i = torch.arange(Tq, device=device)[:, None]
    j = torch.arange(Tk, device=device)[None, :]
    return j <= i + (Tk - Tq)


def _attention(q, k, v, do, causal, scale, keep_mask, p, dt, rd, order, block, vis=None, fwd=None, ds_p_rounded="",
               defer_log2=0.0):
    """Forward + backward in dtype ``dt`` with rounding ``rd`` at the low-precision points.
    Returns (O, lse, dQ, dK, dV) in [B, T, H, d] layout, dtype dt (values already rounded by rd)."""
    B, Tq, H, _ = q.shape
    Tk, Hkv = k.shape[1], k.shape[2]
    G = H // Hkv
    qh = q.to(dt).transpose(1, 2)                                   # [B, H, Tq, dk]
    kh = k.to(dt).transpose(1, 2).repeat_interleave(G, dim=1)       # [B, H, Tk, dk]
    vh = v.to(dt).transpose(1, 2).repeat_interleave(G, dim=1)       # [B, H, Tk, dv]
    doh = do.to(dt).transpose(1, 2)                                 # [B, H, Tq, dv]
    if vis is None:
        vis = visible_mask(Tq, Tk, causal, q.device)
    S = (qh @ kh.transpose(-1, -2)) * scale
    S = S.masked_fill(~vis, float("-inf"))
    ds_ = 1.0 / (1.0 - p) if p > 0 else 1.0
    keep = keep_mask.to(dt) if (p > 0 and keep_mask is not None) else None
    if order == "materialised":
        m = S.amax(-1, keepdim=True)
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        E = torch.exp(S - m)
        l = E.sum(-1, keepdim=True)
        acc = rd(E if keep is None else E * keep) @ vh
    else:
        m = torch.full((B, H, Tq, 1), float("-inf"), dtype=dt, device=q.device)
        l = torch.zeros_like(m)
        acc = torch.zeros(B, H, Tq, vh.shape[-1], dtype=dt, device=q.device)
        for j0 in range(0, Tk, block):
            Sb = S[..., j0:j0 + block]
            mn = torch.maximum(m, Sb.amax(-1, keepdim=True))
            if defer_log2 > 0:
                # kernel-specific step, on request: the bf16 forward kernels keep a stale row maximum until a
                # sub-tile's maximum exceeds it by 2^8 (csrc/kernels/attention.hip:200 and :442, kRescaleThr in
                # csrc/include/attn_common.h:18), so P (up to 256) is rounded at other mantissas
                mn = torch.where(mn > m + defer_log2 * 0.69314718055994531, mn, m)
            ms = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
            alpha = torch.exp(m - ms)
            Eb = torch.exp(Sb - ms)
            l = l * alpha + Eb.sum(-1, keepdim=True)
            Pb = rd(Eb if keep is None else Eb * keep[..., j0:j0 + block])
            acc = acc * alpha + Pb @ vh[..., j0:j0 + block, :]
            m = mn
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    live = l > 0
    O = rd(torch.where(live, acc * (ds_ / l), torch.zeros_like(acc)))
    lse = torch.where(live, m + torch.log(l), torch.full_like(m, float("-inf")))   # -inf: no visible key
    O_out, lse_out = O, lse
    if fwd is not None:       # the backward reads a given forward result (a kernel's: +inf marks a dead row)
        O = fwd[0].to(dt).transpose(1, 2)
        if fwd[1] is not None:
            lse = fwd[1].to(dt).unsqueeze(-1)
            live = torch.isfinite(lse)
    # backward from the stored (rounded) O and lse
    P = torch.exp(S - torch.where(live, lse, torch.zeros_like(lse)))
    P = torch.where(live, P, torch.zeros_like(P))
    Pd = P if keep is None else P * keep * ds_
    dV = (rd(Pd).transpose(-1, -2) @ doh).view(B, Hkv, G, Tk, -1).sum(2)
    dP = doh @ vh.transpose(-1, -2)
    if keep is not None:
        dP = dP * keep * ds_
    delta = (doh * O).sum(-1, keepdim=True)
    dS = rd(P * (dP - delta))
    # kernel-specific step, on request: the paired-wave dK/dV kernels hand P from one wave to the other as
    # bf16 and form dS = (float)P_bf16 * (dP - delta) before rounding dS itself (csrc/kernels/attention.hip
    # :1312-1320, the bf16 P stores at :1277-1278; csrc/kernels/attention_dkdv5.hip:321-329). Their dK, and the dQ / dK of
    # the passes that stream the dS they store, carry both roundings.
    dS2 = rd(rd(P) * (dP - delta)) if ds_p_rounded else dS
    dQ = ((dS2 if "dq" in ds_p_rounded else dS) @ kh) * scale
    dK = ((dS2 if "dk" in ds_p_rounded else dS).transpose(-1, -2) @ qh).view(B, Hkv, G, Tk, -1).sum(2) * scale
    t = lambda x: rd(x).transpose(1, 2)
    return O_out.transpose(1, 2), lse_out.squeeze(-1), t(dQ), t(dK), t(dV)


def ref64(q, k, v, do, causal, scale, keep_mask=None, p=0.0, vis=None):
    """Materialised fp64 attention with GQA mapping and bottom-right causal alignment. Returns
    (O [B,Tq,H,dv], lse [B,H,Tq], dQ, dK, dV), all fp64. ``keep_mask``: ops.attention.dropout_keep_mask
    (bool [B,H,Tq,Tk]) for dropout ``p``. ``vis`` (bool [Tq,Tk]) overrides the mask (test mutations)."""
    return _attention(q, k, v, do, causal, scale, keep_mask, p, torch.float64, lambda x: x, "materialised", 0, vis)


def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def emulate_bf16(q, k, v, do, causal, scale, keep_mask=None, p=0.0, order="materialised", block=32, vis=None,
                 fwd=None, ds_p_rounded="", defer_log2=0.0):
    """The operation with exactly the roundings of a bf16 flash kernel (module docstring); ``order``
    "materialised" or "blockwise" (online softmax over ``block``-key tiles). Returns fp32 tensors
    holding bf16 values (lse fp32). ``fwd`` = (O, lse): the backward reads this forward result instead of
    the emulation's own (the returned O and lse stay the emulation's), as a backward kernel reads the
    O and lse it is handed: delta = rowsum(dO * O) then carries the same rounding of O in the kernel
    and in the yardstick. That rounding is one scalar per query row which dQ / dK amplify on peaked
    scores; left independent, it makes the error ratio of a ragged tile with a few rows the ratio of
    a few random numbers (observed up to 6x between the two orderings). ``ds_p_rounded``: "dk" or "dqdk",
    the gradients whose dS is formed from the bf16 P; ``defer_log2``: the blockwise ordering's deferred
    rescale threshold in log2 units (both in _attention)."""
    q, k, v, do = (_bf16(t.float()) for t in (q, k, v, do))
    return _attention(q, k, v, do, causal, scale, keep_mask, p, torch.float32, _bf16, order, block, vis, fwd, ds_p_rounded, defer_log2)


def emulate_fp32(q, k, v, do, causal, scale, keep_mask=None, p=0.0, order="materialised", block=16, vis=None,
                 fwd=None):
    """The operation in fp32 throughout (the yardstick of csrc/kernels/attention_f32.hip and of lse)."""
    return _attention(q, k, v, do, causal, scale, keep_mask, p, torch.float32, lambda x: x, order, block, vis, fwd)


def lse_log2_fp32(q, k, causal, scale):
    """lse as every forward kernel here forms it, in fp32: scores in log2 units (s * scale * log2 e), lse = (m +
    log2 l) * ln 2 (csrc/kernels/attention.hip:316, attention_f32.hip:213, attention_wide.hip:164). [B, H, Tq]."""
    G = q.shape[2] // k.shape[2]
    qh = q.float().transpose(1, 2)
    kh = k.float().transpose(1, 2).repeat_interleave(G, dim=1)
    c = torch.tensor(scale * 1.4426950408889634, dtype=torch.float32)
    S = (qh @ kh.transpose(-1, -2)) * c
    S = S.masked_fill(~visible_mask(q.shape[1], k.shape[1], causal, q.device), float("-inf"))
    m = S.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    l = torch.exp2(S - m).sum(-1, keepdim=True)
    return torch.where(l > 0, (m + torch.log2(l)) * 0.69314718055994531, torch.full_like(m, float("-inf"))).squeeze(-1)


def tile_errors(x, ref, rows=TILE):
    """x, ref [B, T, H, d] -> (rms [B, H, nt], maxabs [B, H, nt]): per (batch, head, ``rows``-row
    tile) the RMS error and the max abs error, both divided by the RMS of the reference tile (the
    ragged last tile counted by its real rows; an exactly-zero reference tile divides by 1)."""
    x, ref = x.double(), ref.double()
    B, T, H, d = ref.shape
    nt = (T + rows - 1) // rows
    pad = nt * rows - T
    e = (x - ref).transpose(1, 2)                    # [B, H, T, d]
    r = ref.transpose(1, 2)
    if pad:
        e = torch.nn.functional.pad(e, (0, 0, 0, pad))
        r = torch.nn.functional.pad(r, (0, 0, 0, pad))
    e = e.reshape(B, H, nt, rows * d)
    r = r.reshape(B, H, nt, rows * d)
    n = torch.full((nt,), float(rows * d), dtype=torch.float64, device=ref.device)
    n[-1] = float((T - (nt - 1) * rows) * d)
    rr = (r.square().sum(-1) / n).sqrt()
    rr = torch.where(rr == 0, torch.ones_like(rr), rr)
    return (e.square().sum(-1) / n).sqrt() / rr, e.abs().amax(-1) / rr


def yard_errors(yard, ref, rows=TILE):
    """Tile errors of the yardstick: one tensor, or the per-tile larger of several."""
    ys = yard if isinstance(yard, (list, tuple)) else [yard]
    es = [tile_errors(y, ref, rows) for y in ys]
    return (torch.stack([e[0] for e in es]).amax(0), torch.stack([e[1] for e in es]).amax(0))


def worst_ratios(x, ref, yard, rows=TILE, floor=0.0):
    """(worst rms ratio, worst maxabs ratio, per-tile tensors) of x against the yardstick."""
    kr, km = tile_errors(x, ref, rows)
    yr, ym = yard_errors(yard, ref, rows)
    yr, ym = yr.clamp_min(floor), ym.clamp_min(floor)
    tiny = 1e-300
    return kr / yr.clamp_min(tiny), km / ym.clamp_min(tiny), (kr, km, yr, ym)


def assert_tiles(x, ref, yard, name, rms_margin=RMS_MARGIN, max_margin=MAX_MARGIN, rows=TILE, floor=0.0):
    """Every tile of x: rms error <= rms_margin x the yardstick's, max-abs error <= max_margin x the
    yardstick's (both against ``ref``). Fails with the worst tile's (b, head, first row), its error
    and the yardstick's. Returns the worst (rms, maxabs) ratios."""
    assert x.shape == ref.shape, (name, tuple(x.shape), tuple(ref.shape))
    assert bool(torch.isfinite(x).all()), f"{name}: non-finite values"
    rr, rm, (kr, km, yr, ym) = worst_ratios(x, ref, yard, rows, floor)
    bad_r = kr > rms_margin * yr
    bad_m = km > max_margin * ym
    for what, bad, ratio, ke, ye, margin in (("rms", bad_r, rr, kr, yr, rms_margin),
                                             ("maxabs", bad_m, rm, km, ym, max_margin)):
        if bool(bad.any()):
            score = torch.where(bad, ratio, torch.zeros_like(ratio))
            i = int(score.argmax())
            nt, H = ratio.shape[2], ratio.shape[1]
            b, h, t = i // (H * nt), (i // nt) % H, i % nt
            raise AssertionError(
                f"{name}: {int(bad.sum())} of {bad.numel()} tiles over the {what} bound; worst (b={b}, head={h}, "
                f"first row={t * rows}): {what} error {ke[b, h, t].item():.3e} vs yardstick {ye[b, h, t].item():.3e} "
                f"(ratio {ratio[b, h, t].item():.2f} > {margin})")
    return float(rr.max()), float(rm.max())


def assert_lse(lse, lse64, yard_lses, name, margin=LSE_MARGIN):
    """|lse - lse64| <= margin x the yardstick's max abs lse error, per (b, h). Rows without a visible
    key (lse64 = -inf) must hold +inf, as the kernels store them (attention.hip: l > 0 ? .. : INFINITY)."""
    lse = lse.double()
    dead = torch.isinf(lse64)
    assert bool((lse[dead] == float("inf")).all()), f"{name}: a row without visible keys must store +inf"
    z = torch.zeros_like(lse64)
    err = torch.where(dead, z, (lse - lse64).abs())
    assert bool(torch.isfinite(err).all()), f"{name}: non-finite lse"
    ys = yard_lses if isinstance(yard_lses, (list, tuple)) else [yard_lses]
    ye = torch.stack([torch.where(dead, z, (y.double() - lse64).abs()).amax(-1) for y in ys]).amax(0)   # [B, H]
    # lse is stored in fp32: no yardstick can claim less than half an ulp of the largest stored value
    ye = torch.maximum(ye, torch.where(dead, z, lse64.abs()).amax(-1) * 2.0 ** -24)
    ke = err.amax(-1)
    bad = ke > margin * ye
    ratio = ke / ye.clamp_min(1e-300)
    if bool(bad.any()):
        i = int(torch.where(bad, ratio, torch.zeros_like(ratio)).argmax())
        b, h = i // ratio.shape[1], i % ratio.shape[1]
        row = int(err[b, h].argmax())
        raise AssertionError(f"{name}: lse of (b={b}, head={h}, row={row}) off by {ke[b, h].item():.3e} vs yardstick "
                             f"{ye[b, h].item():.3e} (ratio {ratio[b, h].item():.2f} > {margin})")
    return float(ratio.max())


def rel(a, b):
    """The whole-tensor measure of the older attention tests (< 2e-2 for O, < 3e-2 for gradients)."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


# ------------------------------------------------------------------ inputs
KINDS = ("randn", "peaked", "ramp_lo", "ramp_hi")
# ramps: scaled scores (in log2 units) grow by this much per 32 keys -- below and above the 2^8
# deferred-rescale threshold of the bf16 forward kernels (attention.hip)
RAMP_LOG2_PER_32 = {"ramp_lo": 3.0, "ramp_hi": 12.0}


def make_inputs(kind, B, Tq, Tk, H, Hkv, dqk, dv, scale, dtype, device, seed=0):
    """(q, k, v, do) of the given input kind, generated on the CPU generator (same values on every
    device) and rounded to ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k = rn(B, Tq, H, dqk), rn(B, Tk, Hkv, dqk)
    v, do = rn(B, Tk, Hkv, dv), rn(B, Tq, H, dv)
    if kind == "peaked":
        q, k = q * 2.5, k * 2.5
    elif kind in RAMP_LOG2_PER_32:
        # randn plus a ramp carried by every column: q += a, k += g * j, with a * dqk * g * scale *
        # log2(e) = the wanted growth per key and the ramp kept below ~2 in k (a >= 1 takes the rest).
        # A ramp in one huge column would make dQ = dS K amplify the single rounding of delta per
        # row far above every other rounding, and the tile error the ratio of two random scalars.
        per_key = RAMP_LOG2_PER_32[kind] / 32.0 / (scale * 1.4426950408889634 * dqk)   # = a * g
        a = max(1.0, per_key * max(Tk - 1, 1) / 2.0)
        q = q + a
        k = k + (per_key / a) * torch.arange(Tk, dtype=torch.float32).view(1, Tk, 1, 1)
    elif kind != "randn":
        raise ValueError(kind)
    return tuple(t.to(dtype).to(device) for t in (q, k, v, do))
