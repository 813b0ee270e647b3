"""Every attention kernel path against the fp64 oracle with per-tile bounds (tests/attn_oracle.py):
each output tensor's error per (batch, head, 32-row tile) is bounded by a small multiple of what a
plain emulation of the kernel's roundings achieves on the same inputs, on random, peaked and ramped
scores, at the smallest shapes that reach each path. dQ / dK / dV are written into strided views
with a sentinel row before and after in the token dimension, in the fused-backward child process too
(O and lse are allocated by the ops themselves, so they carry no guard rows; they are checked for
finiteness and against the oracle; the public-op tests go through autograd, which allocates the gradients).

The comment beside each case cites the host condition that routes it (csrc/kernels/attention.hip
unless another file is named)."""
import math
import os
import subprocess
import sys
from collections import namedtuple

import pytest
import torch

import attn_oracle as A
from solvingpapers_amd.ops import _ext
from solvingpapers_amd.ops.attention import dropout_keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 123456789012345
ENV_KEYS = ("SPA_ATTN_XCD", "SPA_ATTN_KSPLIT", "SPA_ATTN_FWD256", "SPA_ATTN_SPLITV", "SPA_ATTN_DQ_DS",
            "SPA_ATTN_DKDV5", "SPA_ATTN_DS_NT", "SPA_ATTN_DKDV256", "SPA_ATTN_DKDV_MLA", "SPA_ATTN_SHORT",
            "SPA_ATTN_DKDV", "SPA_ATTN_KVBLOCKS", "SPA_ATTN_STAMP")

Case = namedtuple("Case", "id B Tq Tk H Hkv dqk dv causal p env kinds dsp")
RANDN = ("randn",)


def C(id, Tq, Tk, H, Hkv, hd, causal=True, p=0.0, env=None, B=2, kinds=A.KINDS, dsp=""):
    """dsp: which gradients come from a dS formed from the bf16 P (attn_oracle._attention ds_p_rounded): "dk" where
    the paired-wave attn_bwd_dkdv3_kernel / dkdv5 computes dK, "dqdk" where the dQ (and dK) passes stream its dS."""
    dqk, dv = hd if isinstance(hd, tuple) else (hd, hd)
    return Case(id, B, Tq, Tk, H, Hkv, dqk, dv, causal, p, dict(env or {}), tuple(kinds), dsp)


MLA = (192, 128)
BF16_CASES = [
    # ---- head dim 64. Forward: attn_fwd_kernel<64,64,8> (HDKV_SWITCH, :1981). Backward: H == Hkv, T <= 256,
    # no dropout -> the fused short kernel (:2243, attention_short.hip launch_bwd_short); else
    # attn_bwd_dq_kernel + single-wave attn_bwd_dkdv_kernel (:2164, :2178; piped needs HDV == 128, :2171)
    C("hd64-short-T1", 1, 1, 2, 2, 64),
    C("hd64-short-T31", 31, 31, 3, 3, 64),
    C("hd64-short-T65-nc", 65, 65, 2, 2, 64, causal=False),
    C("hd64-short-T197-nc", 197, 197, 4, 4, 64, causal=False),          # B * Hkv = 8: XCD order on (:1891)
    C("hd64-short-T197-xcd0", 197, 197, 4, 4, 64, env={"SPA_ATTN_XCD": "0"}, kinds=RANDN),   # :1890
    C("hd64-split-64x325", 64, 325, 2, 2, 64, kinds=RANDN),             # Tk > 256: not short (:2243) -> split
    C("hd64-short-256x131-nc", 256, 131, 2, 2, 64, causal=False),       # Tq > 32, Tk < Tq, short kernel
    C("hd64-short0-T97", 97, 97, 2, 2, 64, env={"SPA_ATTN_SHORT": "0"}),   # :2242 -> split dq + dK/dV
    C("hd64-split-T325", 325, 325, 2, 2, 64),                           # T > 256 (:2243) -> split
    C("hd64-split-gqa2-T33", 33, 33, 4, 2, 64),                         # H != Hkv (:2243); q-head split hsplit = 2 (:2270)
    C("hd64-split-mqa8-T197", 197, 197, 8, 1, 64),                      # hsplit = 8 + attn_kv_reduce_kernel (:2181)
    C("hd64-split-ks3-T325", 325, 325, 4, 1, 64, env={"SPA_ATTN_KSPLIT": "3"}),   # forced odd key split: fwd merge
                                                                        # (:1995) and attn_dq_reduce_kernel (:2166)
    C("hd64-drop0.1-T197", 197, 197, 8, 1, 64, p=0.1),                  # DROP kernels (:1984, :2301)
    C("hd64-drop0.5-T65-nc", 65, 65, 3, 3, 64, causal=False, p=0.5),    # dropout keeps the short kernel off (:2243)
    # ---- head dim 128. Default backward with hsplit == 1 (G == 1 here, :2270) and Tq == Tk: dkdv5 + dS + dq_ds
    # (:2032, :2046, attention_dkdv5.hip launch_dkdv5)
    C("hd128-dkdv5-T1", 1, 1, 2, 2, 128, dsp="dqdk"),
    C("hd128-dkdv5-T33", 33, 33, 2, 2, 128, dsp="dqdk"),
    C("hd128-dkdv5-T64-nc", 64, 64, 4, 4, 128, causal=False, dsp="dqdk"),           # B * Hkv = 8: XCD order on
    C("hd128-dkdv5-T325", 325, 325, 2, 2, 128, dsp="dqdk"),                         # half key block + ragged tail
    C("hd128-dkdv5-256x131-nc", 256, 131, 2, 2, 128, causal=False, dsp="dqdk"),     # non-causal: causal_off not required (:2032)
    C("hd128-dkdv5-gqa4-T197", 197, 197, 8, 2, 128, env={"SPA_ATTN_KVBLOCKS": "1"}, dsp="dqdk"),   # :2268 keeps hsplit == 1, so
                                                                        # GQA reaches the dS path (:2032)
    C("hd128-dkdv5-mqa-T97", 97, 97, 4, 1, 128, env={"SPA_ATTN_KVBLOCKS": "1"}, dsp="dqdk"),
    C("hd128-dkdv3ds-T325", 325, 325, 2, 2, 128, env={"SPA_ATTN_DKDV5": "0"}, dsp="dqdk"),   # :2036 -> delta + dkdv3 storing dS
    C("hd128-dsnt0-T97", 97, 97, 2, 2, 128, env={"SPA_ATTN_DS_NT": "0"}, kinds=RANDN, dsp="dqdk"),   # :2058
    C("hd128-dqds0-T325", 325, 325, 2, 2, 128, env={"SPA_ATTN_DQ_DS": "0"}, dsp="dk"),   # :2029 -> dq kernel + piped dkdv3 (:2171)
    C("hd128-dqds2-T65", 65, 65, 2, 2, 128, env={"SPA_ATTN_DQ_DS": "2"}, kinds=RANDN, dsp="dqdk"),   # :2029: same as default
    C("hd128-dkdv1-T197", 197, 197, 2, 2, 128, env={"SPA_ATTN_DKDV": "1"}),    # :2262, :2032 off -> single-wave dK/dV
    C("hd128-hsplit-gqa8-T65", 65, 65, 16, 2, 128, dsp="dk"),                     # hsplit = 8 (:2270) -> :2032 off: dq kernel +
                                                                        # piped dkdv3 over q-head shares + reduce
    C("hd128-hsplit-gqa2-64x325", 64, 325, 4, 2, 128, dsp="dk"),                  # Tq < Tk: causal_off != 0 (:2032)
    C("hd128-1x77", 1, 77, 4, 2, 128, dsp="dk"),                                  # single decode row, causal_off = 76
    C("hd128-ks3-T325", 325, 325, 2, 1, 128, env={"SPA_ATTN_KSPLIT": "3"}, dsp="dk"),    # forced odd key split
    C("hd128-ksauto-T1024", 1024, 1024, 2, 2, 128, B=1, kinds=RANDN, dsp="dqdk"),   # attn_ksplit auto: ntk = 16 -> 4 shares (:1916)
    C("hd128-drop0.1-T325", 325, 325, 4, 2, 128, p=0.1),                # DROP: dq kernel + single-wave dK/dV (:2011)
    C("hd128-drop0.5-T97", 97, 97, 2, 2, 128, p=0.5),
    # ---- head dim 256. Forward: pshare (default, :1957); SPA_ATTN_FWD256=0 -> split-V (:1959), with
    # SPA_ATTN_SPLITV=0 the single 4-wave kernel. Key split automatic from Tk >= 225 (ntk = cdiv(Tk, 32), :1962).
    # Backward dS path needs wg >= 512 or SPA_ATTN_DQ_DS=2 (:2083)
    C("hd256-T33", 33, 33, 2, 1, 256, env={"SPA_ATTN_DQ_DS": "2"}, dsp="dqdk"),     # hsplit = 2 = G (:2270): paired dV-split + dK
                                                                        # pass + dq_ds256 (:2104)
    C("hd256-T325", 325, 325, 2, 2, 256, env={"SPA_ATTN_DQ_DS": "2"}),  # automatic key split in the forward. Backward: G = 1
                                                                        # and the iteration split gives hsplit = 2 (:2279), so
                                                                        # G % hsplit != 0 (:2104): single-wave dK/dV + dS (:2136)
    C("hd256-T325-ks1", 325, 325, 2, 2, 256, env={"SPA_ATTN_DQ_DS": "2", "SPA_ATTN_KSPLIT": "1"}, kinds=RANDN),   # as above
    C("hd256-T197-ks3-nc", 197, 197, 4, 4, 256, causal=False, env={"SPA_ATTN_DQ_DS": "2", "SPA_ATTN_KSPLIT": "3"}, dsp="dqdk"),
    C("hd256-splitv-T197", 197, 197, 2, 1, 256, env={"SPA_ATTN_FWD256": "0", "SPA_ATTN_DQ_DS": "2",
                                                     "SPA_ATTN_DKDV256": "0"}),   # :2103 -> single-wave dK/dV + dS
    C("hd256-single-T65", 65, 65, 2, 1, 256, env={"SPA_ATTN_FWD256": "0", "SPA_ATTN_SPLITV": "0"}),   # backward: wg < 512
                                                                        # (:2083) -> dq kernel + single-wave dK/dV
    C("hd256-single-64x325", 64, 325, 2, 1, 256, env={"SPA_ATTN_FWD256": "0", "SPA_ATTN_SPLITV": "0"}, kinds=RANDN),
    C("hd256-256x131-nc", 256, 131, 2, 2, 256, causal=False, env={"SPA_ATTN_DQ_DS": "2"}),   # Tq 256: hsplit = 2 (:2279),
                                                                        # G = 1 -> single-wave dK/dV + dS as hd256-T325
    C("hd256-mqa16-T325", 325, 325, 16, 1, 256, env={"SPA_ATTN_DQ_DS": "2"}, dsp="dqdk"),   # q-head split hsplit = 16 (:2270),
                                                                        # G % hsplit == 0 -> dV-split kernel (:2104)
    C("hd256-mqa2-T1024", 1024, 1024, 2, 1, 256, B=1, kinds=RANDN, env={"SPA_ATTN_DQ_DS": "2"}),   # iteration split
                                                                        # hsplit = 8 (:2279), G % 8 != 0 -> single-wave
    C("hd256-512kb-T1024", 1024, 1024, 32, 32, 256, kinds=RANDN, dsp="dqdk"),       # nkv = 8 * 32 * 2 = 512 key blocks: no split;
                                                                        # wg = 8 * 64 = 512 -> dS path by grid size
    C("hd256-drop0.1-T197", 197, 197, 2, 1, 256, p=0.1),                # DROP: 4-wave forward, dq + single-wave dK/dV
    # ---- MLA (192, 128): dS path by grid size or SPA_ATTN_DQ_DS=2 (:2083); paired dK/dV when hsplit == 1 (:2129)
    C("mla-single-T97", 97, 97, 4, 4, MLA, env={"SPA_ATTN_DQ_DS": "2", "SPA_ATTN_DKDV_MLA": "1"}),   # :2129, :2136
    C("mla-paired-T197", 197, 197, 4, 4, MLA, env={"SPA_ATTN_DQ_DS": "2"}, dsp="dqdk"),   # G == 1, Tq < 225: hsplit == 1 (:2279)
    C("mla-dq-T325", 325, 325, 2, 2, MLA),                              # wg < 512 (:2083): dq kernel + single-wave dK/dV
                                                                        # with the iteration split hsplit = 2 (:2279)
    C("mla-paired-grid-T1024", 1024, 1024, 64, 64, MLA, B=1, kinds=RANDN, dsp="dqdk"),   # wg = 512, nkv = 512: paired by grid size
]
BF16_PARAMS = [pytest.param(c, k, id=f"{c.id}-{k}") for c in BF16_CASES for k in c.kinds]

F32_CASES = [
    # csrc/kernels/attention_f32.hip F32_HD_SWITCH (:347): head dims 16 / 64 / 128 / 256; DROP template by p (:393)
    # (fp32 error is a handful of roundings per element: ragged tails of 1 row would compare two numbers, so the
    # tails here keep 5 .. 13 rows; the kernels' query / key tiles are 16 rows, :391, :422)
    C("f32-hd16-T45-nc", 45, 45, 4, 4, 16, causal=False),
    C("f32-hd64-T77-gqa2", 77, 77, 4, 2, 64),
    C("f32-hd64-T109-drop", 109, 109, 2, 1, 64, p=0.1),
    C("f32-hd128-64x325", 64, 325, 4, 2, 128, kinds=RANDN),
    C("f32-hd128-T31-drop", 31, 31, 2, 2, 128, p=0.5, kinds=RANDN),
    C("f32-hd256-T197", 197, 197, 2, 1, 256, kinds=RANDN),
    C("f32-hd256-256x131-nc", 256, 131, 1, 1, 256, causal=False, kinds=RANDN),
]
F32_PARAMS = [pytest.param(c, k, id=f"{c.id}-{k}") for c in F32_CASES for k in c.kinds]
F32_PAD_CASE = C("f32-hd48-pad64-T77", 77, 77, 2, 1, 48)    # ops/attention.py:226: zero-padded to 64

WIDE_CASES = [
    # ops/attention.py:220 _wide_ok: bf16, equal head dims 512 / 768 -> csrc/kernels/attention_wide.hip
    C("wide512-T65-nc", 65, 65, 4, 2, 512, causal=False),
    C("wide768-T97-mqa", 97, 97, 2, 1, 768),
    C("wide768-64x325", 64, 325, 2, 1, 768, kinds=RANDN),
]
WIDE_PARAMS = [pytest.param(c, k, id=f"{c.id}-{k}") for c in WIDE_CASES for k in c.kinds]

PACKED_CASES = [C("packed-hd128-gqa4-T97", 97, 97, 8, 2, 128, dsp="dk"), C("packed-hd64-T65", 65, 65, 2, 2, 64, kinds=RANDN)]
PREFIX_CASES = [C("prefix-hd128-33+64", 64, 97, 4, 2, 128, kinds=RANDN, dsp="dk"), C("prefix-hd256-65+32", 32, 97, 2, 1, 256, kinds=RANDN)]
MLA_FUSED_CASES = [C("mlafused-192-T97", 97, 97, 4, 4, MLA, kinds=RANDN), C("mlafused-128-T65", 65, 65, 2, 2, 128, kinds=RANDN, dsp="dqdk")]
# SPA_ATTN_BWD_FUSED=1 (:2237, read once per process): HDK <= 128, square, no dropout (:2238)
FUSED_CASES = [C("fused-hd128-gqa2-T325", 325, 325, 4, 2, 128), C("fused-hd64-T97-nc", 97, 97, 2, 2, 64, causal=False, kinds=RANDN),
               C("fused-hd128-1x77", 1, 77, 4, 2, 128, kinds=RANDN)]


def all_cases():
    """Every (case, kind, dtype) of this file (tests/test_attn_oracle_cpu.py checks the emulations' spread on them)."""
    out = [(c, k, torch.bfloat16) for c in BF16_CASES + WIDE_CASES + PACKED_CASES + PREFIX_CASES + MLA_FUSED_CASES + FUSED_CASES
           for k in c.kinds]
    out += [(c, k, torch.float32) for c in F32_CASES + [F32_PAD_CASE] for k in c.kinds]
    return out


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    assert _ext.load(), "HIP extension must load on the GPU box"
    for key in ENV_KEYS:
        monkeypatch.delenv(key, raising=False)


SENTINEL = {torch.bfloat16: 1234.0, torch.float32: 1234.5}


def guarded(B, T, H, d, dtype):
    """(buffer [B, T + 2, H, d], view buffer[:, 1:-1]): the view is NaN, the two sentinel rows hold a fixed value."""
    buf = torch.full((B, T + 2, H, d), SENTINEL[dtype], device=DEV, dtype=dtype)
    view = buf[:, 1:-1]
    view.fill_(float("nan"))
    return buf, view


def check_guards(buf, name, errs):
    s = torch.full_like(buf[:, :1], SENTINEL[buf.dtype])
    if not (torch.equal(buf[:, :1], s) and torch.equal(buf[:, -1:], s)):
        errs.append(f"{name}: a sentinel row next to the output view was overwritten")
    if not bool(torch.isfinite(buf[:, 1:-1]).all()):
        bad = (~torch.isfinite(buf[:, 1:-1])).nonzero()[0].tolist()
        errs.append(f"{name}: element (b, t, h, c) = {bad} of the output view was never written (or is non-finite)")


def oracle(c, q, k, v, do, sc, f32=False, fwd=None, defer=True):
    """(ref64, yardstick, fp32 yardsticks). ``fwd`` = the kernel's (O, lse), which the yardsticks' backward
    reads as the backward kernel does (attn_oracle.emulate_bf16)."""
    keep = dropout_keep_mask(SEED, c.B, c.H, c.Tq, c.Tk, c.p, device=q.device) if c.p > 0 else None
    ref = A.ref64(q, k, v, do, c.causal, sc, keep, c.p)
    f32y = (A.emulate_fp32(q, k, v, do, c.causal, sc, keep, c.p, fwd=fwd if f32 else None),
            A.emulate_fp32(q, k, v, do, c.causal, sc, keep, c.p, order="blockwise", block=16, fwd=fwd if f32 else None))
    if f32:
        return ref, f32y, f32y + ((None, A.lse_log2_fp32(q, k, c.causal, sc)),)
    f32y += ((None, A.lse_log2_fp32(q, k, c.causal, sc)),)     # a third lse yardstick (compare() reads [1] only)
    return ref, bf16_yardstick(q, k, v, do, c.causal, sc, keep, c.p, fwd, c.dsp, defer), f32y


def bf16_yardstick(q, k, v, do, causal, sc, keep, p, fwd, dsp, defer=True):
    """The one emulation a bf16 kernel is bounded by: the blockwise ordering over 32-key sub-tiles that its forward's
    source shows. ``defer``: the forward kernels of attention.hip keep a stale row maximum below 2^8 (attn_fwd_kernel
    :192-218, attn_fwd256p_kernel :442); attention_wide.hip rescales at every sub-tile ("exact online softmax (no
    deferral ...)", attention_wide.hip:127) and takes the plain blockwise emulation."""
    return A.emulate_bf16(q, k, v, do, causal, sc, keep, p, fwd=fwd, ds_p_rounded=dsp, order="blockwise", block=32,
                          defer_log2=8.0 if defer else 0.0)


def zero_ref_floor(c, q, k, v, do, sc):
    """Tq == Tk == 1: the softmax has one key, dS = P (dP - delta) is exactly zero and so are dQ and dK; what a
    kernel stores is the fp32 rounding noise of dP - delta, two dv-term dot products of dO with v: at most
    2 * dv * 2^-24 * max|dO| max|v| each, times max|k| or |q| and the scale."""
    if not (c.Tq == 1 and c.Tk == 1):
        return 0.0
    m = lambda t: float(t.abs().max())
    return 4 * c.dv * 2.0 ** -24 * m(do) * m(v) * max(m(k), m(q)) * sc


def compare(c, kind, got, ref, yard, f32y, floor, f32=False, lse=True):
    """got: (O, lse, dQ, dK, dV) of the kernel. Collects every failing tensor before raising; prints the
    worst kernel-to-yardstick ratios (information only)."""
    errs, line = [], []
    rm, mm = (A.F32_RMS_MARGIN, A.F32_MAX_MARGIN) if f32 else (A.RMS_MARGIN, A.MAX_MARGIN)
    for i, name in ((0, "O"), (2, "dQ"), (3, "dK"), (4, "dV")):
        if got[i] is None:
            continue
        fl = floor if name in ("dQ", "dK") else 0.0
        ys = yard[i] if not f32 else [y[i] for y in yard]
        wr, wm, _ = A.worst_ratios(got[i], ref[i], ys, floor=fl)
        line.append(f"{name} {float(wr.max()):.2f}/{float(wm.max()):.2f}")
        try:
            A.assert_tiles(got[i], ref[i], ys, f"{c.id}-{kind} {name}", rm, mm, floor=fl)
        except AssertionError as e:
            errs.append(str(e))
    if lse and got[1] is not None:
        try:
            line.append(f"lse {A.assert_lse(got[1], ref[1], [y[1] for y in f32y], f'{c.id}-{kind} lse'):.2f}")
        except AssertionError as e:
            errs.append(str(e))
    print(f"RATIO {c.id} {kind}: " + "  ".join(line) + ("  FAIL" if errs else ""))
    return errs


def inputs(c, kind, dtype=torch.bfloat16):
    sc = 1.0 / math.sqrt(c.dqk)
    return A.make_inputs(kind, c.B, c.Tq, c.Tk, c.H, c.Hkv, c.dqk, c.dv, sc, dtype, DEV) + (sc,)


def run_direct(c, kind, monkeypatch, fwd, bwd, dtype=torch.bfloat16, f32=False, drop_args=True, defer=True):
    for key, val in c.env.items():
        monkeypatch.setenv(key, val)
    q, k, v, do, sc = inputs(c, kind, dtype)
    extra = (c.p, SEED, None) if drop_args else ()
    out, lse = fwd(q, k, v, sc, c.causal, *extra)
    (bq, dq), (bk, dk), (bv, dv) = (guarded(c.B, c.Tq, c.H, c.dqk, dtype), guarded(c.B, c.Tk, c.Hkv, c.dqk, dtype),
                                    guarded(c.B, c.Tk, c.Hkv, c.dv, dtype))
    bwd(do, q, k, v, out, lse, dq, dk, dv, sc, c.causal, *extra)
    torch.cuda.synchronize()
    errs = []
    for buf, name in ((bq, "dQ"), (bk, "dK"), (bv, "dV")):
        check_guards(buf, name, errs)
    if not bool(torch.isfinite(out).all()):
        errs.append("O: non-finite values")
    if not errs:
        ref, yard, f32y = oracle(c, q, k, v, do, sc, f32, fwd=(out, lse), defer=defer)
        errs += compare(c, kind, (out, lse, dq, dk, dv), ref, yard, f32y, zero_ref_floor(c, q, k, v, do, sc), f32)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("c,kind", BF16_PARAMS)
def test_bf16_kernels(c, kind, monkeypatch):
    ops = _ext.ops()
    run_direct(c, kind, monkeypatch, ops.attn_fwd, ops.attn_bwd)


@pytest.mark.parametrize("c,kind", F32_PARAMS)
def test_f32_kernels(c, kind, monkeypatch):
    ops = _ext.ops()
    run_direct(c, kind, monkeypatch, ops.attn_f32_fwd, ops.attn_f32_bwd, torch.float32, f32=True)


@pytest.mark.parametrize("c,kind", WIDE_PARAMS)
def test_wide_kernels(c, kind, monkeypatch):
    ops = _ext.ops()
    run_direct(c, kind, monkeypatch, ops.attn_wide_fwd, ops.attn_wide_bwd, drop_args=False, defer=False)


def test_f32_padded_head_dim():
    """Head dim 48 through the public op: zero-padded onto the 64-wide fp32 kernel (ops/attention.py:226)."""
    from solvingpapers_amd.ops import flash_attention
    c = F32_PAD_CASE
    q, k, v, do, sc = inputs(c, "randn", torch.float32)
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    o = flash_attention(q, k, v, causal=True, scale=sc)
    o.backward(do)
    ref, yard, f32y = oracle(c, q.detach(), k.detach(), v.detach(), do, sc, True, fwd=(o.detach(), None))
    errs = compare(c, "randn", (o.detach(), None, q.grad, k.grad, v.grad), ref, yard, f32y, 0.0, True)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("c", PACKED_CASES, ids=lambda c: c.id)
def test_attention_packed(c):
    """ops.attention_packed: q / k / v and the three gradients as slices of one packed buffer."""
    from solvingpapers_amd.ops import attention_packed
    q, k, v, do, sc = inputs(c, "randn")
    qkv = torch.cat([q, k, v], dim=2).reshape(c.B, c.Tq, -1).requires_grad_()
    o = attention_packed(qkv, c.H, c.Hkv, causal=True, scale=sc, head_dim=c.dqk)
    o.backward(do.reshape(c.B, c.Tq, -1))
    g = qkv.grad.view(c.B, c.Tq, c.H + 2 * c.Hkv, c.dqk)
    ref, yard, f32y = oracle(c, q, k, v, do, sc, fwd=(o.detach().view(c.B, c.Tq, c.H, c.dv), None))
    got = (o.detach().view(c.B, c.Tq, c.H, c.dv), None, g[:, :, :c.H], g[:, :, c.H:c.H + c.Hkv], g[:, :, c.H + c.Hkv:])
    errs = compare(c, "randn", got, ref, yard, f32y, 0.0)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("c", PREFIX_CASES, ids=lambda c: c.id)
def test_attention_packed_prefix(c):
    """ops.attention_packed_prefix: chunk B's queries (the last Tq positions) over chunk A's keys and its own."""
    from solvingpapers_amd.ops.attention import attention_packed_prefix
    q, k, v, do, sc = inputs(c, "randn")
    Ta = c.Tk - c.Tq
    qa = torch.zeros(c.B, Ta, c.H, c.dqk, device=DEV, dtype=torch.bfloat16)     # chunk A's queries take no part
    a = torch.cat([qa, k[:, :Ta], v[:, :Ta]], dim=2).reshape(c.B, Ta, -1).requires_grad_()
    b = torch.cat([q, k[:, Ta:], v[:, Ta:]], dim=2).reshape(c.B, c.Tq, -1).requires_grad_()
    o = attention_packed_prefix(b, a, c.H, c.Hkv, c.dqk, scale=sc)
    o.backward(do.reshape(c.B, c.Tq, -1))
    ga = a.grad.view(c.B, Ta, c.H + 2 * c.Hkv, c.dqk)
    gb = b.grad.view(c.B, c.Tq, c.H + 2 * c.Hkv, c.dqk)
    assert not bool(ga[:, :, :c.H].any()), "chunk A's q columns get no gradient from chunk B"
    dk = torch.cat([ga[:, :, c.H:c.H + c.Hkv], gb[:, :, c.H:c.H + c.Hkv]], dim=1)
    dv = torch.cat([ga[:, :, c.H + c.Hkv:], gb[:, :, c.H + c.Hkv:]], dim=1)
    ref, yard, f32y = oracle(c, q, k, v, do, sc, fwd=(o.detach().view(c.B, c.Tq, c.H, c.dv), None))
    errs = compare(c, "randn", (o.detach().view(c.B, c.Tq, c.H, c.dv), None, gb[:, :, :c.H], dk, dv), ref, yard, f32y, 0.0)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("c", MLA_FUSED_CASES, ids=lambda c: c.id)
def test_mla_attention_fused(c):
    """ops.mla_attention's fused path: O, dQ and dV of the attention core against the oracle fed with the
    assembled (rotated) heads; the rope and head-sum glue around it is covered by
    test_mla_attention_fused_matches_composition."""
    from solvingpapers_amd.ops.attention import mla_attention
    from solvingpapers_amd.ops.rope import apply_rope
    dr, theta = 64, 10000.0
    dn = c.dqk - dr
    q, k, v, do, sc = inputs(c, "randn")
    kr = k[:, :, :1, dn:].contiguous()
    kv = torch.cat([k[..., :dn], v], dim=-1)
    q_, kv_, kr_ = (t.clone().requires_grad_() for t in (q, kv, kr))
    o = mla_attention(q_, kv_, kr_, dn, sc, theta)
    o.backward(do)
    with torch.no_grad():      # the heads the kernels see: rope applied in bf16, the rope key shared by all heads
        qf = torch.cat([q[..., :dn], apply_rope(q[..., dn:], theta, 0)], dim=-1)
        kf = torch.cat([k[..., :dn], apply_rope(kr, theta, 0).expand(c.B, c.Tk, c.H, dr)], dim=-1)
    ref, yard, f32y = oracle(c, qf, kf, v, do, sc, fwd=(o.detach(), None))
    got = (o.detach(), None, None, None, kv_.grad[..., dn:])
    errs = compare(c, "randn", got, ref, yard, f32y, 0.0)
    # the nope columns of dQ / dK pass through unrotated
    for name, g, i in (("dQ nope", q_.grad[..., :dn], 2), ("dK nope", kv_.grad[..., :dn], 3)):
        try:
            A.assert_tiles(g, ref[i][..., :dn], yard[i][..., :dn], f"{c.id} {name}")
        except AssertionError as e:
            errs.append(str(e))
    assert not errs, "\n".join(errs)


CHILD = """
import math, sys, torch
sys.path.insert(0, sys.argv[2])
import attn_oracle as A
from solvingpapers_amd.ops import _ext
ops = _ext.ops()
res = {}
def guarded(t):      # as guarded() of the parent: a NaN view between two sentinel rows
    buf = torch.full((t.shape[0], t.shape[1] + 2) + tuple(t.shape[2:]), SENTINEL, device=t.device, dtype=t.dtype)
    buf[:, 1:-1].fill_(float("nan"))
    return buf
for (cid, B, Tq, Tk, H, Hkv, hd, causal, kind) in CASES:
    sc = 1.0 / math.sqrt(hd)
    q, k, v, do = A.make_inputs(kind, B, Tq, Tk, H, Hkv, hd, hd, sc, torch.bfloat16, "cuda")
    o, lse = ops.attn_fwd(q, k, v, sc, causal)
    bq, bk, bv = guarded(q), guarded(k), guarded(v)
    ops.attn_bwd(do, q, k, v, o, lse, bq[:, 1:-1], bk[:, 1:-1], bv[:, 1:-1], sc, causal)
    torch.cuda.synchronize()
    res[cid + "-" + kind] = [t.cpu() for t in (o, lse, bq, bk, bv)]
torch.save(res, sys.argv[1])
"""


def test_bwd_fused_in_child(tmp_path):
    """SPA_ATTN_BWD_FUSED=1 (dQ by fp32 atomics inside the dK/dV kernel) is read once per process: a fresh
    child runs the kernels (gradients into views between sentinel rows) and saves the buffers, this process checks
    the sentinels and applies the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = [(c.id, c.B, c.Tq, c.Tk, c.H, c.Hkv, c.dqk, c.causal, k) for c in FUSED_CASES for k in c.kinds]
    path = str(tmp_path / "fused.pt")
    env = dict(os.environ, PYTHONPATH=root, SPA_ATTN_BWD_FUSED="1")
    for key in ENV_KEYS:
        env.pop(key, None)
    subprocess.run([sys.executable, "-c", CHILD.replace("CASES", repr(cases)).replace("SENTINEL", repr(SENTINEL[torch.bfloat16])), path, os.path.join(root, "tests")],
                   check=True, env=env, cwd=root, timeout=120)
    res = torch.load(path, weights_only=True)
    errs = []
    for c in FUSED_CASES:
        for kind in c.kinds:
            q, k, v, do, sc = inputs(c, kind)
            got = [t.to(DEV) for t in res[f"{c.id}-{kind}"]]
            for buf, name in zip(got[2:], ("dQ", "dK", "dV")):
                check_guards(buf, f"{c.id}-{kind} {name}", errs)
            got[2:] = [buf[:, 1:-1] for buf in got[2:]]
            ref, yard, f32y = oracle(c, q, k, v, do, sc, fwd=(got[0], got[1]))
            errs += compare(c, kind, got, ref, yard, f32y, 0.0)
    assert not errs, "\n".join(errs)
