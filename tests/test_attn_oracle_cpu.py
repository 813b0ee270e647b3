"""The per-tile attention oracle (tests/attn_oracle.py) proven on the CPU before the GPU file uses it:
the two legitimate orderings of the emulation stay inside the margins of each other on every shape and
input kind of tests/test_attention_tiles_gpu.py; localised faults that pass the whole-tensor rel
bounds of the older tests are caught; and the CPU routes of the attention ops meet the fp32 yardstick."""
import math

import pytest
import torch

import attn_oracle as A
import test_attention_tiles_gpu as G
from solvingpapers_amd.ops.attention import _materialised, dropout_keep_mask, flash_attention, mla_attention

NAMES = ((0, "O"), (2, "dQ"), (3, "dK"), (4, "dV"))


def _spread_cases():
    seen, out = set(), []
    for c, kind, dt in G.all_cases():
        key = (c.B, c.Tq, c.Tk, c.H, c.Hkv, c.dqk, c.dv, c.causal, c.p, kind, dt)
        if key not in seen:
            seen.add(key)
            out.append(pytest.param(c, kind, dt, id=f"{c.id}-{kind}"))
    return out


@pytest.mark.parametrize("c,kind,dt", _spread_cases())
def test_emulations_stay_within_margins_of_each_other(c, kind, dt):
    """Materialised vs blockwise (32 keys in bf16, 16 in fp32), each measured with the other as the
    yardstick, on every tile of O: the condition under which a correct kernel in either ordering passes
    the GPU file. dQ / dK / dV run through the same assertion but measure nothing here: the yardstick's
    backward reads the other result's O and lse, and from the same O and lse both orderings compute the
    same backward, so their ratio is 1.00 by construction (it checks the plumbing, not a spread)."""
    sc = 1.0 / math.sqrt(c.dqk)
    q, k, v, do = A.make_inputs(kind, c.B, c.Tq, c.Tk, c.H, c.Hkv, c.dqk, c.dv, sc, dt, "cpu")
    keep = dropout_keep_mask(G.SEED, c.B, c.H, c.Tq, c.Tk, c.p) if c.p > 0 else None
    ref = A.ref64(q, k, v, do, c.causal, sc, keep, c.p)
    if dt == torch.bfloat16:
        emu, blk = A.emulate_bf16, 32
        rm, mm = A.RMS_MARGIN, A.MAX_MARGIN
    else:
        emu, blk = A.emulate_fp32, 16
        rm, mm = A.F32_RMS_MARGIN, A.F32_MAX_MARGIN
    # each ordering as the "kernel", the other as its yardstick (whose backward reads the kernel's O and lse)
    m = emu(q, k, v, do, c.causal, sc, keep, c.p)
    b = emu(q, k, v, do, c.causal, sc, keep, c.p, order="blockwise", block=blk)
    ym = emu(q, k, v, do, c.causal, sc, keep, c.p, fwd=(b[0], b[1]))
    yb = emu(q, k, v, do, c.causal, sc, keep, c.p, order="blockwise", block=blk, fwd=(m[0], m[1]))
    pairs = [(b, ym, "blockwise vs materialised"), (m, yb, "materialised vs blockwise")]
    if dt == torch.bfloat16 and c.B * c.H * c.Tq * c.Tk < 10 ** 7:    # the forward kernels' own order (deferred rescale) against the materialised one: printed
        # only. It is a kernel-specific step (the GPU file's yardstick for the attention.hip kernels); one single-row
        # tile (Tq 1 x Tk 77, ramp_hi) sits at 2.22x of the materialised ordering here.
        d = emu(q, k, v, do, c.causal, sc, keep, c.p, order="blockwise", block=32, defer_log2=8.0)
        pairs.append((d, emu(q, k, v, do, c.causal, sc, keep, c.p, fwd=(d[0], d[1])), "deferred blockwise vs materialised"))
    floor = G.zero_ref_floor(c, q, k, v, do, sc)
    errs, line = [], []
    for i, name in NAMES:
        fl = floor if name in ("dQ", "dK") else 0.0
        for x, y, tag in pairs:
            wr, wm, _ = A.worst_ratios(x[i], ref[i], y[i], floor=fl)
            line.append(f"{name} {float(wr.max()):.2f}/{float(wm.max()):.2f}")
            if tag.startswith("deferred"):
                continue
            try:
                A.assert_tiles(x[i], ref[i], y[i], f"{name} {tag}", rm, mm, floor=fl)
            except AssertionError as e:
                errs.append(str(e))
    print(f"SPREAD {c.id} {kind}: " + "  ".join(line))
    # lse: both orderings of the fp32 emulation are the yardstick of the GPU file, so nothing to compare
    # here beyond both being close to fp64 at all
    assert float((m[1].double() - ref[1]).abs().max()) < 1e-3
    assert not errs, "\n".join(errs)


# ------------------------------------------------------------------ mutations
MB, MT, MH, MHKV, MHD = 8, 325, 16, 2, 32


@pytest.fixture(scope="module")
def mut():
    sc = 1.0 / math.sqrt(MHD)
    q, k, v, do = A.make_inputs("randn", MB, MT, MT, MH, MHKV, MHD, MHD, sc, torch.bfloat16, "cpu", seed=11)
    ref = A.ref64(q, k, v, do, True, sc)
    blk = A.emulate_bf16(q, k, v, do, True, sc, order="blockwise", block=32)
    # the yardstick the GPU file deploys for the attention.hip kernels
    yard = G.bf16_yardstick(q, k, v, do, True, sc, None, 0.0, (blk[0], blk[1]), "")
    return dict(q=q, k=k, v=v, do=do, sc=sc, ref=ref, yard=yard, blk=blk)


def _old_rel_ok(x, ref, i):
    return A.rel(x, ref[i]) < (2e-2 if i == 0 else 3e-2)


def _caught(x, mt, i, name):
    assert _old_rel_ok(x, mt["ref"], i), f"{name}: the mutation must pass the old rel bound ({A.rel(x, mt['ref'][i]):.2e})"
    with pytest.raises(AssertionError) as e:
        A.assert_tiles(x, mt["ref"][i], mt["yard"][i], name)
    return str(e.value)


def _lse_yards(mt):
    """The three lse yardsticks of the GPU file (its oracle())."""
    a = (mt["q"], mt["k"], mt["v"], mt["do"], True, mt["sc"])
    return [A.emulate_fp32(*a)[1], A.emulate_fp32(*a, order="blockwise", block=16)[1],
            A.lse_log2_fp32(mt["q"], mt["k"], True, mt["sc"])]


def test_unmutated_result_passes(mut):
    for i, name in NAMES:
        A.assert_tiles(mut["blk"][i], mut["ref"][i], mut["yard"][i], name)
    A.assert_lse(mut["blk"][1], mut["ref"][1], _lse_yards(mut), "lse")


def test_mutation_query_tile_scaled(mut):
    x = mut["blk"][0].clone()
    x[3, 64:96, 5] *= 1.02
    msg = _caught(x, mut, 0, "O")
    assert "b=3, head=5, first row=64" in msg, msg


def test_mutation_dk_tail_rows_scaled(mut):
    x = mut["blk"][3].clone()
    x[2, MT - 5:, 1] *= 0.9
    msg = _caught(x, mut, 3, "dK")
    assert "b=2, head=1, first row=320" in msg, msg


def test_mutation_dq_row_zeroed(mut):
    x = mut["blk"][2].clone()
    x[MB - 1, MT - 1, MH - 1] = 0
    msg = _caught(x, mut, 2, "dQ")
    assert f"b={MB - 1}, head={MH - 1}, first row=320" in msg, msg


def test_mutation_causal_mask_shifted_on_diagonal_tile(mut):
    """One (b, head): the queries of rows 288..319 see one key too many inside their diagonal tile."""
    i = torch.arange(MT)[:, None]
    j = torch.arange(MT)[None, :]
    vis = (j <= i).expand(MB, MH, MT, MT).clone()
    diag = (i >= 288) & (i < 320) & (j >= 288) & (j < 320)
    vis[4, 7] = (j <= i) | (diag & (j <= i + 1))
    x = A.emulate_bf16(mut["q"], mut["k"], mut["v"], mut["do"], True, mut["sc"], order="blockwise", block=32, vis=vis)
    msg = _caught(x[0], mut, 0, "O")
    assert "b=4, head=7, first row=288" in msg, msg
    for n, (idx, name) in enumerate(NAMES[1:]):
        _caught(x[idx], mut, idx, name)


def test_mutation_q_head_left_out_of_dk_dv(mut):
    """q-head 11 (of kv head 1's group of 8) contributes nothing to dK / dV of the key tile at rows 96..127."""
    b, h, g = 5, 11, 1
    part = A.emulate_bf16(mut["q"][b:b + 1, :, h:h + 1], mut["k"][b:b + 1, :, g:g + 1], mut["v"][b:b + 1, :, g:g + 1],
                          mut["do"][b:b + 1, :, h:h + 1], True, mut["sc"])
    for idx, name in ((3, "dK"), (4, "dV")):
        x = mut["blk"][idx].clone()
        x[b, 96:128, g] -= part[idx][0, 96:128, 0]
        msg = _caught(x, mut, idx, name)
        assert "b=5, head=1, first row=96" in msg, msg


def test_mutation_lse_row_off(mut):
    x = mut["blk"][1].clone()
    x[6, 9, 200] += 1e-2
    assert float((x.double() - mut["ref"][1]).abs().max()) < 5e-2      # the older tests' widest lse bound
    with pytest.raises(AssertionError, match=r"b=6, head=9, row=200"):
        A.assert_lse(x, mut["ref"][1], _lse_yards(mut), "lse")


# ------------------------------------------------------------------ CPU routes of the ops
def _f32_yards(q, k, v, do, causal, sc, keep=None, p=0.0):
    return (A.emulate_fp32(q, k, v, do, causal, sc, keep, p),
            A.emulate_fp32(q, k, v, do, causal, sc, keep, p, order="blockwise", block=16))


_ROUTE_SHAPES = [(True, 77, 77, 4, 2, 64, 0.0), (False, 45, 109, 2, 1, 32, 0.0), (True, 64, 109, 4, 4, 16, 0.3)]


@pytest.mark.parametrize("route,causal,Tq,Tk,H,Hkv,hd,p", [
    (r,) + sh for r in ("flash_attention", "_materialised", "no_grad") for sh in _ROUTE_SHAPES
    if not (r == "no_grad" and sh[-1] > 0)])     # dropout always takes _materialised: no such route without grad
def test_cpu_routes_meet_fp32_yardstick(route, causal, Tq, Tk, H, Hkv, hd, p):
    """flash_attention on the CPU (autograd through _materialised; reference.attention without grad) and
    _materialised itself, fp32 inputs, against ref64 with the fp32 yardstick."""
    sc = 1.0 / math.sqrt(hd)
    q, k, v, do = A.make_inputs("randn", 2, Tq, Tk, H, Hkv, hd, hd, sc, torch.float32, "cpu", seed=3)
    keep = dropout_keep_mask(77, 2, H, Tq, Tk, p) if p > 0 else None
    ref = A.ref64(q, k, v, do, causal, sc, keep, p)
    yards = _f32_yards(q, k, v, do, causal, sc, keep, p)
    if route == "no_grad":
        with torch.no_grad():
            o = flash_attention(q, k, v, causal, sc)
        A.assert_tiles(o, ref[0], [y[0] for y in yards], "O", A.F32_RMS_MARGIN, A.F32_MAX_MARGIN)
        return
    ql, kl, vl = (t.clone().requires_grad_() for t in (q, k, v))
    if route == "flash_attention":
        o = flash_attention(ql, kl, vl, causal, sc, dropout_p=p, seed=77)
    else:
        o = _materialised(ql, kl, vl, causal, sc, p, 77)
    o.backward(do)
    for (i, name), x in zip(NAMES, (o.detach(), ql.grad, kl.grad, vl.grad)):
        A.assert_tiles(x, ref[i], [y[i] for y in yards], name, A.F32_RMS_MARGIN, A.F32_MAX_MARGIN)


def test_mla_attention_cpu_path_meets_fp32_yardstick():
    """mla_attention's op-by-op CPU path: O, dV and the unrotated (nope) columns of dQ / dK against the
    oracle fed with the assembled heads."""
    from solvingpapers_amd.ops.rope import apply_rope
    B, T, H, dn, dr, dv, theta = 2, 77, 4, 32, 16, 32, 10000.0
    sc = 1.0 / math.sqrt(dn + dr)
    q, k, v, do = A.make_inputs("randn", B, T, T, H, H, dn + dr, dv, sc, torch.float32, "cpu", seed=5)
    kr = k[:, :, :1, dn:].contiguous()
    kv = torch.cat([k[..., :dn], v], dim=-1)
    q_, kv_, kr_ = (t.clone().requires_grad_() for t in (q, kv, kr))
    o = mla_attention(q_, kv_, kr_, dn, sc, theta)
    o.backward(do)
    with torch.no_grad():
        qf = torch.cat([q[..., :dn], apply_rope(q[..., dn:], theta, 0)], dim=-1)
        kf = torch.cat([k[..., :dn], apply_rope(kr, theta, 0).expand(B, T, H, dr)], dim=-1)
    ref = A.ref64(qf, kf, v, do, True, sc)
    yards = _f32_yards(qf, kf, v, do, True, sc)
    m = (A.F32_RMS_MARGIN, A.F32_MAX_MARGIN)
    A.assert_tiles(o.detach(), ref[0], [y[0] for y in yards], "O", *m)
    A.assert_tiles(kv_.grad[..., dn:], ref[4], [y[4] for y in yards], "dV", *m)
    A.assert_tiles(q_.grad[..., :dn], ref[2][..., :dn], [y[2][..., :dn] for y in yards], "dQ nope", *m)
    A.assert_tiles(kv_.grad[..., :dn], ref[3][..., :dn], [y[3][..., :dn] for y in yards], "dK nope", *m)
