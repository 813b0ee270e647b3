"""The streaming kernels on every dispatch path against the fp64 oracle with per-row bounds (tests/rowop_oracle.py):
each output's error per row (or per 64 columns, or per fp32 scalar) is bounded by a small multiple of what a plain
emulation of the kernel's roundings achieves on the same inputs. The case lists and the ``*_check`` functions are
shared with tests/test_rowop_oracle_cpu.py, which runs the emulations and the mutations through them.

Paths and the cases that reach them (csrc/kernels/):
  norm.hip  <64,1> D 8 / 512; <64,2> D 520 / 1024; <256,1> D 1032 / 2048; <256,2> D 2056 / 4096; <256,4> D 4104 /
            7168 / 8192; <256,8> D 8200 / 16384: NORM_CASES "D*" (RMS and LN, bf16 and fp32, residual on every other)
            second row sweep, one-wave path (M > 4096), three valid sub-rows in the tail: "sweep-D8/512/1024-M4099"
            second row sweep, block path (M > 1024): "sweep-D1032/8200/16384-M1027"
            invalid sub-rows in the only sweep: every M = 1, 3, 65 case at D <= 1024
            one- / two-level colsum (64 / 65 partial rows): M = 64 and M = 65 cases (block path: nparts = M; one-wave
            path: nparts = 64 / 68), two levels also in every sweep case
            dw_out / db_out direct writes: test_norm_direct_weight_grads; M = 0: test_norm_empty
            eps: "tiny-*" (rows at 2^-9, eps 1e-5 and 1e-6); offset and spike rows: "offset-*", "spike-*"
  xent.hip  smoothing 0.1, write_grad off, fp32 logits, the [:, :V] view of a 128-padded buffer: XENT_CASES fields
            rows shorter than a vector: V 5; rows under 2048 columns with the maximum in the scalar head / tail
            (idle threads hold m = -inf): "edges" at V 5 / 65 / 2047; every 16-byte phase of the row start: odd V, 16 rows
            chunk kernels at a second rank's v0, Vtot != Vc: test_xent_chunks
  rope.hip  modes 0 / 1 / 2 forward and inverse, bf16 / fp32, hd 16 / 64 / 128 / 256, pos tensor, pos_off, packed strided
            view with nrot < NH: ROPE_CASES; grid-stride loop (> 4096 x 256 vectors): "gridstride"
  activation.hip  glu_fwd / glu_bwd (bf16, fp32), glu_fwd_t / glu_bwd_t (bf16): GLU_CASES
  optim.hip adamw_kernel <float,float,false>, <bf16,float,true>, <bf16,bf16,true>, <bf16,bf16,true,bf16>, scalar tail
            (n 5, 10007), adam_l2, clip coefficient, NaN coefficient, device hyper: ADAMW_CASES, test_adamw_*

Infinite logits are outside what the cross-entropy kernels promise (a first vector of -inf makes exp(-inf + inf)):
not tested."""
import functools
from collections import namedtuple

import pytest
import torch

import rowop_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF, "fp32": F32}
WORST = {}          # (op, output) -> worst (rms ratio, maxabs ratio) seen in this process


def _ops():
    from solvingpapers_amd.ops import _ext
    assert _ext.load(), "HIP extension must load on the GPU box"
    return _ext.ops()


class Checks:
    """Collects every bound of one case, so a failure reports all outputs over their bound."""

    def __init__(self, op, cid):
        self.op, self.cid, self.errors = op, cid, []

    def _note(self, out, r):
        r = r if isinstance(r, tuple) else (r, r)
        w = WORST.get((self.op, out), (0.0, 0.0))
        WORST[(self.op, out)] = (max(w[0], r[0]), max(w[1], r[1]))

    def run(self, out, fn, *a, **k):
        try:
            self._note(out, fn(*a, **k))
        except AssertionError as e:
            self.errors.append(str(e))

    def units(self, out, x, ref, yards, dtype, cols=False, floor=0.0):
        rm, mm = O.margins(dtype)
        yards = yards if dtype == F32 else yards[:1]      # bf16: ONE emulation, the kernel-shaped order
        self.run(out, O.assert_units, x, ref, yards, f"{self.cid} {out}", rm, mm, cols, floor)

    def done(self):
        assert not self.errors, "\n".join(self.errors)


def _orders(dtype):
    return ("kernel", "seq") if dtype == F32 else ("kernel",)


def _cpu(t):
    return None if t is None else t.detach().cpu()


# =============================================================================================== norm
NormCase = namedtuple("NormCase", "id D M ln res dtype kind eps")
NORM_DS = (8, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 7168, 8192, 8200, 16384)
NORM_MS = (1, 3, 64, 65, 300)


def _norm_cases():
    cs = []
    for d, D in enumerate(NORM_DS):
        for j, (ln, dt) in enumerate(((False, "bf16"), (False, "fp32"), (True, "bf16"), (True, "fp32"))):
            M = NORM_MS[(j + 2 * d) % 5]
            cs.append(NormCase(f"D{D}-M{M}-{'ln' if ln else 'rms'}-{dt}", D, M, ln, (j + d) % 2 == 1, dt, "randn", 1e-5))
    for D in (8, 512, 1024):      # M > 4096: a second sweep of the one-wave path with three valid sub-rows
        cs.append(NormCase(f"sweep-D{D}-M4099-rms-bf16", D, 4099, False, D == 512, "bf16", "randn", 1e-5))
    cs.append(NormCase("sweep-D512-M4099-ln-fp32", 512, 4099, True, True, "fp32", "randn", 1e-5))
    for D, ln, dt in ((1032, True, "bf16"), (8200, True, "fp32"), (16384, False, "bf16")):   # M > 1024: block path
        cs.append(NormCase(f"sweep-D{D}-M1027-{'ln' if ln else 'rms'}-{dt}", D, 1027, ln, D == 1032, dt, "randn", 1e-5))
    for D, ln, dt, eps in ((512, False, "bf16", 1e-5), (512, False, "fp32", 1e-6), (4096, False, "bf16", 1e-6),
                           (4096, True, "bf16", 1e-5), (1032, True, "fp32", 1e-6)):
        cs.append(NormCase(f"tiny-D{D}-{'ln' if ln else 'rms'}-{dt}-eps{eps:g}", D, 65, ln, False, dt, "tiny", eps))
    for D, dt in ((1032, "bf16"), (4104, "fp32")):
        cs.append(NormCase(f"offset-D{D}-ln-{dt}", D, 65, True, D == 4104, dt, "offset", 1e-5))
    for D, ln, dt in ((520, False, "bf16"), (2056, True, "bf16"), (2056, False, "fp32")):
        cs.append(NormCase(f"spike-D{D}-{'ln' if ln else 'rms'}-{dt}", D, 65, ln, False, dt, "spike", 1e-5))
    return cs


NORM_CASES = _norm_cases()


@functools.lru_cache(maxsize=4)
def norm_refs(c, wgrad_dtype=None):
    """(inputs, fp64 reference, yardsticks) of a case; computed once and shared, never modified."""
    inp = O.make_inputs("norm", c.kind, DT[c.dtype], seed=len(c.id) + c.D + c.M, M=c.M, D=c.D, ln=c.ln, res=c.res)
    a = (inp["x"], inp["res"], inp["w"], inp["b"], c.eps, inp["dy"], inp["dres"])
    ref = O.norm_ref64(*a)
    orders = _orders(F32 if wgrad_dtype == F32 else DT[c.dtype])       # fp32 weight gradients of bf16 I/O: both
    yards = [O.norm_emulate(*a, order=o, wgrad_dtype=wgrad_dtype) for o in orders]
    return inp, ref, yards


def norm_check(out, c, wgrad_dtype=None, keys=("y", "h", "rstd", "mean", "dx", "dw", "db")):
    """out: dict of y, h, rstd, mean, dx, dw, db (CPU tensors) of case c against the oracle."""
    inp, ref, yards = norm_refs(c, wgrad_dtype)
    dt = DT[c.dtype]
    ck = Checks("norm", c.id)
    for k in keys:
        if (k == "h" and not c.res) or (k in ("mean", "db") and not c.ln):
            continue
        ys = [y[k] for y in yards]
        if k in ("rstd", "mean"):
            ck.run(k, O.assert_scalars, out[k], ref[k], ys, f"{c.id} {k}")
        elif k in ("dw", "db"):
            ck.units(k, out[k], ref[k], ys, wgrad_dtype or dt, cols=True)
        else:
            ck.units(k, out[k], ref[k], ys, dt)
    ck.done()


def norm_run(c):
    """The public ops (autograd) for y, h, dx, dw, db; the extension op itself for rstd / mean."""
    from solvingpapers_amd.ops import layer_norm, rms_norm
    inp, _, _ = norm_refs(c)
    g = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
    x, w = g["x"].clone().requires_grad_(), g["w"].clone().requires_grad_()
    r = g["res"].clone().requires_grad_() if c.res else None
    b = g["b"].clone().requires_grad_() if c.ln else None
    o = layer_norm(x, w, b, c.eps, residual=r) if c.ln else rms_norm(x, w, c.eps, residual=r)
    y, h = o if c.res else (o, None)
    torch.autograd.backward([y, h] if c.res else [y], [g["dy"], g["dres"]] if c.res else [g["dy"]])
    if c.res:
        assert torch.equal(r.grad, x.grad), "the residual's gradient is dx"
    _, _, rstd, mean = _ops().norm_fwd(g["x"], g["res"], g["w"], g["b"], c.eps)
    return dict(y=_cpu(y), h=_cpu(h), rstd=_cpu(rstd), mean=_cpu(mean) if c.ln else None, dx=_cpu(x.grad),
                dw=_cpu(w.grad), db=_cpu(b.grad) if c.ln else None)


@pytest.mark.parametrize("c", NORM_CASES, ids=[c.id for c in NORM_CASES])
def test_norm(c):
    norm_check(norm_run(c), c)


@pytest.mark.parametrize("dt,wdt", [("bf16", BF), ("fp32", F32), ("bf16", F32)])
def test_norm_direct_weight_grads(dt, wdt):
    """dw_out / db_out written straight into a main_grad view lying between sentinel rows of a larger buffer."""
    c = NormCase(f"direct-{dt}", 1032, 65, True, False, dt, "randn", 1e-5)
    inp, _, _ = norm_refs(c, wdt)
    g = {k: (None if v is None else v.to(DEV)) for k, v in inp.items()}
    y, _, rstd, mean = _ops().norm_fwd(g["x"], None, g["w"], g["b"], c.eps)
    buf = torch.full((4, c.D), 777.0, device=DEV, dtype=wdt)
    before = buf.clone()
    dx, dw, db = _ops().norm_bwd(g["dy"], g["x"], g["w"], rstd, mean, None, buf[1], buf[2])
    assert dw.data_ptr() == buf[1].data_ptr() and db.data_ptr() == buf[2].data_ptr()
    assert torch.equal(buf[0], before[0]) and torch.equal(buf[3], before[3]), "sentinel rows written"
    norm_check(dict(y=_cpu(y), rstd=_cpu(rstd), mean=_cpu(mean), dx=_cpu(dx), dw=_cpu(buf[1]), db=_cpu(buf[2])), c, wdt)


@pytest.mark.parametrize("ln", [False, True])
def test_norm_empty(ln):
    """M = 0 returns zero weight gradients (norm.hip:362)."""
    D = 520
    z = torch.empty(0, D, device=DEV, dtype=BF)
    w = torch.ones(D, device=DEV, dtype=BF)
    b = torch.ones(D, device=DEV, dtype=BF) if ln else None
    y, _, rstd, mean = _ops().norm_fwd(z, None, w, b, 1e-5)
    out = torch.full((2, D), 5.0, device=DEV, dtype=BF)
    dx, dw, db = _ops().norm_bwd(z, z, w, rstd, mean if ln else None, None, out[0], out[1] if ln else None)
    assert y.shape == (0, D) and dx.shape == (0, D) and rstd.numel() == 0
    assert bool((out[0] == 0).all()) and bool((out[1] == (0 if ln else 5)).all())


# =============================================================================================== cross-entropy
XentCase = namedtuple("XentCase", "id V dtype kind smoothing grad scale padded fast")
XENT_N = 16


def _xent_cases():
    cs = []

    def add(V, dt, kind, sm=0.0, grad=True, scale=None, padded=False, fast=True):
        # fast: xent.hip forms every exp / log through __expf / __logf (rowop_oracle fast_exp)
        cs.append(XentCase(f"V{V}-{dt}-{kind}-s{sm:g}{'' if grad else '-nograd'}{'-scale' if scale else ''}"
                           f"{'-padded' if padded else ''}", V, dt, kind, sm, grad, scale, padded, fast))
    for V in (5, 65, 2047, 2048, 2055, 50257):
        add(V, "bf16", "randn", 0.0, True, 1.0 / 15, padded=True)
        add(V, "fp32", "edges", 0.1)
        add(V, "bf16", "edges", 0.1, True, 1.0 / 15)
        add(V, "fp32", "randn", 0.0, padded=True)
    for V in (65, 2055, 50257):
        add(V, "bf16", "wide", 0.0, True, 0.25)
        add(V, "fp32", "wide", 0.1)
        add(V, "bf16", "randn", 0.1, grad=False)
        add(V, "fp32", "edges", 0.0, grad=False, padded=True)
    add(128256, "bf16", "randn", 0.0, True, 1.0 / 15)
    add(128256, "fp32", "edges", 0.1, padded=True)
    add(128256, "bf16", "wide", 0.1, True, 1.0 / 15, padded=True)
    return cs


XENT_CASES = _xent_cases()
PAD_VALUE = -3.0


def row_heads(N, ld, elt, col0=0):
    """Scalar head (elements before the first 16-byte boundary, xent.hip:36) of each row of a [N, V] view with row
    stride ld whose allocation is 16-byte aligned and whose first column is col0 of it."""
    byte = (torch.arange(N) * ld + col0) * elt
    return ((16 - byte % 16) % 16) // elt


@functools.lru_cache(maxsize=4)
def xent_refs(c):
    dt = DT[c.dtype]
    inp = O.make_inputs("xent", c.kind, dt, seed=c.V + len(c.id), N=XENT_N, V=c.V)
    sc = 1.0 if c.scale is None else float(torch.tensor(c.scale, dtype=F32))     # the fp32 value the kernel reads
    ref = O.xent_ref64(inp["logits"], inp["tgt"], -100, c.smoothing, sc)
    ld = (c.V // 128 + 1) * 128 if c.padded else c.V
    h0 = row_heads(XENT_N, ld, 2 if dt == BF else 4)
    yards = [O.xent_emulate(inp["logits"], inp["tgt"], -100, c.smoothing, sc, order=o, h0=h0, fast_exp=c.fast)
             for o in _orders(dt)]
    return inp, ref, yards


def xent_check(out, c, scalars=("loss", "lse")):
    """out: dict of loss, lse and (write_grad) grad."""
    inp, ref, yards = xent_refs(c)
    dt = DT[c.dtype]
    ck = Checks("xent", c.id)
    for k in scalars:
        ck.run(k, O.assert_scalars, out[k], ref[k], [y[k] for y in yards], f"{c.id} {k}")
    if c.grad:
        # the gradient pass reads the lse the statistics pass left (xent.hip:110, :124): one scalar per row whose
        # rounding error multiplies the whole row coherently. The kernel-shaped yardstick reads the lse of the result it
        # is compared with, as attn_oracle's backward reads the forward's; lse is bounded on its own above.
        tgt = inp["tgt"]
        sc = 1.0 if c.scale is None else float(torch.tensor(c.scale, dtype=F32))
        gy = O.xent_grad_emulate(inp["logits"].float(), tgt, out["lse"].float(), dt, -100, c.smoothing, sc,
                                 fast_exp=c.fast)
        parts = [O.split_target(t, tgt) for t in [out["grad"].double(), ref["grad"], gy] + [y["grad"] for y in yards[1:]]]
        (gk, tk, _), (gr, tr, _), ys = parts[0], parts[1], parts[2:]
        ck.units("grad", gk, gr, [y[0] for y in ys], dt)
        ck.run("grad target", O.assert_elements, tk, tr, [y[1] for y in (ys if dt == F32 else ys[:1])],
               f"{c.id} grad target column", dt)
    ck.done()


def xent_run(c):
    inp, _, _ = xent_refs(c)
    N, V = XENT_N, c.V
    lg = inp["logits"].to(DEV)
    if c.padded:   # the way ops/xent.py _LinearXentFn calls it: a [:, :V] view of a buffer padded to 128 columns
        buf = torch.full((N, (V // 128 + 1) * 128), PAD_VALUE, device=DEV, dtype=lg.dtype)
        buf[:, :V] = lg
        view = buf[:, :V]
    else:
        buf = view = lg.clone()
    scale = None if c.scale is None else torch.tensor([c.scale], device=DEV, dtype=F32)
    loss, lse = _ops().xent_fwd(view, inp["tgt"].to(DEV), -100, c.smoothing, c.grad, scale)
    if c.padded:
        assert bool((buf[:, V:] == PAD_VALUE).all()), "padding columns written"
    if not c.grad:
        assert torch.equal(view, lg), "write_grad = false must leave the logits alone"
    return dict(loss=_cpu(loss), lse=_cpu(lse), grad=_cpu(view).clone())


@pytest.mark.parametrize("c", XENT_CASES, ids=[c.id for c in XENT_CASES])
def test_xent(c):
    xent_check(xent_run(c), c)


CHUNK_VL, CHUNK_WIDTHS = 1361, (256, 1105)      # the widths of V = 50257's last chunks at 1024-column chunks: 256-
                                                # aligned body and the 1105-column remainder
ChunkCase = namedtuple("ChunkCase", "id dtype smoothing")
CHUNK_CASES = [ChunkCase("chunks-bf16", "bf16", 0.1), ChunkCase("chunks-fp32", "fp32", 0.1)]


@functools.lru_cache(maxsize=2)
def chunk_refs(c):
    """A second tensor-parallel rank's shard: local columns [0, Vl) are global [Vl, 2 Vl); targets on rank 0 (never
    seen here), on this rank (both chunks) and ignored. Per chunk: exact (m, s, t, x) running values in fp64 and the
    emulations' in fp32; then the gradient of each chunk from the fp32 lse the kernel is handed."""
    dt = DT[c.dtype]
    N, Vl = XENT_N, CHUNK_VL
    gen = torch.Generator().manual_seed(77)
    x = (torch.randn(N, Vl, generator=gen) * 2.0).to(dt)
    tgt = torch.randint(0, Vl, (N,), generator=gen)
    tgt[6:13] += Vl
    tgt[6], tgt[7], tgt[8] = Vl + 3, Vl + 255, Vl + 256          # chunk edges
    tgt[12] = 2 * Vl - 1
    tgt[13:] = -100
    steps, run64 = [], None
    runs = {o: None for o in _orders(dt)}
    init = lambda d: (torch.full((N,), float("-inf"), dtype=d), torch.zeros(N, dtype=d), torch.zeros(N, dtype=d),
                      torch.zeros(N, dtype=d))
    run64 = init(torch.float64)
    runs = {o: init(F32) for o in runs}
    c0 = 0
    for wdt in CHUNK_WIDTHS:
        xc = x[:, c0:c0 + wdt]
        v0 = Vl + c0
        loc = tgt - v0
        inside = (loc >= 0) & (loc < wdt)
        xt = xc.float().gather(1, torch.where(inside, loc, torch.zeros_like(loc))[:, None]).squeeze(1)
        x64 = xc.double()
        m64 = x64.amax(-1)
        run64 = O.chunk_fold_emulate(run64, m64, torch.exp(x64 - m64[:, None]).sum(-1), x64.sum(-1), (inside, xt),
                                     dt=torch.float64)
        h0 = row_heads(N, Vl, 2 if dt == BF else 4, c0)
        for o in runs:
            runs[o] = O.chunk_fold_emulate(runs[o], *O.xent_stats_emulate(xc.float(), o, h0), (inside, xt))
        steps.append((c0, wdt, v0, run64, dict(runs)))
        c0 += wdt
    lse = (run64[0] + torch.log(run64[1])).float()
    scale = float(torch.tensor(1.0 / 13, dtype=F32))
    grads = []
    for c0, wdt, v0, _, _ in steps:
        xc = x[:, c0:c0 + wdt]
        ref = O.xent_ref64(xc, tgt, -100, c.smoothing, scale, v0=v0, Vtot=2 * Vl)
        g64 = (torch.exp(xc.double() - lse.double()[:, None]) - torch.exp(xc.double() - ref["lse"][:, None])) * \
            ((tgt != -100).double() * scale)[:, None] + ref["grad"]           # softmax from the given lse
        ge = O.xent_grad_emulate(xc.float(), tgt, lse, dt, -100, c.smoothing, scale, v0, 2 * Vl)
        grads.append((g64, ge))
    return x, tgt, steps, lse, scale, grads


def chunk_check(out_runs, out_grads, c):
    x, tgt, steps, lse, scale, grads = chunk_refs(c)
    dt = DT[c.dtype]
    ck = Checks("xent_chunk", c.id)
    for (c0, wdt, v0, r64, runs), got in zip(steps, out_runs):
        for i, k in enumerate("mstx"):
            ck.run(f"run_{k}", O.assert_scalars, got[i], r64[i], [r[i] for r in runs.values()],
                   f"{c.id} run_{k} after chunk at {c0}")
    for (c0, wdt, v0, _, _), (g64, ge), got in zip(steps, grads, out_grads):
        (gk, tk, _), (gr, tr, _), (gy, ty, _) = (O.split_target(t, tgt, v0) for t in (got.double(), g64, ge))
        ck.units("grad", gk, gr, [gy], dt)
        ck.run("grad target", O.assert_elements, tk, tr, [ty], f"{c.id} grad target column, chunk at {c0}", dt)
    ck.done()


@pytest.mark.parametrize("c", CHUNK_CASES, ids=[c.id for c in CHUNK_CASES])
def test_xent_chunks(c):
    x, tgt, steps, lse, scale, _ = chunk_refs(c)
    N = XENT_N
    buf = x.to(DEV).clone()
    t = tgt.to(DEV)
    m = torch.full((N,), float("-inf"), device=DEV)
    s, tl, sx = (torch.zeros(N, device=DEV) for _ in range(3))
    out_runs = []
    for c0, wdt, v0, _, _ in steps:
        _ops().xent_chunk_stats(buf[:, c0:c0 + wdt], t, v0, m, s, tl, sx)
        out_runs.append(tuple(_cpu(r).clone() for r in (m, s, tl, sx)))
    assert torch.equal(buf.cpu(), x), "xent_chunk_stats must not write the logits"
    out_grads = []
    sc = torch.tensor([1.0 / 13], device=DEV, dtype=F32)
    for c0, wdt, v0, _, _ in steps:
        _ops().xent_chunk_grad_(buf[:, c0:c0 + wdt], t, v0, lse.to(DEV), sc, -100, c.smoothing, 2 * CHUNK_VL)
        out_grads.append(_cpu(buf[:, c0:c0 + wdt]).clone())
    chunk_check(out_runs, out_grads, c)


# =============================================================================================== rope
RopeCase = namedtuple("RopeCase", "id mode dtype hd B T H Hkv pos theta")
ROPE_TMAX = 40


def _rope_cases():
    cs = []
    i = 0
    for mode in (0, 1, 2):
        for dt in ("bf16", "fp32"):
            for hd in (16, 64, 128, 256):
                pos = ("off0", "off27", "tensor")[i % 3]
                cs.append(RopeCase(f"m{mode}-{dt}-hd{hd}-{pos}", mode, dt, hd, 2, 13, 3, 1 + i % 2, pos, 100.0))
                i += 1
    # more than 4096 x 256 vectors: the grid-stride loop takes a second turn (rope.hip:33, :103)
    cs.append(RopeCase("gridstride-m1-bf16", 1, "bf16", 128, 4, 1100, 15, 1, "off0", 100.0))
    return cs


ROPE_CASES = _rope_cases()


@functools.lru_cache(maxsize=2)
def rope_refs(c):
    """x is the packed [B, T, H + 2 Hkv, hd] view's content; heads [0, H + Hkv) are rotated. Returns (x, cos, sin, pos,
    nrot, ref forward, ref inverse (of a second tensor dy), yardsticks)."""
    from solvingpapers_amd.ops import reference as R
    dt = DT[c.dtype]
    NH, nrot = c.H + 2 * c.Hkv, c.H + c.Hkv
    Tmax = max(ROPE_TMAX, c.T)
    cos, sin = R.rope_tables(Tmax, c.hd, c.theta)
    if c.pos == "tensor":      # unsorted, up to the table's last row
        gen = torch.Generator().manual_seed(5)
        pos = torch.randint(0, Tmax, (c.B, c.T), generator=gen)
        pos[0, 0], pos[-1, -1] = Tmax - 1, 0
    else:
        off = int(c.pos[3:])
        pos = (torch.arange(c.T) + off)[None, :].expand(c.B, c.T).contiguous()
    # every pair turns by more than 0.1 rad somewhere in the case
    assert bool((sin[pos.reshape(-1)].abs().amax(0) > math_sin_01).all()), "a pair never rotates visibly"
    x = O.make_inputs("rope", "randn", dt, seed=c.hd + c.mode, B=c.B, T=c.T, NH=NH, hd=c.hd)["x"]
    dy = O.make_inputs("rope", "randn", dt, seed=c.hd + c.mode + 100, B=c.B, T=c.T, NH=NH, hd=c.hd)["x"]
    ref = {inv: O.rope_ref64((dy if inv else x)[:, :, :nrot], cos, sin, pos, c.mode, inv) for inv in (False, True)}
    yards = {inv: [O.rope_emulate((dy if inv else x)[:, :, :nrot], cos, sin, pos, c.mode, inv, order=o)
                   for o in _orders(dt)] for inv in (False, True)}
    return x, dy, cos, sin, pos, nrot, ref, yards


math_sin_01 = 0.09983341664682815     # sin(0.1)


def rope_check(out, c):
    """out: {False: rotated heads of x, True: inverse-mapped heads of dy}, [B, T, nrot, hd]."""
    x, dy, cos, sin, pos, nrot, ref, yards = rope_refs(c)
    ck = Checks("rope", c.id)
    for inv in (False, True):
        ck.units("inverse" if inv else "forward", out[inv], ref[inv], yards[inv], DT[c.dtype])
    ck.done()


def rope_run(c):
    x, dy, cos, sin, pos, nrot, _, _ = rope_refs(c)
    B, T, NH, hd = x.shape
    out = {}
    for inv, src in ((False, x), (True, dy)):
        # the packed view sliced out of a wider buffer: one spare head slot before and after every token's heads
        wide = torch.full((B, T, NH + 2, hd), 9.0, device=DEV, dtype=src.dtype)
        wide[:, :, 1:1 + NH] = src.to(DEV)
        before = wide.clone()
        view = wide[:, :, 1:1 + NH]
        if c.pos == "tensor":
            _ops().rope_(view, cos.to(DEV), sin.to(DEV), pos.to(DEV).int().contiguous(), nrot, 0, c.mode, inv)
        else:
            _ops().rope_(view, cos.to(DEV), sin.to(DEV), None, nrot, int(c.pos[3:]), c.mode, inv)
        assert torch.equal(wide[:, :, 1 + nrot:], before[:, :, 1 + nrot:]), "heads >= nrot or the bytes after changed"
        assert torch.equal(wide[:, :, :1], before[:, :, :1]), "bytes before the view changed"
        out[inv] = _cpu(view[:, :, :nrot]).clone()
    return out


@pytest.mark.parametrize("c", ROPE_CASES, ids=[c.id for c in ROPE_CASES])
def test_rope(c):
    rope_check(rope_run(c), c)


# =============================================================================================== GLU
GluCase = namedtuple("GluCase", "id kind dtype M F inputs fast")
GLU_CASES = [GluCase(f"{k}-{dt}-{M}x{Fd}-{inp}", k, dt, M, Fd, inp, k == "silu")      # act_common.h SILU: __expf
             for k in ("silu", "gelu_tanh", "gelu") for dt in ("bf16", "fp32")
             for M, Fd in ((8, 8), (72, 136), (1000, 200)) for inp in ("grid", "randn")]


@functools.lru_cache(maxsize=2)
def glu_refs(c):
    dt = DT[c.dtype]
    inp = O.make_inputs("glu", c.inputs, dt, seed=c.M + c.F, M=c.M, F=c.F)
    ref = O.glu_ref64(inp["gu"], inp["dy"], c.kind)
    yards = [O.glu_emulate(inp["gu"], inp["dy"], c.kind, order=o, fast_exp=c.fast) for o in _orders(dt)]
    return inp, ref, yards


def glu_check(out, c):
    """out: y, dgu and (bf16) the transposed yt [F, M], dgut [2F, M], checked as columns."""
    inp, ref, yards = glu_refs(c)
    dt = DT[c.dtype]
    ck = Checks("glu", c.id)
    Fd = c.F
    ck.units("y", out["y"], ref["y"], [y["y"] for y in yards], dt)
    for nm, sl in (("dg", slice(0, Fd)), ("du", slice(Fd, 2 * Fd))):
        ck.units(nm, out["dgu"][:, sl], ref["dgu"][:, sl], [y["dgu"][:, sl] for y in yards], dt)
    if "yt" in out:
        ck.units("y (fwd_t)", out["y2"], ref["y"], [y["y"] for y in yards], dt)
        for nm, sl in (("dg (bwd_t)", slice(0, Fd)), ("du (bwd_t)", slice(Fd, 2 * Fd))):
            ck.units(nm, out["dgu2"][:, sl], ref["dgu"][:, sl], [y["dgu"][:, sl] for y in yards], dt)
        ck.units("y^T", out["yt"].t(), ref["y"], [y["y"] for y in yards], dt, cols=True)
        for nm, sl in (("dg^T", slice(0, Fd)), ("du^T", slice(Fd, 2 * Fd))):
            ck.units(nm, out["dgut"][sl].t(), ref["dgu"][:, sl], [y["dgu"][:, sl] for y in yards], dt, cols=True)
    ck.done()


def glu_run(c):
    inp, _, _ = glu_refs(c)
    gu, dy = inp["gu"].to(DEV), inp["dy"].to(DEV)
    kind = O.GLU_KINDS[c.kind]
    out = dict(y=_cpu(_ops().glu_fwd(gu, kind)), dgu=_cpu(_ops().glu_bwd(dy, gu, kind)))
    if c.dtype == "bf16":
        y2, yt = _ops().glu_fwd_t(gu, kind)
        d2, dt_ = _ops().glu_bwd_t(dy, gu, kind)
        assert torch.equal(yt.t(), y2) and torch.equal(dt_.t(), d2), "the transposed output is not the row-major one"
        out.update(y2=_cpu(y2), dgu2=_cpu(d2), yt=_cpu(yt), dgut=_cpu(dt_))
    return out


@pytest.mark.parametrize("c", GLU_CASES, ids=[c.id for c in GLU_CASES])
def test_glu(c):
    glu_check(glu_run(c), c)


# =============================================================================================== AdamW
AdamCase = namedtuple("AdamCase", "id inst n variant")
ADAM_INST = {   # p dtype, master, g dtype, moment dtype
    "fp32": (F32, False, F32, F32), "bf16-master": (BF, True, F32, F32), "bf16-grad": (BF, True, BF, F32),
    "bf16-moments": (BF, True, BF, BF)}
ADAMW_CASES = [AdamCase(f"{i}-n{n}-{v}", i, n, v) for i in ADAM_INST for n in (5, 10007) for v in ("plain", "l2", "clip")]
ADAM_HP = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)
CLIP = 0.37


def adam_state(c, dev, seed=0):
    pdt, master, gdt, mdt = ADAM_INST[c.inst]
    inp = O.make_inputs("adamw", "randn", F32, seed=c.n + seed, n=c.n)
    p0 = inp["p"]
    st = dict(p=p0.to(pdt).to(dev), master=p0.clone().to(dev) if master else None,
              m=torch.zeros(c.n, dtype=mdt, device=dev), v=torch.zeros(c.n, dtype=mdt, device=dev))
    return st, [g.to(gdt).to(dev) for g in inp["grads"]]


def adam_step_check(ck, c, before, after, g, step, hp, coef, l2, tag="", ref_step=None):
    """One step: the update src_after - src_before per element against adamw_ref64 from the state the kernel received;
    yardstick: the emulations' update error, floor half an ulp of the stored dtype at |src|. m and v likewise."""
    src_k = "master" if before["master"] is not None else "p"
    a = (before[src_k], g, before["m"], before["v"], hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"],
         step if ref_step is None else ref_step, coef, l2)
    r = O.adamw_ref64(*a)
    ys = [O.adamw_emulate(*a, order=o) for o in ("kernel", "seq")]
    s0 = before[src_k].double()
    sdt = before[src_k].dtype
    # the floor: storing the new value costs half an ulp at its magnitude (the larger of before and after, so an
    # update that carries a small parameter across a binade is held to the coarser of the two grids)
    ck.run("update", O.assert_elements, after[src_k].double() - s0, r[0] - s0, [y[0].double() - s0 for y in ys],
           f"{c.id}{tag} step {step} update", sdt, at=torch.maximum(s0.abs(), r[0].abs()))
    mdt = before["m"].dtype
    for i, k in ((1, "m"), (2, "v")):
        ck.run(k, O.assert_elements, after[k], r[i], [y[i] for y in (ys if mdt == F32 else ys[:1])],
               f"{c.id}{tag} step {step} {k}", mdt)
    if src_k == "master":
        assert torch.equal(after["p"], after["master"].to(after["p"].dtype)), "p is the rounded master"


def adam_kernel(st, g, step, hp, coef, l2, hyper=None):
    from solvingpapers_amd.ops import optim_kernels as K
    K.adamw_(st["p"], st["master"], g, st["m"], st["v"], hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step,
             coef, l2, hyper)


def _snap(st):
    return {k: (None if v is None else v.detach().cpu().clone()) for k, v in st.items()}


@pytest.mark.parametrize("c", ADAMW_CASES, ids=[c.id for c in ADAMW_CASES])
def test_adamw(c):
    """Three steps; each step's update, m and v per element from the state the kernel received."""
    st, grads = adam_state(c, DEV)
    coef = torch.tensor([CLIP], device=DEV) if c.variant == "clip" else None
    cf = float(torch.tensor(CLIP, dtype=F32)) if c.variant == "clip" else 1.0
    ck = Checks("adamw", c.id)
    for step, g in enumerate(grads, 1):
        before = _snap(st)
        adam_kernel(st, g, step, ADAM_HP, coef, c.variant == "l2")
        adam_step_check(ck, c, before, _snap(st), g.cpu(), step, ADAM_HP, cf, c.variant == "l2")
    ck.done()


@pytest.mark.parametrize("inst", list(ADAM_INST))
def test_adamw_nan_coef_skips(inst):
    """A NaN clip coefficient leaves p, master, m and v bitwise unchanged (optim.hip:33)."""
    c = AdamCase(f"{inst}-nan", inst, 10007, "clip")
    st, grads = adam_state(c, DEV)
    adam_kernel(st, grads[0], 1, ADAM_HP, None, False)
    before = _snap(st)
    adam_kernel(st, grads[1], 2, ADAM_HP, torch.tensor([float("nan")], device=DEV), False)
    after = _snap(st)
    for k, v in before.items():
        assert v is None or torch.equal(v.view(torch.int16 if v.dtype == BF else torch.int32),
                                        after[k].view(torch.int16 if v.dtype == BF else torch.int32)), k


HYPER_HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)


def hyper_state(c, dev):
    """A mid-training state: moments of a stationary gradient stream, so every step number is plausible."""
    st, grads = adam_state(c, "cpu", seed=3)
    mdt = st["m"].dtype
    st["m"] = (grads[1].float() * 0.3).to(mdt)
    st["v"] = (grads[2].float().square() * 0.5 + 0.1).to(mdt)
    return {k: (None if v is None else v.to(dev)) for k, v in st.items()}, grads[0].to(dev)


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("inst", ["fp32", "bf16-moments"])
def test_adamw_device_hyper(inst, step):
    """lr and the step read on the device (bias corrections formed in the kernel), bounded through the same oracle as
    the host-scalar path; the host arguments are deliberately wrong."""
    c = AdamCase(f"{inst}-hyper", inst, 10007, "plain")
    st, g = hyper_state(c, DEV)
    before = _snap(st)
    hyper = torch.tensor([HYPER_HP["lr"], float(step)], device=DEV, dtype=F32)
    adam_kernel(st, g, 77, dict(HYPER_HP, lr=0.5), None, False, hyper)
    ck = Checks("adamw_hyper", c.id)
    adam_step_check(ck, c, before, _snap(st), g.cpu(), step, HYPER_HP, 1.0, False, tag=" hyper")
    ck.done()
