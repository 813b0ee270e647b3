"""Per-row error bounds for the streaming kernels against an fp64 oracle (pure torch, any device).

Operations: RMSNorm / LayerNorm (csrc/kernels/norm.hip), softmax cross-entropy and its vocab-chunked form
(xent.hip), rotary embedding (rope.hip ``rope_``), the gated linear units (activation.hip) and AdamW (optim.hip).
For each there is ``*_ref64`` (every output and gradient from explicit formulas in fp64, inputs taken at the values
the kernel receives), ``*_emulate`` (the same operation with only the roundings a kernel of that I/O type must
make: inputs as given, fp32 arithmetic, one rounding to the output dtype) and the measures below. A kernel's error
per unit is bounded by a small multiple of the emulation's error on the same inputs: a self-calibrating bound
with no fixed constants, in the shape of tests/attn_oracle.py.

Units. Row-shaped outputs (y, h, dx, GLU outputs, rotated heads, the logit gradient): one row; rows under 64
elements are grouped into consecutive rows totalling at least 64 (``row_errors``). Column-shaped outputs (dw, db, the
transposed GLU outputs): 64 consecutive columns, colsum_kernel's block (``col_errors``). Per-row fp32 scalars (rstd,
mean, lse, per-row loss, the chunk kernels' running m, s, t, x): absolute error per row, the yardstick never below
|ref| * 2^-24, which is at least half an fp32 ulp of the reference (``assert_scalars``). The target column of a
cross-entropy gradient row is measured on its own (``assert_elements``, the floor half an ulp of the stored dtype),
the remaining columns as the row: otherwise the one-hot entry's rounding is the whole RMS.

Emulation orders. Each reduction comes in two legitimate orders: "seq", plain sequential, and "kernel", the order
the source shows: norm.hip: 8 elements per thread and vector, vectors strided by NT, the xor-butterfly of
wave_sum, the waves' partials added in order (spa_common.h block_sum); dw / db: one partial row per (block, sub-row)
over rows p, p + nparts, .., then colsum_partial_kernel / colsum_kernel (4 row slices, s0 + s1 + s2 + s3).
xent.hip row_stats: online (max, sum-exp) per thread over vectors strided by 256 after a scalar head that
reaches 16-byte alignment, scalar head and tail folded in after, wave butterfly, 4 waves in order. Elementwise
operations (rope_, GLU, AdamW) have no reduction; their two orders are two algebraically equal fp32 forms
("kernel": the expression of the source with the fused multiply-adds hipcc contracts it into -- read from the
assembly for AdamW: m = fma(b1, m, (1 - b1) g), v = fma(b2, v, ((1 - b2) g) g), denom = fma(sqrt v, 1 / sqrt bc2, eps),
1 - lr wd = fma(-lr, wd, 1); "seq": the form of ops/reference.py, operation for operation).

The cross-entropy gradient's kernel-shaped yardstick reads the lse of the result it is compared with (the kernel's
gradient pass reads the lse its statistics pass left): that one scalar per row multiplies the whole row coherently, and
with independent lse roundings a row's error ratio is the ratio of two random numbers (measured 10 x on an fp32 row of
2047 columns whose emulations both happened to round lse exactly). lse is bounded on its own.

Margins in force (kernel unit error <= margin x yardstick unit error on the same inputs):

    bf16 I/O:  RMS 1.502, max-abs 4.0 yardstick: ONE emulation, the kernel-shaped order
    fp32 I/O:  RMS 4.0, max-abs 4.0   yardstick: per unit, the larger of the two orders
    scalars:   4.0                    yardstick: the larger of the two orders and |ref| * 2^-24
    single stored elements (xent target column, AdamW updates): 4.0, floor half an ulp of the stored dtype

Observed spread between the two orders (tests/test_rowop_oracle_cpu.py measures it over every case and input kind of
tests/test_rowops_gpu.py, prints it and holds it to ``SPREADS`` below; worst per-unit ratio, either order as the
yardstick of the other):

    op      bf16 RMS   bf16 max-abs   fp32 RMS   fp32 max-abs
    norm    1.0004     1.002          497        733     (y, dx rows; dw, db columns)
    xent    1.0010     1.000          607        693     (logit gradient rows, target column apart)
    rope    1.0000     1.000          1.97       3.85
    glu     1.0000     1.000          4.20       7.14
    adamw   --         --             1.05       1.11    (whole-vector RMS / max of the update)

    -> bf16 RMS margin 1.5 x 1.001 = 1.502 (the project's rule in attn_oracle.py: 1.5 x the worst spread), below the
       2.0 the CPU file asserts; bf16 truncation measures 1.58 - 2.65 x the yardstick per row and fails it.
    -> fp32: the two orders are NOT within 4.0 of each other. A plain sequential fp32 sum over a row carries an error
       that grows with the row's length (random walk of D roundings at the magnitude of the running sum), the
       kernels' trees do not: 9 x at D 512, 36 x at D 16384, 343 x on "offset" rows (mean 30 x std: the running
       sum is 900 x the variance it is meant to resolve), 497 x on "spike" rows, 609 x on the coherent lse error of a
       50257-column row. The fp32 yardstick is, per unit, the larger of the two, so on long rows it is the sequential
       order's error that bounds an fp32 kernel, and the bf16 cases of the same shapes carry the sharp bound.
       The GLU spread is the cancellation in 1 + erf / 1 + tanh at negative gates, formed differently by the two forms.

A unit whose yardstick error is exactly zero (an ignored cross-entropy row, a reference that is exactly
representable) must match exactly, or within the ``floor`` the caller derives and passes in. No unit is left out of
a bound.

Kernel-specific steps (off unless asked for; never part of a margin):
    fast_exp   xent.hip row_stats / row_grad (:30-31, :48-49, :58, :68, :77, :86) and act_common.h SILU (:23, :48)
               evaluate exp through __expf = exp2(fl(x * log2 e)), and xent.hip:110 log through __logf =
               log2(x) * ln 2. The product x * log2 e is rounded before the exponential, which at |x| ~ 80
               ("wide" logits) is a relative error of up to 80 * 1.44 * 2^-24 = 7e-6 in the term.
    fma        hipcc contracts a * b + c into one fused operation (rope.hip:55-56, :78-79); the rope emulation's
               "kernel" order is the contracted form, "seq" the three-rounding form.

Infinite logits are outside what the cross-entropy kernels promise (a first vector of -inf makes exp(-inf + inf))
and are not tested.
"""
import math

import torch
import torch.nn.functional as F

RMS_MARGIN, MAX_MARGIN = 1.502, 4.0        # bf16 I/O (1.5 x the observed spread of 1.001)
F32_RMS_MARGIN, F32_MAX_MARGIN = 4.0, 4.0  # fp32 I/O
SCALAR_MARGIN = 4.0
UNIT = 64
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

# worst spread between the two emulation orders per operation: (bf16 RMS, bf16 max-abs, fp32 RMS, fp32 max-abs),
# measured by tests/test_rowop_oracle_cpu.py test_*_emulations, which fail when a measurement exceeds its entry
SPREADS = {
    "norm": (1.001, 1.003, 497.0, 733.0),
    "xent": (1.001, 1.000, 607.0, 693.0),
    "rope": (1.000, 1.000, 1.97, 3.85),
    "glu": (1.000, 1.000, 4.20, 7.14),
    "adamw": (0.0, 0.0, 1.05, 1.11),
}


def margins(dtype):
    return (RMS_MARGIN, MAX_MARGIN) if dtype == torch.bfloat16 else (F32_RMS_MARGIN, F32_MAX_MARGIN)


def _cdiv(a, b):
    return (a + b - 1) // b


def _rd(dtype):
    """Rounding to the I/O dtype, result held in fp32."""
    return lambda t: t.to(dtype).to(torch.float32)


def rel(a, b):
    """The whole-tensor measure of the older tests (tests/test_kernels_gpu.py)."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


# ------------------------------------------------------------------ reductions in the two orders
def seq_sum(x, dim=-1):
    """Plain sequential sum along ``dim`` in the tensor's dtype (every partial sum rounded)."""
    x = x.movedim(dim, 0).contiguous()
    acc = torch.zeros_like(x[0])
    for j in range(x.shape[0]):
        acc = acc + x[j]
    return acc


def _wave_tree(v):
    """spa_common.h wave_sum: xor butterfly over 64 lanes (32, 16, .., 1). [.., 64] -> [..]."""
    o = 32
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o //= 2
    return v[..., 0]


def norm_dispatch(D):
    """(NT, MAXV) of norm.hip NORM_FWD_DISPATCH / NORM_BWD_DISPATCH (:309-314, :371-376)."""
    nv = D // 8
    for lim, cfg in ((64, (64, 1)), (128, (64, 2)), (256, (256, 1)), (512, (256, 2)), (1024, (256, 4))):
        if nv <= lim:
            return cfg
    return (256, 8)


def kernel_row_sum(t, NT, MAXV):
    """Row sums of t [M, D] in the order of norm_fwd_kernel / norm_bwd_kernel: thread j adds its vectors
    j, j + NT, .. element by element (:34-52), wave_sum, then the waves in order (block_sum)."""
    M, D = t.shape
    tp = F.pad(t, (0, NT * MAXV * 8 - D)).view(M, MAXV, NT, 8)
    acc = torch.zeros(M, NT, dtype=t.dtype, device=t.device)
    for k in range(MAXV):
        for i in range(8):
            acc = acc + tp[:, k, :, i]
    w = _wave_tree(acc.view(M, NT // 64, 64))
    s = w[:, 0]
    for i in range(1, NT // 64):
        s = s + w[:, i]
    return s


def _colsum4(p):
    """colsum_kernel / colsum_partial_kernel (:192-221): row slices rs, rs + 4, .. then s0 + s1 + s2 + s3."""
    P, D = p.shape
    if P == 0:
        return torch.zeros(D, dtype=p.dtype, device=p.device)
    p = F.pad(p, (0, 0, 0, _cdiv(P, 4) * 4 - P)).view(-1, 4, D)
    a = seq_sum(p, 0)
    return ((a[0] + a[1]) + a[2]) + a[3]


def kernel_col_sum(t, RPB):
    """Column sums of t [M, D] as norm_bwd_kernel + colsum form them: partial row p = block * RPB + sub adds
    rows p, p + nparts, .. (:114), then one or (more than 64 partial rows, :383) two levels of _colsum4."""
    M, D = t.shape
    nparts = min(_cdiv(M, RPB), 1024) * RPB
    nsw = _cdiv(M, nparts)
    part = seq_sum(F.pad(t, (0, 0, 0, nsw * nparts - M)).view(nsw, nparts, D), 0)
    P = nparts
    if P > 64:
        Y = min(64, _cdiv(P, 16))
        chunk = _cdiv(P, Y)
        part = torch.stack([_colsum4(part[y * chunk:min(P, (y + 1) * chunk)]) for y in range(Y)])
    return _colsum4(part)


# ------------------------------------------------------------------ norm
def norm_ref64(x, res, w, b, eps, dy, dres=None):
    """fp64 RMSNorm (b None) / LayerNorm with the optional fused residual: h = x + res rounded to the I/O dtype
    once, the rounded value normalised (norm.hip:44). Returns a dict of y, h, rstd, mean, dx, dw, db (fp64)."""
    dt = x.dtype
    h = x.double() if res is None else (x.double() + res.double()).to(dt).double()
    # the kernel adds in fp32: for bf16 inputs the fp32 sum is exact before the single rounding; for fp32 inputs
    # the fp32 sum IS the stored h (one rounding either way)
    wd, dyd = w.double(), dy.double()
    D = h.shape[-1]
    mean = h.mean(-1, keepdim=True) if b is not None else torch.zeros_like(h[:, :1])
    var = ((h - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (h - mean) * rstd
    y = xh * wd + (b.double() if b is not None else 0.0)
    g = dyd * wd
    a1 = (g * xh).sum(-1, keepdim=True) / D
    a2 = g.sum(-1, keepdim=True) / D if b is not None else 0.0
    dx = rstd * (g - a2 - xh * a1)
    if dres is not None:
        dx = dx + dres.double()
    return dict(y=y, h=h, rstd=rstd.squeeze(-1), mean=mean.squeeze(-1), dx=dx, dw=(dyd * xh).sum(0), db=dyd.sum(0))


def norm_emulate(x, res, w, b, eps, dy, dres=None, order="kernel", wgrad_dtype=None, mut=""):
    """fp32 arithmetic, one rounding per output. ``mut``: a deliberate fault for tests/test_rowop_oracle_cpu.py
    ("noeps", "div8": mean over D + 8, "proj0.9": the projection term of dx scaled by 0.9)."""
    dt = x.dtype
    rd, rdw = _rd(dt), _rd(wgrad_dtype or w.dtype)
    M, D = x.shape
    NT, MAXV = norm_dispatch(D)
    rsum = (lambda t: kernel_row_sum(t, NT, MAXV)) if order == "kernel" else (lambda t: seq_sum(t, -1))
    csum = (lambda t: kernel_col_sum(t, 256 // NT)) if order == "kernel" else (lambda t: seq_sum(t, 0))
    ln = b is not None
    h = x.float() if res is None else rd(x.float() + res.float())
    wf, dyf = w.float(), dy.float()
    Dd = D + 8 if mut == "div8" else D
    e = 0.0 if mut == "noeps" else eps
    mean = (rsum(h) / Dd)[:, None] if ln else torch.zeros(M, 1)
    d = h - mean
    rstd = torch.rsqrt(rsum(d * d) / Dd + torch.tensor(e, dtype=torch.float32))[:, None]
    y = rd(d * rstd * wf + b.float()) if ln else rd(d * rstd * wf)
    xh = d * rstd
    g = dyf * wf
    a1 = (rsum(g * xh) / D)[:, None]
    a2 = (rsum(g) / D)[:, None] if ln else torch.zeros(M, 1)
    if mut == "proj0.9":
        a1 = a1 * 0.9
    dx = rstd * (g - a2 - xh * a1)
    if dres is not None:
        dx = dx + dres.float()
    return dict(y=y, h=h, rstd=rstd.squeeze(-1), mean=mean.squeeze(-1), dx=rd(dx), dw=rdw(csum(dyf * xh)),
                db=rdw(csum(dyf)))


# ------------------------------------------------------------------ cross-entropy
def _exp(fast):
    if fast:   # kernel-specific step: __expf (module docstring, fast_exp)
        c = torch.tensor(LOG2E, dtype=torch.float32)
        return lambda t: torch.exp2(t * c)
    return torch.exp


def _log(fast):
    if fast:   # __logf
        c = torch.tensor(LN2, dtype=torch.float32)
        return lambda t: torch.log2(t) * c
    return torch.log


def xent_ref64(logits, tgt, ignore_index=-100, smoothing=0.0, scale=1.0, v0=0, Vtot=None, skip_cols=0):
    """fp64 per-row loss, lse and the gradient scale * (softmax - smoothing / Vtot - (1 - smoothing) onehot); ignored
    rows have loss 0 and a zero gradient. ``v0`` / ``Vtot``: the logits are columns [v0, v0 + V) of a wider
    vocabulary (loss and lse are then this chunk's alone). ``skip_cols``: test mutation, the first columns left out of
    the row statistics."""
    x = logits.double()
    N, V = x.shape
    Vtot = V if Vtot is None else Vtot
    xs = x[:, skip_cols:]
    lse = torch.logsumexp(xs, -1)
    valid = tgt != ignore_index
    loc = tgt - v0
    inside = valid & (loc >= 0) & (loc < V)
    idx = torch.where(inside, loc, torch.zeros_like(loc))
    xt = torch.where(inside, x.gather(1, idx[:, None]).squeeze(1), torch.zeros_like(lse))
    loss = (1.0 - smoothing) * (lse - xt) + smoothing * (lse - xs.sum(-1) / Vtot)
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    onehot = torch.zeros_like(x)
    onehot[torch.arange(N, device=x.device)[inside], idx[inside]] = 1.0
    g = torch.exp(x - lse[:, None]) - smoothing / Vtot - (1.0 - smoothing) * onehot
    g = g * (valid.double() * scale)[:, None]
    return dict(loss=loss, lse=lse, grad=g, m=xs.amax(-1), sx=xs.sum(-1), xt=xt)


def xent_stats_emulate(x, order="kernel", h0=None, fast_exp=False, skip_cols=0):
    """(M, S, SX) of x [N, V] (fp32 values): row maximum, sum exp(x - M), sum x. ``h0`` [N]: the scalar head of
    each row (elements before the first 16-byte boundary, xent.hip:36), default 0."""
    E = _exp(fast_exp)
    N, V = x.shape
    if order == "seq":
        xs = x[:, skip_cols:]
        m = xs.amax(-1)
        both = seq_sum(torch.stack([E(xs - m[:, None]), xs]), -1)
        return m, both[0], both[1]
    assert skip_cols == 0, "the skipped-columns mutation is formed in the sequential order"
    h0 = torch.zeros(N, dtype=torch.long) if h0 is None else h0.clamp(max=V)
    Mo, So, Xo = (torch.empty(N, dtype=torch.float32) for _ in range(3))
    ninf = float("-inf")
    for hh in sorted(set(h0.tolist())):
        rows = (h0 == hh).nonzero().squeeze(1)
        xr = x[rows]
        n = xr.shape[0]
        nv = (V - hh) // 8
        K = _cdiv(nv, 256)
        body = F.pad(xr[:, hh:hh + nv * 8], (0, K * 2048 - nv * 8)).view(n, K, 256, 8)
        m = torch.full((n, 256), ninf)
        s = torch.zeros(n, 256)
        sx = torch.zeros(n, 256)
        lane = torch.arange(256)
        for k in range(K):                                        # vector body (:39-51)
            v = body[:, k]
            ok = (k * 256 + lane < nv)[None, :]
            nm = torch.maximum(m, v.amax(-1))
            acc = torch.zeros(n, 256)
            sxn = sx
            for i in range(8):
                acc = acc + E(v[..., i] - nm)
                sxn = sxn + v[..., i]
            sn = s * E(torch.where(m == ninf, torch.full_like(m, ninf), m - nm)) + acc
            m, s, sx = torch.where(ok, nm, m), torch.where(ok, sn, s), torch.where(ok, sxn, sx)

        def upd(vals, m, s, sx):                                  # scalar head / tail: lane i takes element i (:29-33)
            c = vals.shape[1]
            if c == 0:
                return m, s, sx
            mm, ss, xx = m[:, :c], s[:, :c], sx[:, :c]
            up = vals > mm
            s_up = ss * E(torch.where(mm == ninf, torch.full_like(mm, ninf), mm - vals)) + 1.0
            s_dn = ss + E(vals - torch.where(mm == ninf, vals, mm))
            m = torch.cat([torch.where(up, vals, mm), m[:, c:]], 1)
            s = torch.cat([torch.where(up, s_up, s_dn), s[:, c:]], 1)
            sx = torch.cat([xx + vals, sx[:, c:]], 1)
            return m, s, sx
        head, tail = xr[:, :hh], xr[:, hh + nv * 8:]
        m, s, sx = upd(head, m, s, sx)
        m, s, sx = upd(tail, m, s, sx)
        m, s, sx = (t.view(n, 4, 64) for t in (m, s, sx))         # wave, then block (:57-68)
        wm = m.amax(-1)
        ws = torch.where(m == ninf, torch.zeros_like(s), s * E(torch.where(m == ninf, torch.zeros_like(m), m - wm[..., None])))
        ws, wx = _wave_tree(ws), _wave_tree(sx)
        Mr = wm.amax(-1)
        S = torch.zeros(n)
        for i in range(4):
            S = S + torch.where(wm[:, i] == ninf, torch.zeros(n),
                                ws[:, i] * E(torch.where(wm[:, i] == ninf, torch.zeros(n), wm[:, i] - Mr)))
        Mo[rows], So[rows], Xo[rows] = Mr, S, ((wx[:, 0] + wx[:, 1]) + wx[:, 2]) + wx[:, 3]
    return Mo, So, Xo


def xent_grad_emulate(x, tgt, lse, dtype, ignore_index=-100, smoothing=0.0, scale=1.0, v0=0, Vtot=None,
                      fast_exp=False, mut=""):
    """row_grad (xent.hip:73-95): sc * (exp(x - lse) - smoothing / Vtot - [col == y] (1 - smoothing)), rounded once.
    ``mut``: "soft0.5" scales the softmax part by 0.5; "offVc" divides the smoothing by the chunk width."""
    E = _exp(fast_exp)
    N, V = x.shape
    Vtot = V if Vtot is None else Vtot
    f = lambda a: torch.tensor(a, dtype=torch.float32)
    off = f(smoothing) / float(V if mut == "offVc" else Vtot)
    onv = 1.0 - f(smoothing)
    sc = torch.where(tgt != ignore_index, f(scale), f(0.0))[:, None]
    cols = torch.arange(v0, v0 + V)[None, :]
    p = E(x - lse[:, None])
    if mut == "soft0.5":
        p = p * 0.5
    return _rd(dtype)(sc * (p - off - torch.where(cols == tgt[:, None], onv, f(0.0))))


def xent_emulate(logits, tgt, ignore_index=-100, smoothing=0.0, scale=1.0, order="kernel", h0=None, fast_exp=False,
                 mut=""):
    """xent_kernel (xent.hip:97-126) in fp32: per-row loss, lse and the in-place gradient in the logits' dtype."""
    x = logits.float()
    N, V = x.shape
    skip = 7 if mut == "skip7" else 0
    M, S, SX = xent_stats_emulate(x, order, h0, fast_exp, skip)
    lse = M + _log(fast_exp)(S)
    valid = tgt != ignore_index
    xt = x.gather(1, torch.where(valid, tgt, torch.zeros_like(tgt))[:, None]).squeeze(1)
    sm = torch.tensor(smoothing, dtype=torch.float32)
    loss = (1.0 - sm) * (lse - xt) + sm * (lse - SX / V)
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    if mut == "loss+0.1":
        loss = loss + 0.1
    g = xent_grad_emulate(x, tgt, lse, logits.dtype, ignore_index, smoothing, scale, 0, V, fast_exp, mut)
    return dict(loss=loss, lse=lse, grad=g)


def chunk_fold_emulate(run, M, S, SX, xt_new, fast_exp=False, dt=torch.float32):
    """xent_chunk_stats_kernel thread 0 (xent.hip:147-155): fold a chunk's (M, S, SX) into the running (m, s, t, x);
    ``xt_new``: (inside mask, target logit). Returns the new (m, s, t, x). dt fp64: the oracle's running values."""
    E = _exp(fast_exp) if dt == torch.float32 else torch.exp
    m0, s0, t0, x0 = (r.to(dt) for r in run)
    M, S, SX = M.to(dt), S.to(dt), SX.to(dt)
    ninf = float("-inf")
    nm = torch.maximum(m0, M)
    z = torch.zeros_like(s0)
    s = torch.where(m0 == ninf, z, s0 * E(torch.where(m0 == ninf, z, m0 - nm))) + \
        torch.where(M == ninf, z, S * E(torch.where(M == ninf, z, M - nm)))
    inside, xt = xt_new
    return nm, s, torch.where(inside, xt.to(dt), t0), x0 + SX


# ------------------------------------------------------------------ rope
def _fma(a, b, c):
    """fl32(a * b + c) for fp32 a, b, c: the product is exact in fp64 (2 x 24 bits)."""
    return (a.double() * b.double() + c.double()).float()


def rope_apply(x, cos, sin, pos, mode, inverse, dt=torch.float64, rd=None, order="kernel", mut=""):
    """rope_kernel (rope.hip:26-85) on x [B, T, H, hd] (every head rotated), cos / sin fp32 tables [Tmax, hd / 2],
    pos int [B, T]. mode 0: interleaved pairs, 1: rotate_half pairs, 2: the Gemma-reference map y_e = c (x_e + x_o),
    y_o = s (x_o - x_e), whose "inverse" is its transpose dx_e = c dy_e - s dy_o, dx_o = c dy_e + s dy_o (not a
    rotation). dt fp64: the reference; fp32 with ``rd``: the emulation ("kernel": products contracted into fused
    multiply-adds as hipcc does, "seq": every product rounded). ``mut``: "half" / "quarter": the upper half / quarter of the
    pairs not rotated; "fwdinv": the mode-2 inverse using the forward map."""
    B, T, H, hd = x.shape
    c = cos[pos.long()].to(dt)[:, :, None, :]
    s = sin[pos.long()].to(dt)[:, :, None, :]
    xf = x.to(dt)
    if mode == 1:
        x0, x1 = xf[..., :hd // 2], xf[..., hd // 2:]
    else:
        x0, x1 = xf[..., 0::2], xf[..., 1::2]
    fused = dt == torch.float32 and order == "kernel"
    if mode == 2 and mut == "fwdinv":
        inverse = False
    if mode == 2:
        if not inverse:
            o0, o1 = c * (x0 + x1), s * (x1 - x0)
        elif fused:
            o0, o1 = _fma(c, x0, -(s * x1)), _fma(c, x0, s * x1)
        else:
            o0, o1 = c * x0 - s * x1, c * x0 + s * x1
    else:
        sn = -s if inverse else s
        if fused:
            o0, o1 = _fma(x0, c, -(x1 * sn)), _fma(x0, sn, x1 * c)
        else:
            o0, o1 = x0 * c - x1 * sn, x0 * sn + x1 * c
    if mut in ("half", "quarter"):
        hp = hd // 4 if mut == "half" else 3 * hd // 8
        o0 = torch.cat([o0[..., :hp], x0[..., hp:].expand_as(o0[..., hp:])], -1)
        o1 = torch.cat([o1[..., :hp], x1[..., hp:].expand_as(o1[..., hp:])], -1)
    out = torch.cat([o0, o1], -1) if mode == 1 else torch.stack([o0, o1], -1).flatten(-2)
    return rd(out) if rd is not None else out


def rope_ref64(x, cos, sin, pos, mode, inverse):
    return rope_apply(x, cos, sin, pos, mode, inverse)


def rope_emulate(x, cos, sin, pos, mode, inverse, order="kernel", mut=""):
    return rope_apply(x, cos, sin, pos, mode, inverse, torch.float32, _rd(x.dtype), order, mut)


# ------------------------------------------------------------------ GLU
K0, K1 = 0.7978845608028654, 0.044715
GLU_KINDS = {"gelu_tanh": 4, "gelu": 5, "silu": 6}   # act_common.h ActKind


def _act64(g, kind):
    """(act, d act / dg) in fp64, cancellation-free forms (erfc for the Gaussian tail, sigmoid for silu)."""
    if kind == "silu":
        s = torch.sigmoid(g)
        return g * s, s * (1.0 + g * (1.0 - s))
    if kind == "gelu":
        cdf = 0.5 * torch.erfc(-g * 0.7071067811865476)
        return g * cdf, cdf + g * 0.3989422804014327 * torch.exp(-0.5 * g * g)
    if kind == "gelu_tanh":
        u = K0 * (g + K1 * g ** 3)
        cdf = torch.sigmoid(2.0 * u)                       # 0.5 (1 + tanh u) without the cancellation at u << 0
        return g * cdf, cdf + g * 2.0 * cdf * (1.0 - cdf) * K0 * (1.0 + 3.0 * K1 * g * g)
    raise ValueError(kind)


def _act32(g, kind, order, fast_exp):
    """(act, d act) in fp32. "kernel": the expressions of act_common.h act_f / act_df; "seq": torch's own."""
    E = _exp(fast_exp)
    if order == "kernel":
        if kind == "silu":
            s = 1.0 / (1.0 + E(-g))
            return g / (1.0 + E(-g)), s * (1.0 + g * (1.0 - s))
        if kind == "gelu":
            cdf = 0.5 * (1.0 + torch.erf(g * 0.7071067811865476))
            return 0.5 * g * (1.0 + torch.erf(g * 0.7071067811865476)), cdf + g * (0.3989422804014327 * E(-0.5 * g * g))
        u = K0 * (g + K1 * g * g * g)
        th = torch.tanh(u)
        return 0.5 * g * (1.0 + th), 0.5 * (1.0 + th) + 0.5 * g * (1.0 - th * th) * K0 * (1.0 + 3.0 * K1 * g * g)
    raise ValueError(order)


def glu_ref64(gu, dy, kind):
    """y = act(g) u, dg = dy u act'(g), du = dy act(g) for gu = [g | u] ([M, 2F]), fp64. dgu = [dg | du]."""
    g, u = gu.double().chunk(2, -1)
    a, da = _act64(g, kind)
    d = dy.double()
    return dict(y=a * u, dgu=torch.cat([d * u * da, d * a], -1))


def glu_emulate(gu, dy, kind, order="kernel", fast_exp=False):
    rd = _rd(gu.dtype)
    g, u = gu.float().chunk(2, -1)
    d = dy.float()
    if order != "kernel":      # "seq": ops/reference.py glu (torch's own activations) and its autograd gradients
        gl = gu.float().detach().requires_grad_()
        gg, ul = gl.chunk(2, -1)
        a = F.silu(gg) if kind == "silu" else F.gelu(gg) if kind == "gelu" else \
            0.5 * gg * (1 + torch.tanh(math.sqrt(2 / math.pi) * (gg + 0.044715 * gg ** 3)))
        y = a * ul
        (dgu,) = torch.autograd.grad(y, gl, d)
        return dict(y=rd(y.detach()), dgu=rd(dgu))
    a, da = _act32(g, kind, order, fast_exp)
    return dict(y=rd(a * u), dgu=torch.cat([rd(d * u * da), rd(d * a)], -1))


# ------------------------------------------------------------------ AdamW
def adamw_ref64(src, g, m, v, lr, b1, b2, eps, wd, step, coef=1.0, adam_l2=False, mut=""):
    """One AdamW step in fp64 from the state the kernel receives: src (the master, or p without one), g, m, v and the
    hyperparameters as the op receives them (doubles: rounding them to fp32 is the kernel's own, and 1 - fl32(0.9) is
    four fp32 ulps from 0.1, which the kernel-shaped emulation carries too).
    Returns (new src, new m, new v) before any storage rounding. ``mut``: "nodecay", "step+1" (test mutations)."""
    p, gr, m, v = src.double(), g.double() * coef, m.double(), v.double()
    if adam_l2:
        gr = gr + wd * p
    m = b1 * m + (1.0 - b1) * gr
    v = b2 * v + (1.0 - b2) * gr * gr
    st = step + 1 if mut == "step+1" else step
    bc1, bc2 = 1.0 - b1 ** st, 1.0 - b2 ** st
    if not adam_l2 and mut != "nodecay":
        p = p * (1.0 - lr * wd)
    return p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps), m, v


def adamw_emulate(src, g, m, v, lr, b1, b2, eps, wd, step, coef=1.0, adam_l2=False, order="kernel", mut=""):
    """The step in fp32 with the moments rounded to their stored dtype after the update and the master kept in
    fp32 (optim.hip:61-70). "kernel": the kernel's expression with the host's fp32 bias corrections (:164-165);
    "seq": ops/reference.py adamw_ (lr / bc1 and sqrt(bc2) formed in double by the host, as torch.optim does).
    Returns (new src fp32, new m, new v) with m, v holding values of their stored dtype."""
    f = lambda a: torch.tensor(a, dtype=torch.float32)
    p, mf, vf = src.float(), m.float(), v.float()
    gr = g.float() * f(coef)
    lr_, b1_, b2_, eps_, wd_ = f(lr), f(b1), f(b2), f(eps), f(wd)
    if adam_l2 and order != "kernel":
        gr = gr + wd * p
    st = step + 1 if mut == "step+1" else step
    if order == "kernel":       # products feeding a sum contracted into fused multiply-adds, as hipcc compiles :62-69
        if adam_l2:
            gr = _fma(wd_.expand_as(p), p, g.float() * f(coef))
        mf = _fma(b1_.expand_as(mf), mf, (1.0 - b1_) * gr)
        vf = _fma(b2_.expand_as(vf), vf, (1.0 - b2_) * gr * gr)
        # the host's std::pow(float, float): the correctly rounded fp32 power, formed in double and rounded once, so
        # that it does not depend on torch's vectorised pow (1 / (1 - b^t) amplifies an ulp of it)
        powf = lambda b, t: f(math.pow(float(b), float(t)))
        inv_bc1 = 1.0 / (1.0 - powf(b1_, st))
        # the correctly rounded square root of the host and of the kernel (hipcc's default), taken in double and rounded
        # once: torch.sqrt on fp32 CPU tensors is not correctly rounded, and by how much depends on the CPU
        sqrt32 = lambda t: t.double().sqrt().float()
        inv_sqrt_bc2 = 1.0 / sqrt32(1.0 - powf(b2_, st))
        denom = _fma(sqrt32(vf), inv_sqrt_bc2.expand_as(vf), eps_.expand_as(vf))
        if not adam_l2 and mut != "nodecay":
            p = p * _fma(-lr_, wd_, f(1.0))      # rounded: the select on adam_l2 keeps it out of the subtraction
        p = p - lr_ * inv_bc1 * mf / denom
    else:                       # ops/reference.py adamw_, operation for operation
        mf = mf.clone().mul_(b1).add_(gr, alpha=1 - b1)
        vf = vf.clone().mul_(b2).addcmul_(gr, gr, value=1 - b2)
        bc1, bc2 = 1 - b1 ** st, 1 - b2 ** st
        denom = vf.sqrt() / math.sqrt(bc2) + eps
        if not adam_l2 and mut != "nodecay":
            p = p * (1 - lr * wd)
        p = p - (lr / bc1) * mf / denom
    return p, _rd(m.dtype)(mf), _rd(v.dtype)(vf)


# ------------------------------------------------------------------ measures
def _unit_index(M, D, device):
    g = max(1, _cdiv(UNIT, D))
    nu = max(1, M // g)
    return (torch.arange(M, device=device) // g).clamp(max=nu - 1), nu


def row_errors(x, ref):
    """x, ref [.., D] -> (rms [nu], maxabs [nu]) of x - ref per unit: one row of the flattened [M, D], or (D < 64)
    consecutive rows totalling at least 64 elements; a short remainder joins the last unit."""
    D = ref.shape[-1]
    e = (x.double() - ref.double()).reshape(-1, D)
    idx, nu = _unit_index(e.shape[0], D, e.device)
    z = torch.zeros(nu, dtype=torch.float64, device=e.device)
    ss = z.clone().index_add_(0, idx, e.square().sum(-1))
    cnt = z.clone().index_add_(0, idx, torch.full_like(e[:, 0], float(D)))
    mx = z.clone().scatter_reduce_(0, idx, e.abs().amax(-1) if D else e[:, 0], "amax", include_self=True)
    return (ss / cnt.clamp_min(1.0)).sqrt(), mx


def col_errors(x, ref):
    """x, ref [D] or [R, D] -> per 64 consecutive columns (all rows): (rms, maxabs)."""
    e = (x.double() - ref.double())
    e = e.reshape(-1, e.shape[-1])
    R, D = e.shape
    nb = _cdiv(D, UNIT)
    e = F.pad(e, (0, nb * UNIT - D)).view(R, nb, UNIT).transpose(0, 1).reshape(nb, -1)
    n = torch.full((nb,), float(R * UNIT), dtype=torch.float64, device=e.device)
    n[-1] = float(R * (D - (nb - 1) * UNIT))
    return (e.square().sum(-1) / n).sqrt(), e.abs().amax(-1)


def unit_ratios(x, ref, yard, cols=False, floor=0.0):
    """(worst rms ratio, worst maxabs ratio, (kr, km, yr, ym)) of x against the yardstick (one tensor, or the
    per-unit larger of several). A unit whose yardstick error and floor are zero and which x matches exactly has
    ratio 0."""
    fn = col_errors if cols else row_errors
    kr, km = fn(x, ref)
    ys = yard if isinstance(yard, (list, tuple)) else [yard]
    es = [fn(y, ref) for y in ys]
    yr = torch.stack([e[0] for e in es]).amax(0).clamp_min(floor)
    ym = torch.stack([e[1] for e in es]).amax(0).clamp_min(floor)
    big = 1e300
    rr = torch.where(kr > 0, kr / yr.clamp_min(1.0 / big), torch.zeros_like(kr))
    rm = torch.where(km > 0, km / ym.clamp_min(1.0 / big), torch.zeros_like(km))
    return rr, rm, (kr, km, yr, ym)


def assert_units(x, ref, yard, name, rms_margin, max_margin, cols=False, floor=0.0):
    """Every unit of x: rms error <= rms_margin x the yardstick's, max-abs error <= max_margin x the yardstick's
    (both against ``ref``). Returns the worst (rms, maxabs) ratios."""
    assert x.shape == ref.shape, (name, tuple(x.shape), tuple(ref.shape))
    assert bool(torch.isfinite(x.float()).all()), f"{name}: non-finite values"
    rr, rm, (kr, km, yr, ym) = unit_ratios(x, ref, yard, cols, floor)
    for what, ratio, ke, ye, margin in (("rms", rr, kr, yr, rms_margin), ("maxabs", rm, km, ym, max_margin)):
        bad = ke > margin * ye
        if bool(bad.any()):
            i = int(torch.where(bad, ratio, torch.zeros_like(ratio)).argmax())
            raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} units over the {what} bound; worst unit {i}: "
                                 f"{what} error {ke[i].item():.3e} vs yardstick {ye[i].item():.3e} "
                                 f"(ratio {ratio[i].item():.2f} > {margin})")
    return float(rr.max()), float(rm.max())


def _elem_check(x, ref, yards, name, margin, floor):
    x, ref = x.double().reshape(-1), ref.double().reshape(-1)
    assert bool(torch.isfinite(x).all()), f"{name}: non-finite values"
    ys = yards if isinstance(yards, (list, tuple)) else [yards]
    ye = torch.stack([(y.double().reshape(-1) - ref).abs() for y in ys]).amax(0)
    ye = torch.maximum(ye, floor if torch.is_tensor(floor) else torch.full_like(ye, float(floor)))
    ke = (x - ref).abs()
    bad = ke > margin * ye
    ratio = torch.where(ke > 0, ke / ye.clamp_min(1e-300), torch.zeros_like(ke))
    if bool(bad.any()):
        i = int(torch.where(bad, ratio, torch.zeros_like(ratio)).argmax())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} entries over the bound; worst entry {i}: got "
                             f"{x[i].item():.9g}, reference {ref[i].item():.9g}, error {ke[i].item():.3e} vs yardstick "
                             f"{ye[i].item():.3e} (ratio {ratio[i].item():.2f} > {margin})")
    return float(ratio.max()) if ratio.numel() else 0.0


def assert_scalars(x, ref, yards, name, margin=SCALAR_MARGIN):
    """Per-row fp32 scalars: |x - ref| <= margin x max(yardsticks' |error|, |ref| * 2^-24) per row."""
    return _elem_check(x, ref, yards, name, margin, ref.double().reshape(-1).abs() * 2.0 ** -24)


def half_ulp(ref, dtype):
    """Half an ulp of ``dtype`` at |ref| (fp64 tensor), the smallest normal's for smaller values."""
    mant, tiny = (8, 2.0 ** -126) if dtype == torch.bfloat16 else (24, 2.0 ** -126)
    e = torch.frexp(ref.double().abs().clamp_min(tiny))[1].double()      # |ref| = f * 2^e, f in [0.5, 1)
    return torch.exp2(e - mant - 1)


def assert_elements(x, ref, yards, name, dtype, margin=SCALAR_MARGIN, at=None):
    """Single stored elements (no unit to average over): |x - ref| <= margin x max(yardsticks' |error|, half an
    ulp of the stored ``dtype`` at |at| (default |ref|))."""
    return _elem_check(x, ref, yards, name, margin, half_ulp(ref if at is None else at, dtype).reshape(-1))


def split_target(g, tgt, v0=0):
    """(gradient with the target entries zeroed, the target entries [N], inside mask): the one-hot column of a
    cross-entropy gradient is measured on its own."""
    N, V = g.shape
    loc = tgt - v0
    inside = (loc >= 0) & (loc < V)
    idx = torch.where(inside, loc, torch.zeros_like(loc))
    t = torch.where(inside, g.gather(1, idx[:, None]).squeeze(1), torch.zeros_like(g[:, 0]))
    rest = g.clone()
    rest[torch.arange(N, device=g.device)[inside], idx[inside]] = 0
    return rest, t, inside


# ------------------------------------------------------------------ inputs
NORM_KINDS = ("randn", "tiny", "offset", "spike")
XENT_KINDS = ("randn", "edges", "wide")


def make_inputs(op, kind, dtype, seed=0, **k):
    """Seeded inputs (CPU generator: the same values on every device), rounded to ``dtype``; a dict of CPU tensors.
    norm (M, D, ln, res): x, res, w, b, dy, dres. kinds: randn; tiny (rows scaled by 2^-9, so eps carries weight);
      offset (rows with mean 30 x std); spike (one element 2^10 x the rest, in the first vector of even rows and the
      last vector of odd rows).
    xent (N, V): logits (randn * 2), tgt with row 3 ignored (N > 3). kinds: randn; edges (the row maximum and the
      target in columns 0-6 and the last 7 columns, cycling over the rows); wide (logits spread over +-40).
    rope (B, T, NH, hd): x. glu (M, F, grid): gu, dy; grid: gate values on a grid over [-30, 30] crossed with up / dy of
      both signs. adamw (n): p, g (3 steps)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    if op == "norm":
        M, D = k["M"], k["D"]
        x = rn(M, D)
        r = rn(M, D) if k.get("res") else None
        if kind == "tiny":
            x = x * 2.0 ** -9
            r = r * 2.0 ** -9 if r is not None else None
        elif kind == "offset":
            x = x + 30.0
        elif kind == "spike":
            col = torch.where(torch.arange(M) % 2 == 0, torch.full((M,), 3), torch.full((M,), D - 2))
            x[torch.arange(M), col.clamp(0, D - 1)] = 1024.0
        elif kind != "randn":
            raise ValueError(kind)
        w = torch.rand(D, generator=gen) + 0.5
        b = rn(D) if k.get("ln") else None
        dy = rn(M, D)
        dres = rn(M, D) if k.get("res") else None
        c = lambda t: None if t is None else t.to(dtype)
        return dict(x=c(x), res=c(r), w=c(w), b=c(b), dy=c(dy), dres=c(dres))
    if op == "xent":
        N, V = k["N"], k["V"]
        x = rn(N, V) * 2.0
        tgt = torch.randint(0, V, (N,), generator=gen)
        if kind == "wide":
            x = (torch.rand(N, V, generator=gen) * 80.0 - 40.0)
        elif kind == "edges":
            spots = [c for c in list(range(0, 7)) + list(range(V - 7, V)) if 0 <= c < V]
            spots = sorted(set(spots))
            for i in range(N):
                cm, ct = spots[i % len(spots)], spots[(i * 3 + 1) % len(spots)]
                x[i, cm] = 12.0 + i * 0.125
                tgt[i] = ct
        elif kind != "randn":
            raise ValueError(kind)
        if N > 3:
            tgt[3] = -100
        return dict(logits=x.to(dtype), tgt=tgt)
    if op == "rope":
        return dict(x=rn(k["B"], k["T"], k["NH"], k["hd"]).to(dtype))
    if op == "glu":
        M, Fd = k["M"], k["F"]
        if kind == "grid":
            pts = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** -133, -2.0 ** -133]   # 2^-133: bf16's smallest subnormal
            pts += [s * a for a in (0.125, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0, 16.0, 20.0, 25.0, 30.0)
                    for s in (1.0, -1.0)]
            pts += torch.linspace(-30.0, 30.0, 37).tolist()
            pts = torch.tensor(pts, dtype=torch.float32)
            n = M * Fd
            g = pts[torch.arange(n) % pts.numel()].view(M, Fd)
            # up / dy of both signs: the sign pattern has period 4 against the grid's own period
            sg = lambda ph: torch.where(((torch.arange(n) // pts.numel() + ph) % 2) == 0, 1.0, -1.0).view(M, Fd)
            u = (rn(M, Fd).abs() + 0.25) * sg(0)
            dy = (rn(M, Fd).abs() + 0.25) * sg(1) * torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0).view(M, Fd)
        elif kind == "randn":
            g, u, dy = rn(M, Fd), rn(M, Fd), rn(M, Fd)
        else:
            raise ValueError(kind)
        return dict(gu=torch.cat([g, u], -1).to(dtype), dy=dy.to(dtype))
    if op == "adamw":
        n = k["n"]
        return dict(p=rn(n), grads=[rn(n) for _ in range(k.get("steps", 3))])
    raise ValueError(op)
