"""Pure-PyTorch fp32 oracles for every HIP op.

These are the numerics reference for the GPU kernel tests and the CPU
execution path (the tiny-GPT CPU plumbing config). They follow the reference
notebooks' math exactly; citations are on each function.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

def _f(t):
    """fp32 compute, or fp64 for fp64 inputs (the CPU numeric-parity tests run whole models in fp64)."""
    return t if t.dtype == torch.float64 else t.float()


ACT_KINDS = {
    "relu": 0, "leaky_relu": 1, "prelu": 2, "elu": 3, "gelu_tanh": 4, "gelu": 5, "gelu_erf": 5,
    "silu": 6, "swish": 6, "sigmoid": 7, "tanh": 8, "identity": 9,
}


def rms_norm(x, w, eps, residual=None):
    """llama3/LLaMA-jax.ipynb:536-538; gemma/gemma.ipynb:139-150 (fp32 compute)."""
    h = x if residual is None else (_f(x) + _f(residual)).to(x.dtype)
    hf = _f(h)
    y = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + eps) * _f(w)
    return y.to(x.dtype), h


def layer_norm(x, w, b, eps, residual=None):
    """gpt/gpt-jax.ipynb:414-416 (flax LayerNorm eps 1e-6); ViT.ipynb:205-206."""
    h = x if residual is None else (_f(x) + _f(residual)).to(x.dtype)
    y = F.layer_norm(_f(h), (h.shape[-1],), _f(w), _f(b), eps)
    return y.to(x.dtype), h


def act(x, kind: str, alpha: float = 0.0):
    """activation functions/GELU.ipynb:54-55, ReLU.ipynb:20-54."""
    xf = _f(x)
    if kind == "relu":
        y = F.relu(xf)
    elif kind in ("leaky_relu", "prelu"):
        y = torch.where(xf > 0, xf, alpha * xf)
    elif kind == "elu":
        y = torch.where(xf > 0, xf, alpha * (torch.exp(xf) - 1))
    elif kind == "gelu_tanh":
        y = 0.5 * xf * (1 + torch.tanh(math.sqrt(2 / math.pi) * (xf + 0.044715 * xf ** 3)))
    elif kind in ("gelu", "gelu_erf"):
        y = F.gelu(xf)
    elif kind in ("silu", "swish"):
        y = F.silu(xf)
    elif kind == "sigmoid":
        y = torch.sigmoid(xf)
    elif kind == "tanh":
        y = torch.tanh(xf)
    elif kind == "identity":
        y = xf
    else:
        raise ValueError(kind)
    return y.to(x.dtype)


def glu(gu, kind: str):
    """SwiGLU llama3/LLaMA-jax.ipynb:854-855 (gate=w3 in the ref), GeGLU gemma.ipynb:281-286."""
    g, u = _f(gu).chunk(2, dim=-1)
    return (_f(act(g, kind)) * u).to(gu.dtype)


def rope_tables(T, hd, theta=10000.0, device=None, ref_freqs=False):
    """Angles t*freq_i, i < hd/2. Standard (Meta) freq_i = theta^(-2i/hd);
    ``ref_freqs=True`` reproduces llama3/LLaMA-jax.ipynb:563-567 exactly, whose
    precompute_freqs_cis uses arange(0, dim//2)/dim, i.e. theta^(-i/hd)."""
    expo = torch.arange(0, hd // 2, dtype=torch.float64) / hd if ref_freqs else \
        torch.arange(0, hd, 2, dtype=torch.float64) / hd
    inv = 1.0 / (theta ** expo)
    t = torch.arange(T, dtype=torch.float64)
    ang = torch.outer(t, inv)
    return ang.cos().float().to(device), ang.sin().float().to(device)


def rope(x, cos, sin, pos_off=0, interleaved=True, inverse=False, positions=None):
    """apply_rotary_emb llama3/LLaMA-jax.ipynb:592-601; x [B,T,H,hd]."""
    B, T, H, hd = x.shape
    if positions is None:
        c = cos[pos_off:pos_off + T][None, :, None, :]
        s = sin[pos_off:pos_off + T][None, :, None, :]
    else:
        c = cos[positions.long()][:, :, None, :]
        s = sin[positions.long()][:, :, None, :]
    if inverse:
        s = -s
    xf = _f(x)
    if interleaved:
        x0, x1 = xf[..., 0::2], xf[..., 1::2]
        o0 = x0 * c - x1 * s
        o1 = x0 * s + x1 * c
        out = torch.stack([o0, o1], dim=-1).flatten(-2)
    else:
        x0, x1 = xf[..., : hd // 2], xf[..., hd // 2:]
        out = torch.cat([x0 * c - x1 * s, x0 * s + x1 * c], dim=-1)
    return out.to(x.dtype)


def attention(q, k, v, causal=True, scale=None):
    """Materialised softmax(QK^T*scale + mask) V with GQA head mapping.

    q [B,Tq,H,hd], k/v [B,Tk,Hkv,hd]; causal aligned bottom-right (key j visible
    to query i iff j <= i + Tk - Tq). gpt-jax.ipynb:344-353, LLaMA-jax.ipynb:809-829.
    Returns (out [B,Tq,H,hd], lse [B,H,Tq]).
    """
    B, Tq, H, hd = q.shape
    Tk, Hkv = k.shape[1], k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    rep = H // Hkv
    kf = _f(k).repeat_interleave(rep, dim=2)
    vf = _f(v).repeat_interleave(rep, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", _f(q), kf) * scale
    if causal:
        i = torch.arange(Tq, device=q.device)[:, None]
        j = torch.arange(Tk, device=q.device)[None, :]
        s = s.masked_fill(j > i + (Tk - Tq), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1).nan_to_num(0.0)
    o = torch.einsum("bhqk,bkhd->bqhd", p, vf)
    return o.to(q.dtype), lse


def cross_entropy(logits, target, ignore_index=-100, smoothing=0.0):
    """Per-row CE losses (fp32), F.cross_entropy semantics. gpt-jax.ipynb:503."""
    return F.cross_entropy(_f(logits), target, ignore_index=ignore_index, reduction="none",
                           label_smoothing=smoothing)


def embedding(W, idx, pos=None, scale=1.0):
    if bool((idx < 0).any()):       # negative id: a zero row (vocab-parallel foreign tokens)
        keep = (idx >= 0).unsqueeze(-1).to(W.dtype)
        out = W[idx.clamp_min(0)] * keep
        out = out * scale if scale != 1.0 else out
    else:
        out = W[idx] * scale if scale != 1.0 else W[idx]
    if pos is not None:
        T = idx.shape[-1]
        out = out + pos.reshape(-1, W.shape[1])[:T]
    return out


def adamw_(p, master, g, m, v, lr, b1, b2, eps, wd, step, coef=None, adam_l2=False):
    """torch.optim.AdamW / Adam math on flat fp32 state (in place). A NaN ``coef``
    (non-finite global grad norm) skips the update, as the HIP kernel does."""
    if coef is not None and bool(torch.isnan(coef).any()):
        return
    src = master if master is not None else p
    pf = src.float()
    gf = g.float() * (coef.float() if coef is not None else 1.0)
    if adam_l2:
        gf = gf + wd * pf
    mf = m.float().mul_(b1).add_(gf, alpha=1 - b1)      # bf16 moments: update in fp32, store rounded
    vf = v.float().mul_(b2).addcmul_(gf, gf, value=1 - b2)
    m.copy_(mf)
    v.copy_(vf)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = vf.sqrt() / math.sqrt(bc2) + eps
    if not adam_l2:
        pf = pf * (1 - lr * wd)
    pf = pf - (lr / bc1) * mf / denom
    if master is not None:
        master.copy_(pf)
    p.copy_(pf.to(p.dtype))


def sgd_(p, master, g, buf, lr, momentum, wd, coef=None):
    if coef is not None and bool(torch.isnan(coef).any()):
        return
    src = master if master is not None else p
    pf = src.float()
    gf = g.float() * (coef.float() if coef is not None else 1.0) + wd * pf
    if buf is not None:
        buf.mul_(momentum).add_(gf)
        gf = buf
    pf = pf - lr * gf
    if master is not None:
        master.copy_(pf)
    p.copy_(pf.to(p.dtype))


def dequant_w8(wq, s):
    """fp32 weights of a block-scaled e4m3 image: wq [.., N, K] float8_e4m3fn, s [.., N/128, K/128]
    uint8 E8M0 (one scale per 128 x 128 block, DeepSeek-V3, arXiv 2412.19437 sec. 3.3) ->
    q * 2^(s - 127). Every value is exact in bf16."""
    N, K = wq.shape[-2:]
    lead = wq.shape[:-2]
    t = wq.float().view(*lead, N // 128, 128, K // 128, 128)
    return (t * torch.exp2(s.float() - 127)[..., :, None, :, None]).reshape(*lead, N, K)


def gemv_w8(x, wq, s):
    """x [M, K] times the dequantised image [N, K]^T, fp32 (csrc/kernels/gemv.hip)."""
    return x.float() @ dequant_w8(wq, s).t()


def grouped_gemv_w8(x, wq, s, offsets):
    """Expert-sorted rows x [A, K] times the dequantised image of their expert, wq [E, N, K],
    offsets [E+1]: fp32 [A, N]."""
    off = offsets.tolist()
    w = dequant_w8(wq, s)
    out = torch.zeros(x.shape[0], wq.shape[1], dtype=torch.float32, device=x.device)
    for e in range(len(off) - 1):
        if off[e + 1] > off[e]:
            out[off[e]:off[e + 1]] = x[off[e]:off[e + 1]].float() @ w[e].t()
    return out


E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # OCP e2m1 magnitudes by code


def quant_mxfp4(W):
    """The OCP MXFP4 image of W [.., N, K], K % 32 == 0 (bf16 values in any floating dtype):
    (wq uint8 [.., N, K/2], s uint8 E8M0 [.., N, K/32]) with w ~= value(code) * 2^(s - 127). Byte j of a
    row holds the code of k = 2j in bits 3:0 and of k = 2j + 1 in bits 7:4; a code is sign << 3 | mag,
    mag 0..7 = 0, .5, 1, 1.5, 2, 3, 4, 6. One scale per 32 consecutive k of one row: e the smallest
    integer with amax <= 6 * 2^e (read off amax's fp32 bits: amax = m 2^p needs e = p - 2 when m <= 1.5,
    else p - 1), clamped to [-126, 125], 0 for an all-zero block. |w| / 2^e, exact in fp32, goes to the
    nearest magnitude (saturating at 6), a tie to the even code; the sign bit is the weight's own.
    Bit-exact with quant_weight_mxfp4 (csrc/kernels/quant_mxfp4.hip).

    Requantising a dequantised image returns the same VALUES bit for bit, but not always the same bytes: a
    block whose amax rounded down to 3 * 2^e is rescaled to 6 * 2^(e - 1) (every code's value doubles
    exactly), and a block that rounded to all zeros takes the zero block's scale. The bytes are a fixed
    point from that second image on (tests/test_quant_w4_cpu.py)."""
    *lead, N, K = W.shape
    assert K % 32 == 0, K
    t = W.detach().float().reshape(*lead, N, K // 32, 32)
    a = t.abs()
    amax = a.amax(-1)
    bits = amax.contiguous().view(torch.int32)
    e = ((bits >> 23) & 0xff) - 127 - torch.where((bits & 0x7fffff) <= 0x400000, 2, 1)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp(-126, 125)
    v = a * torch.exp2(-e.float())[..., None]
    code = ((v > 0.25).int() + (v >= 0.75).int() + (v > 1.25).int() + (v >= 1.75).int() + (v > 2.5).int()
            + (v >= 3.5).int() + (v > 5.0).int()) | (torch.signbit(t).int() << 3)
    code = code.reshape(*lead, N, K // 2, 2)
    wq = (code[..., 0] | (code[..., 1] << 4)).to(torch.uint8)
    return wq, (e + 127).to(torch.uint8)


def dequant_w4(wq, s):
    """fp32 weights of an MXFP4 image (:func:`quant_mxfp4`'s layout): wq uint8 [.., N, K/2],
    s uint8 [.., N, K/32] -> value(code) * 2^(s - 127), [.., N, K]. Every value is exact in bf16."""
    *lead, N, K2 = wq.shape
    lut = torch.tensor(E2M1 + tuple(-m for m in E2M1), dtype=torch.float32, device=wq.device)
    q = wq.to(torch.int64)
    v = lut[torch.stack((q & 0xf, q >> 4), -1)].reshape(*lead, N, K2 // 16, 32)
    return (v * torch.exp2(s.float() - 127)[..., None]).reshape(*lead, N, 2 * K2)


def gemv_w4(x, wq, s):
    """x [M, K] times the dequantised MXFP4 image [N, K]^T, fp32 (csrc/kernels/gemv.hip)."""
    return x.float() @ dequant_w4(wq, s).t()


def grouped_gemv_w4(x, wq, s, offsets):
    """Expert-sorted rows x [A, K] times the dequantised MXFP4 image of their expert, wq [E, N, K/2],
    offsets [E+1]: fp32 [A, N]."""
    off = offsets.tolist()
    w = dequant_w4(wq, s)
    out = torch.zeros(x.shape[0], wq.shape[1], dtype=torch.float32, device=x.device)
    for e in range(len(off) - 1):
        if off[e + 1] > off[e]:
            out[off[e]:off[e + 1]] = x[off[e]:off[e + 1]].float() @ w[e].t()
    return out


def quant_kv8(x):
    """fp8 KV-cache rows: x [B, T, Hkv, hd] -> (q float8_e4m3fn [B, T, Hkv, hd], s uint8 E8M0
    [B, Hkv, T]) with x ~= q * 2^(s - 127), one scale per (batch, kv head, token) over the row's hd
    values: the smallest exponent with amax / 2^e <= 448 (ops/moe.py _e8m0), the scaled values clamped
    to +-448 and rounded to e4m3. Bit-exact with kv_quant_write_ / rope_kv_write_q8_ (csrc/kernels/rope.hip)."""
    from .moe import _e8m0
    xf = x.float()
    e = _e8m0(xf.abs().amax(-1))                                            # [B, T, Hkv]
    q = (xf * torch.exp2(-e.float())[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn)
    return q, (e + 127).to(torch.uint8).transpose(1, 2).contiguous()


def dequant_kv8(q, s, dtype=torch.float32):
    """Inverse of :func:`quant_kv8`: q [B, T, Hkv, hd] e4m3, s [B, Hkv, >= T] -> q * 2^(s - 127) in
    ``dtype``. Every value is exact in bf16 and fp32."""
    T = q.shape[1]
    return (q.float() * torch.exp2(s[:, :, :T].float() - 127).transpose(1, 2)[..., None]).to(dtype)


def attn_decode_q8(q, kq, ks, vq, vs, causal=True, scale=None):
    """Decode attention over an fp8 cache (csrc/kernels/decode.hip attn_decode_q8): :func:`attention`
    on the dequantised rows. Returns (out, lse)."""
    return attention(_f(q), dequant_kv8(kq, ks), dequant_kv8(vq, vs), causal, scale)


def attention_per_row(q, k, v, kv_len, causal=True, scale=None):
    """Ragged-batch decode attention (attn_decode / attn_decode_q8 with ``per_row``): sequence b
    attends over its own cache rows [0, min(kv_len[b], Tk)), whose last Tq rows are its query
    tokens. k / v are the whole cache buffers [B, Tk, Hkv, hd]. Returns (out, lse)."""
    lens = [min(int(n), k.shape[1]) for n in torch.as_tensor(kv_len).reshape(-1).tolist()]
    if len(lens) != q.shape[0]:
        raise ValueError(f"attention_per_row: {len(lens)} lengths for a batch of {q.shape[0]}")
    parts = [attention(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], causal, scale) for b, n in enumerate(lens)]
    return torch.cat([o for o, _ in parts]), torch.cat([l for _, l in parts])


def paged_rows(block_table, rows, page_size):
    """Pool row ids of a paged KV cache: logical row r of sequence b lives at pool row
    ``block_table[b, r >> lg] * page_size + (r & (page_size - 1))`` (page_size = 1 << lg).
    block_table int [B, NP]; rows int [T] (the same rows for every sequence) or [B, T], every one inside
    [0, NP * page_size). Returns int64 [B, T]."""
    lg = int(page_size).bit_length() - 1
    if page_size != 1 << lg:
        raise ValueError(f"paged_rows: page_size must be a power of two, got {page_size}")
    bt = block_table.long()
    r = torch.as_tensor(rows, device=bt.device).long()
    if r.dim() == 1:
        r = r[None].expand(bt.shape[0], -1)
    if not r.is_cuda and r.numel() and (int(r.min()) < 0 or int(r.max()) >= bt.shape[1] * page_size):  # no device sync
        raise IndexError(f"paged_rows: rows outside the table's [0, {bt.shape[1] * page_size})")
    return bt.gather(1, r >> lg) * page_size + (r & (page_size - 1))


def paged_gather(pool, block_table, n):
    """Rows [0, n) of every sequence of a paged KV pool, as the contiguous cache would hold them: pool
    [num_pages, page_size, Hkv, hd], block_table [B, NP] -> [B, n, Hkv, hd]. This is the definition of
    the paged layout (unreserved rows read the null page, page 0)."""
    P, ps = pool.shape[0], pool.shape[1]
    idx = paged_rows(block_table, torch.arange(n, device=pool.device), ps)
    return pool.reshape(P * ps, *pool.shape[2:])[idx]


def attention_paged(q, cache, n, kv_len=None, per_row=False, causal=True, scale=None):
    """Decode attention over a paged cache layer (``cache.k`` / ``cache.v`` pools, ``cache.block_table``;
    csrc/kernels/decode.hip attn_decode_paged): :func:`attention` / :func:`attention_per_row` on
    :func:`paged_gather` of rows [0, n). Returns (out, lse)."""
    k = paged_gather(cache.k, cache.block_table, n)
    v = paged_gather(cache.v, cache.block_table, n)
    if per_row:
        return attention_per_row(q, k, v, kv_len, causal, scale)
    if kv_len is not None:
        n = min(int(torch.as_tensor(kv_len).reshape(-1)[0]), n)
    return attention(q, k[:, :n], v[:, :n], causal, scale)


def rope_kv_write(x4, cos, sin, positions, index, cache, n_heads, n_kv_heads, mode=0, per_row=False):
    """Decode-step prologue (csrc/kernels/rope.hip rope_kv_write_ / rope_kv_write_q8_) on a packed qkv
    buffer x4 [B, T, H + 2 Hkv, hd]: RoPE at ``positions`` [B, T] on the q heads (in place) and on
    the k heads (mode 0 interleaved, 1 rotate_half); k / v rows into ``cache`` at row index + t
    (``per_row``: index[b] + t). ``cache`` is a (kc, vc) pair [B, Tmax, Hkv, hd] or a KV8-like object
    (kq / ks / vq / vs), which stores :func:`quant_kv8` of the value the pair would hold. Rows
    outside [0, Tmax) are dropped. A paged layer (``k`` / ``v`` pools and ``block_table``;
    rope_kv_write_paged_) takes the same rows through :func:`paged_rows`, Tmax being the table's
    NP * page_size."""
    if hasattr(cache, "block_table"):
        return _rope_kv_write_paged(x4, cos, sin, positions, index, cache, n_heads, n_kv_heads, mode, per_row)
    B, T = x4.shape[0], x4.shape[1]
    H, KV = n_heads, n_kv_heads
    pos = positions.reshape(B, T)
    x4[:, :, :H] = rope(x4[:, :, :H], cos, sin, interleaved=mode == 0, positions=pos)
    k = rope(x4[:, :, H:H + KV], cos, sin, interleaved=mode == 0, positions=pos)
    v = x4[:, :, H + KV:]
    idx = [int(i) for i in index.reshape(-1).tolist()]
    if per_row and len(idx) != B:
        raise ValueError(f"rope_kv_write: per_row needs {B} indices, got {len(idx)}")
    rows = idx if per_row else [idx[0]] * B
    fp8 = hasattr(cache, "kq")
    if fp8:
        (kq, ks), (vq, vs) = quant_kv8(k), quant_kv8(v)
        Tmax = cache.kq.shape[1]
    else:
        Tmax = cache[0].shape[1]
    for b in range(B):
        for t in range(T):
            r = rows[b] + t
            if not 0 <= r < Tmax:
                continue
            if fp8:
                cache.kq.view(torch.uint8)[b, r] = kq.view(torch.uint8)[b, t]
                cache.vq.view(torch.uint8)[b, r] = vq.view(torch.uint8)[b, t]
                cache.ks[b, :, r] = ks[b, :, t]
                cache.vs[b, :, r] = vs[b, :, t]
            else:
                cache[0][b, r] = k[b, t]
                cache[1][b, r] = v[b, t]


def _rope_kv_write_paged(x4, cos, sin, positions, index, cache, n_heads, n_kv_heads, mode, per_row):
    """:func:`rope_kv_write` into a paged layer: the same rotation, each kept row through
    :func:`paged_rows` into the flattened pools."""
    B, T = x4.shape[0], x4.shape[1]
    H, KV = n_heads, n_kv_heads
    pos = positions.reshape(B, T)
    x4[:, :, :H] = rope(x4[:, :, :H], cos, sin, interleaved=mode == 0, positions=pos)
    k = rope(x4[:, :, H:H + KV], cos, sin, interleaved=mode == 0, positions=pos)
    v = x4[:, :, H + KV:]
    idx = [int(i) for i in index.reshape(-1).tolist()]
    if per_row and len(idx) != B:
        raise ValueError(f"rope_kv_write: per_row needs {B} indices, got {len(idx)}")
    rows = idx if per_row else [idx[0]] * B
    ps = cache.k.shape[1]
    Tmax = cache.block_table.shape[1] * ps
    kf, vf = cache.k.view(-1, *cache.k.shape[2:]), cache.v.view(-1, *cache.v.shape[2:])
    for b in range(B):
        for t in range(T):
            r = rows[b] + t
            if not 0 <= r < Tmax:    # dropped before the table is read
                continue
            pr = int(paged_rows(cache.block_table[b:b + 1], [r], ps)[0, 0])
            kf[pr] = k[b, t]
            vf[pr] = v[b, t]


def gather_rows(x, idx):
    """x [B, T, D], idx int64 [B] -> [B, 1, D]: row idx[b] of each batch (csrc/kernels/layout.hip)."""
    return x[torch.arange(x.shape[0], device=x.device), idx][:, None]


def sample_probs(logits, temperature=1.0, top_k=None, top_p=None):
    """Unnormalised fp64 sampling weights [B, V] in vocabulary order (0 for dropped tokens): the
    distribution csrc/kernels/sample.hip draws from. Order: raw logit descending, ties by ascending
    token index (stable sort); top-k keeps the first k of that order (None, 0 or >= V: off); top-p
    keeps a token iff the softmax(logit / T) mass -- renormalised on what top-k kept -- strictly
    before it in the order is <= top_p (None or >= 1: off), so the first token always stays: today's
    infer.sampling._nucleus on today's sample() path. -inf has weight 0."""
    x = logits.detach().double()
    V = x.shape[-1]
    T = max(float(temperature), 1e-6)
    xs, idx = torch.sort(x, dim=-1, descending=True, stable=True)
    e = torch.exp((xs - xs[:, :1]) / T)
    if top_k is not None and 1 <= int(top_k) < V:
        e[:, int(top_k):] = 0.0
    if top_p is not None and float(top_p) < 1.0:
        p = e / e.sum(-1, keepdim=True)
        before = p.cumsum(-1) - p
        e = torch.where(before <= float(top_p), e, torch.zeros_like(e))
    return torch.zeros_like(e).scatter_(1, idx, e)


def sample_logits(logits, temperature=1.0, top_k=None, top_p=None, u=None):
    """logits [B, V], u [B] in (0, 1] -> token ids [B, 1] (int64): with P = sample_probs(...), C its
    inclusive prefix sum in vocabulary order and Z = C[:, -1], the smallest i with C[i] >= u * Z.
    fp64 throughout. u carries 24 bits (ops.sampling.u01), so a token with less than 2^-24 of the kept
    mass may never be drawn. Rows holding NaN, or nothing finite, are unspecified."""
    C = sample_probs(logits, temperature, top_k, top_p).cumsum(-1)
    target = u.detach().double().reshape(-1, 1) * C[:, -1:]
    return (C < target).sum(-1, keepdim=True).clamp_(max=C.shape[-1] - 1)
