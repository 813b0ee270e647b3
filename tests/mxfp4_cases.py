"""Inputs and an independent oracle for the MXFP4 quantisation rule, shared by
tests/test_quant_w4_cpu.py (ops/reference.py quant_mxfp4) and tests/test_gemv_w4_gpu.py (the HIP
quantizer): bf16 matrices [rows, K] whose 1 x 32 blocks exercise the rule's corners, and a brute-force
fp64 quantizer that shares no code with either implementation."""
import functools

import torch

E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


@functools.lru_cache(maxsize=None)
def rule_cases():
    """name -> bf16 [rows, K] on the CPU (cached: built once, never modified)"""
    g = torch.Generator().manual_seed(0)
    out = {}
    # randn with a different power-of-two magnitude per 1 x 32 block, 2^-40 .. 2^40
    e = torch.randint(-40, 41, (24, 8, 1), generator=g).float()
    out["randn_pow2"] = (torch.randn(24, 8, 32, generator=g) * torch.exp2(e)).view(24, 256).to(torch.bfloat16)
    # the seven tie points at several scales, both signs; a 6 pins the block's scale at 2^e
    scales = [-126, -20, -1, 0, 3, 17, 100, 125]
    t = torch.zeros(len(scales), 32, dtype=torch.float64)
    t[:, :7] = torch.tensor(TIES, dtype=torch.float64)
    t[:, 7] = 6.0
    t[:, 8:15] = -torch.tensor(TIES, dtype=torch.float64)
    out["ties"] = (t * torch.exp2(torch.tensor(scales, dtype=torch.float64))[:, None]).to(torch.bfloat16)
    z = torch.zeros(2, 32, dtype=torch.bfloat16)
    z[1, 0] = z[1, 3] = -0.0
    out["zeros_and_negative_zero"] = z
    # amax exactly 6 * 2^e, and one bf16 ulp (2^-5 at 6) above; element 1 stays zero
    body = (torch.randn(6, 32, generator=g) * 1.5).clamp(-5.5, 5.5)
    body[:, 0], body[:, 1] = 6.0, 0.0
    pw = torch.exp2(torch.tensor([-30.0, -3, 0, 1, 9, 60]))[:, None]
    out["amax_6"] = (body * pw).to(torch.bfloat16)
    body = body.clone()
    body[:, 0] = 6.0 + 2.0 ** -5
    out["amax_6_plus_ulp"] = (body * pw).to(torch.bfloat16)
    # the clamps: a block of bf16 subnormals (e = -126) and one at the top of the range (e = 125, saturating)
    edge = torch.zeros(2, 32, dtype=torch.float64)
    edge[0, :4] = torch.tensor([1.0, -3.0, 64.0, 127.0]) * 2.0 ** -133
    edge[1, :6] = torch.tensor([1.0, -0.75, 0.5, 0.1, -0.02, 0.3]) * (2.0 ** 127 * 1.9921875)
    out["clamps"] = edge.to(torch.bfloat16)
    for w in out.values():
        assert torch.isfinite(w.float()).all()
    return out


def brute_force_mxfp4(W):
    """(wq, s) of bf16 W [rows, K] by definition, in fp64 and python integers: per block the smallest e
    with amax <= 6 * 2^e by search, clamped to [-126, 125], 0 for a zero block; per element the nearest of
    the eight magnitudes to min(|w| / 2^e, 6), a tie to the even code; the sign bit of the value itself."""
    Wd = W.double()
    rows, K = Wd.shape
    wq = torch.zeros(rows, K // 2, dtype=torch.uint8)
    s = torch.zeros(rows, K // 32, dtype=torch.uint8)
    sign = torch.signbit(W)
    for r in range(rows):
        for b in range(K // 32):
            blk = Wd[r, 32 * b:32 * b + 32].tolist()
            amax = max(abs(v) for v in blk)
            e = 0
            if amax > 0:
                e = -160
                while amax > 6.0 * 2.0 ** e:
                    e += 1
                e = max(-126, min(125, e))
            s[r, b] = e + 127
            codes = []
            for j, v in enumerate(blk):
                a = min(abs(v) / 2.0 ** e, 6.0)              # exact: a power-of-two quotient in fp64
                best = min(range(8), key=lambda c: (abs(E2M1[c] - a), c % 2))
                codes.append(best | (8 if sign[r, 32 * b + j] else 0))
            for j in range(16):
                wq[r, 16 * b + j] = codes[2 * j] | codes[2 * j + 1] << 4
    return wq, s
