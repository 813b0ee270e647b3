"""Fused sampler, CPU side: the fp64 oracle (ops.reference.sample_probs / sample_logits) against
today's infer.sample() distribution, the tie rules, the host twin of the device RNG, Sampler
determinism and sampled generation; the chi-square body that tests/test_sampling_gpu.py reruns on
the device."""
import numpy as np
import pytest
import torch

from sampling_common import CHI2_SEEDS, chi2_check, chi2_draws

from solvingpapers_amd.infer import Sampler, generate
from solvingpapers_amd.infer.sampling import _nucleus
from solvingpapers_amd.models import gpt, llama3
from solvingpapers_amd.ops import reference as R
from solvingpapers_amd.ops import sample_logits
from solvingpapers_amd.ops.sampling import mix32, u01


def _todays_probs(logits, temperature, top_k, top_p):
    """The distribution infer.sample() draws from (same torch calls, up to its multinomial), laid
    out in vocabulary order."""
    lg = logits.float() / max(temperature, 1e-6)
    if top_k is not None:
        v, ix = torch.topk(lg, min(int(top_k), lg.shape[-1]), dim=-1)
        if top_p is not None:
            v = _nucleus(v, top_p)
        return torch.zeros_like(lg).scatter_(1, ix, torch.softmax(v, -1))
    if top_p is not None:
        v, ix = torch.sort(lg, dim=-1, descending=True)
        return torch.zeros_like(lg).scatter_(1, ix, torch.softmax(_nucleus(v, top_p), -1))
    return torch.softmax(lg, -1)


CASES = [(1.0, None, None), (0.7, None, None), (1.0, 3, None), (0.8, 50, None), (1.0, None, 0.9), (1.3, None, 0.5),
         (0.8, 50, 0.9), (1.0, 4, 0.6), (1.0, 1, None), (1.0, None, 1e-6), (1.0, 5000, None), (0.9, 5000, 0.95)]


@pytest.mark.parametrize("V", [5, 257, 1000, 4099])
def test_oracle_matches_todays_sample_distribution(V):
    g = torch.Generator().manual_seed(V)
    # tie-free by construction: the V normal quantiles, shuffled per row (randn repeats values at V = 4099)
    perm = torch.stack([torch.randperm(V, generator=g) for _ in range(3)])
    lg = (torch.erfinv(2 * (perm.double() + 0.5) / V - 1) * 2 ** 0.5 * 2).float()
    assert all(len(torch.unique(r)) == V for r in lg), "the comparison needs tie-free rows"
    for T, k, p in CASES:
        want = _todays_probs(lg, T, k, p).double()
        got = R.sample_probs(lg, T, k, p)
        got = got / got.sum(-1, keepdim=True)
        assert torch.equal(got > 0, want > 0), (V, T, k, p)
        assert (got - want).abs().max() < 1e-6, (V, T, k, p)


def test_ties_keep_the_lowest_indices():
    #                 0    1    2    3    4    5    6    7    8
    lg = torch.tensor([[1.0, 3.0, 2.0, 2.0, 2.0, 2.0, 0.0, 2.0, -1.0]])
    kept = lambda **kw: torch.nonzero(R.sample_probs(lg, 1.0, **kw)[0]).flatten().tolist()  # noqa: E731
    assert kept(top_k=3) == [1, 2, 3]            # the 3, then the first two of the five 2s
    assert kept(top_k=1) == [1]
    assert kept(top_k=6) == [1, 2, 3, 4, 5, 7]
    # mass before the t-th 2 is (1 + t / e) / 3.0428 = .329, .450, .570, .691, .812
    assert kept(top_p=0.5) == [1, 2, 3]
    assert kept(top_p=0.7) == [1, 2, 3, 4, 5]
    # top-4 = {3, 2, 2, 2}, renormalised: mass before the t-th 2 is (1 + t / e) / 2.1036 = .475, .650, .825
    assert kept(top_k=4, top_p=0.6) == [1, 2]
    assert kept(top_k=4, top_p=0.7) == [1, 2, 3]
    assert kept(top_k=4, top_p=0.9) == [1, 2, 3, 4]
    # -0.0 and 0.0 are one value: index order decides
    z = torch.tensor([[0.0, -0.0, 0.0, -0.0]])
    assert torch.nonzero(R.sample_probs(z, 1.0, top_k=2)[0]).flatten().tolist() == [0, 1]


def test_draw_is_the_prefix_sum_inverse_in_vocabulary_order():
    lg = torch.log(torch.tensor([[0.1, 0.2, 0.3, 0.4], [0.4, 0.3, 0.2, 0.1]]))
    pick = lambda u: R.sample_logits(lg, 1.0, None, None, torch.tensor(u))[:, 0].tolist()  # noqa: E731
    assert pick([0.05, 0.05]) == [0, 0]
    assert pick([0.25, 0.45]) == [1, 1]
    assert pick([0.65, 0.95]) == [3, 3]
    assert pick([1.0, 1.0]) == [3, 3]
    inf = torch.tensor([[float("-inf"), 0.0, float("-inf"), 0.0]])
    assert R.sample_logits(inf, 1.0, None, None, torch.tensor([2.0 ** -24])).item() == 1   # never an -inf entry
    assert R.sample_logits(inf, 1.0, None, None, torch.tensor([1.0])).item() == 3
    assert R.sample_logits(inf, 1.0, 3, None, torch.tensor([1.0])).item() == 3             # top-3 holds one -inf


def test_host_u01_twin():
    assert mix32(0) == 0 and u01(0, 0) == 2.0 ** -24
    assert u01(0, 1) == 0.20609736442565918
    assert u01(1234, 7) == 0.7595095038414001
    assert u01(-1, 5) == 0.5884808301925659

    def np_u01(seed, i):   # the same three multiply-xor rounds in wrapping uint64 arithmetic
        with np.errstate(over="ignore"):
            k = np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(i)
            k ^= k >> np.uint64(33)
            k *= np.uint64(0xff51afd7ed558ccd)
            k ^= k >> np.uint64(33)
            k *= np.uint64(0xc4ceb9fe1a85ec53)
            k ^= k >> np.uint64(33)
        return float(np.float32((int(k) & 0xFFFFFFFF) >> 8) + np.float32(1)) * float(np.float32(1 / 16777216))

    us = [u01(s, i) for s in (0, 5, 2 ** 40 + 3) for i in range(2000)]
    assert min(us) > 0.0 and max(us) <= 1.0
    assert all(u * 2 ** 24 == int(u * 2 ** 24) for u in us)         # 24-bit values: exact in fp32
    assert abs(sum(us) / len(us) - 0.5) < 0.02
    for s, i in ((0, 1), (5, 77), (2 ** 40 + 3, 123456789)):
        assert u01(s, i) == np_u01(s, i)


def test_sampler_is_deterministic_and_counts_calls():
    lg = torch.randn(4, 300, generator=torch.Generator().manual_seed(1))
    s = Sampler(0.8, 20, 0.9, seed=11)
    a = torch.cat([s(lg) for _ in range(6)], 1)
    assert a.shape == (4, 6) and a.dtype == torch.long and int(s.offset.item()) == 6
    b = torch.cat([Sampler(0.8, 20, 0.9, seed=11)(lg) for _ in range(1)], 1)
    assert torch.equal(a[:, :1], b)
    s.reseed(11)
    assert int(s.offset.item()) == 0
    assert torch.equal(torch.cat([s(lg) for _ in range(6)], 1), a)
    s.reseed(11, offset=3)
    assert torch.equal(s(lg), a[:, 3:4])
    assert not torch.equal(torch.cat([Sampler(0.8, 20, 0.9, seed=12)(lg) for _ in range(6)], 1), a)
    # row b of call n draws with u01(seed, n * B + b)
    u = torch.tensor([u01(11, 2 * 4 + b) for b in range(4)])
    assert torch.equal(R.sample_logits(lg, 0.8, 20, 0.9, u), a[:, 2:3])
    out = torch.zeros(4, 1, dtype=torch.long)
    s.reseed(11)
    assert s(lg, out=out) is out and torch.equal(out, a[:, :1])


def test_sample_logits_argument_checks():
    lg = torch.randn(2, 9)
    u = torch.full((2,), 0.5)
    seed, off = torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    for kw in ({}, {"u": u, "seed": seed, "offset": off}, {"seed": seed}, {"u": u, "offset": off}):
        with pytest.raises(ValueError):
            sample_logits(lg, **kw)
    with pytest.raises(ValueError):
        sample_logits(lg, top_p=0.0, u=u)
    with pytest.raises(ValueError):
        Sampler(top_p=0.0)
    assert sample_logits(lg, top_k=1, u=u).flatten().tolist() == lg.argmax(-1).tolist()


def test_generate_with_sampler_matches_hand_rolled_loop():
    torch.manual_seed(0)
    m = llama3.Llama3(llama3.config("llama3_tiny", vocab_size=128, dim=64, n_heads=4, n_kv_heads=2,
                                    ffn_hidden=128, max_seq_len=64)).eval()
    ids = torch.randint(0, 120, (2, 5))
    n, B = 9, 2
    out = generate(m, ids, n, sampler=Sampler(0.9, 12, 0.95, seed=3))
    assert torch.equal(out, m.generate(ids, n, sampler=Sampler(0.9, 12, 0.95, seed=3)))
    ref = ids
    with torch.no_grad():
        cache = m.new_cache(B, ids.shape[1] + n)
        lg = m.step(ids, cache, 0)
        for t in range(n):
            u = torch.tensor([u01(3, t * B + b) for b in range(B)])
            nxt = R.sample_logits(lg, 0.9, 12, 0.95, u)
            ref = torch.cat([ref, nxt], 1)
            if t + 1 < n:
                lg = m.step(nxt, cache, ids.shape[1] + t)
    assert torch.equal(out, ref)
    # EOS handling is unchanged: finished rows keep emitting eos
    eos = int(out[0, 7])
    o2 = generate(m, ids, n, eos_token_id=eos, sampler=Sampler(0.9, 12, 0.95, seed=3))
    assert torch.equal(o2[0, :8], out[0, :8]) and bool((o2[0, 8:] == eos).all())


def test_reforward_loop_takes_the_sampler():
    torch.manual_seed(0)
    m = gpt.GPT(gpt.config("gpt_tiny_cpu", block_size=8)).eval()
    ids = torch.randint(0, 60, (2, 3))
    out = m.generate(ids, 10, sampler=Sampler(1.0, 5, None, seed=2))     # 5 cached tokens, 5 re-forwarded
    ref = ids
    with torch.no_grad():
        for t in range(10):
            lg = m(ref[:, -8:])[:, -1].float()
            ref = torch.cat([ref, R.sample_logits(lg, 1.0, 5, None, torch.tensor([u01(2, t * 2 + b) for b in range(2)]))], 1)
    assert out.shape == (2, 13)
    assert torch.equal(out, ref)


@pytest.mark.parametrize("seed", CHI2_SEEDS)
def test_chi_square_of_the_draws(seed):
    chi2_check(chi2_draws(seed, "cpu"))
