"""Fused sampler on the device (csrc/kernels/sample.hip): the kernel against the fp64 oracle with
constructed uniforms, the seeded stream against the CPU path draw for draw, and the sampler captured
in the decode graph."""
import pytest
import torch

from sampling_common import (CHI2_K, CHI2_P, CHI2_SEEDS, CHI2_T, EDGE, KERNEL_SHAPES, chi2_check, chi2_draws, chi2_row,
                             chi2_uniforms, edge_distance, kernel_cases, kernel_targets, top_p_margin)

from solvingpapers_amd.infer import GraphDecoder, Sampler
from solvingpapers_amd.ops import reference as R
from solvingpapers_amd.ops import sample_logits
from solvingpapers_amd.ops.sampling import u01

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("V,B", KERNEL_SHAPES)
def test_kernel_matches_oracle_on_constructed_uniforms(V, B):
    """u is the midpoint of the target token's interval of C / Z (targets hold >= 1e-3 of the mass), so
    fp32 against fp64 sums cannot move the draw: the id must be EQUAL. Shapes: a vector tail (odd V,
    rows off the 16-byte grid for B > 1), V below one workgroup and below one wave, ties across lane,
    wave and tile boundaries, 128256 for the long row."""
    bad = []
    for name, lg, T, k, p in kernel_cases(B, V):
        if p is not None:
            mg = top_p_margin(lg, T, k, p)
            assert mg > 1e-4, (name, mg)
        tg, us = kernel_targets(R.sample_probs(lg, T, k, p))
        for dt in (torch.float32, torch.bfloat16):
            x = lg.to(DEV, dt)
            assert torch.equal(x.float().cpu(), lg)          # bf16-rounded values: both dtypes hold the same row
            got = torch.stack([sample_logits(x, T, k, p, u=u.to(DEV))[:, 0] for u in us]).cpu()
            if not torch.equal(got, tg):
                bad.append((name, str(dt), got.tolist(), tg.tolist()))
    assert not bad, bad[:4]


@pytest.mark.parametrize("seed", CHI2_SEEDS)
def test_seeded_stream_matches_cpu_path(seed):
    ids = chi2_draws(seed, DEV)
    chi2_check(ids)
    ref = chi2_draws(seed, "cpu")
    P = R.sample_probs(chi2_row(), CHI2_T, CHI2_K, CHI2_P)
    near = edge_distance(P.expand(ids.numel(), -1), chi2_uniforms(seed).reshape(-1)).reshape(ids.shape) < EDGE
    print(f"seed {seed}: {int(near.sum())} of {ids.numel()} draws within {EDGE} of an edge, "
          f"{int((ids != ref).sum())} differ from the CPU path")
    assert near.float().mean() <= 0.01
    assert torch.equal(ids[~near], ref[~near])


def test_out_buffer_and_counters():
    lg = (torch.randn(5, 1003, generator=torch.Generator().manual_seed(3)) * 2).bfloat16().to(DEV)
    seed = torch.full((1,), 9, dtype=torch.long, device=DEV)
    off = torch.full((1,), 4, dtype=torch.long, device=DEV)
    out = torch.full((5, 1), -1, dtype=torch.long, device=DEV)
    r = sample_logits(lg, 0.9, 40, 0.9, seed=seed, offset=off, out=out)
    assert r.data_ptr() == out.data_ptr() and int(out.min()) >= 0 and int(off.item()) == 4   # the op leaves offset alone
    again = sample_logits(lg, 0.9, 40, 0.9, seed=seed, offset=off)
    assert again.shape == (5, 1) and again.dtype == torch.long and torch.equal(again, out)
    u = torch.tensor([u01(9, 4 * 5 + b) for b in range(5)], device=DEV)
    assert torch.equal(sample_logits(lg, 0.9, 40, 0.9, u=u), out)                            # the device draws u01 itself
    far = edge_distance(R.sample_probs(lg.cpu(), 0.9, 40, 0.9), u.cpu()) >= EDGE            # and the CPU path the same one
    assert torch.equal(sample_logits(lg.cpu(), 0.9, 40, 0.9, seed=seed.cpu(), offset=off.cpu())[far], out.cpu()[far])
    s = Sampler(0.9, 40, 0.9, seed=9, device=DEV).reseed(9, 4)
    assert torch.equal(s(lg), out) and int(s.offset.item()) == 5
    assert s(lg, out=out) is out and int(s.offset.item()) == 6
    # a view that starts off the 16-byte grid, and one row of a wider buffer
    wide = torch.zeros(3, 1003 + 5, device=DEV)
    wide[:, 5:] = lg[:3].float()
    row = wide[1, 5:].reshape(1, -1)
    assert row.data_ptr() % 16 != 0
    u1 = torch.tensor([0.37], device=DEV)
    assert torch.equal(sample_logits(row, 1.0, None, 0.9, u=u1), sample_logits(lg[1:2].float().clone(), 1.0, None, 0.9, u=u1))


def test_argument_checks():
    lg = torch.randn(2, 64, device=DEV)
    u = torch.full((2,), 0.5, device=DEV)
    ops = torch.ops.spa
    with pytest.raises(RuntimeError):
        ops.sample_logits(lg.half(), 1.0, 0, 1.0, u, None, None, None)
    with pytest.raises(RuntimeError):
        ops.sample_logits(lg.t(), 1.0, 0, 1.0, u, None, None, None)
    with pytest.raises(RuntimeError):
        ops.sample_logits(lg, 1.0, 0, 0.0, u, None, None, None)
    with pytest.raises(RuntimeError):
        ops.sample_logits(lg, 1.0, 0, 1.0, None, None, None, None)
    with pytest.raises(RuntimeError):
        ops.sample_logits(lg, 1.0, 0, 1.0, u.double(), None, None, None)
    with pytest.raises(RuntimeError):
        ops.sample_logits(lg, 1.0, 0, 1.0, u[:1], None, None, None)
    with pytest.raises(RuntimeError):
        ops.sample_logits(lg, 1.0, 0, 1.0, u, None, None, torch.zeros(2, 1, device=DEV))
    with pytest.raises(RuntimeError):
        ops.sample_logits(lg, 1.0, 0, 1.0, u.cpu(), None, None, None)


def _model(family):
    if family == "llama3":
        from solvingpapers_amd.models import llama3
        return llama3.Llama3(llama3.config("llama3_tiny"), device=DEV, dtype=torch.bfloat16).eval()
    from solvingpapers_amd.models import gemma
    m = gemma.Gemma(gemma.config("gemma_tiny"), device=DEV, dtype=torch.bfloat16).eval()
    # the tied head of a random-init model puts all the mass on the token just fed (its own embedding);
    # a smaller table flattens the logits so that the draws have something to choose from
    m.embed.data.mul_(0.25)
    return m


class _CountingGraph:
    def __init__(self, graph):
        self.graph, self.replays = graph, 0

    def replay(self):
        self.replays += 1
        self.graph.replay()


@pytest.mark.parametrize("family", ["llama3", "gemma"])
def test_captured_sampling(family, monkeypatch):
    torch.manual_seed(0)
    m = _model(family)
    B, T, K, P_, SEED, STEPS = 2, 0.8, 8, 0.95, 5, 16
    ids = torch.randint(0, m.c.vocab_size, (B, 6), device=DEV)
    with torch.no_grad():
        dec = GraphDecoder(m, B, 48, sampler=Sampler(T, K, P_, seed=SEED))
        assert int(dec.sampler.offset.item()) == 0          # the warm-up's offsets were given back
        # every replay's draw against the oracle on that replay's logits
        lg = dec.prefill(ids)
        dec.sampler(lg, out=dec.ids)
        exempt = spread = 0
        for i in range(STEPS):
            dec.graph.replay()
            off = i + 1
            assert int(dec.sampler.offset.item()) == off + 1
            lg, got = dec.logits.float().cpu(), dec.ids.cpu()
            Pr = R.sample_probs(lg, T, K, P_)
            u = torch.tensor([u01(SEED, off * B + b) for b in range(B)])
            want = R.sample_logits(lg, T, K, P_, u)
            near = edge_distance(Pr, u) < EDGE
            spread += int(((Pr / Pr.sum(-1, keepdim=True)).max(-1).values < 0.9).sum())
            for b in range(B):
                assert Pr[b, got[b, 0]] > 0, "a draw outside the kept set"
                if near[b]:
                    exempt += 1
                else:
                    assert got[b, 0] == want[b, 0], (i, b)
        assert exempt <= 1
        assert spread >= STEPS, "the test needs rows whose kept set is more than one likely token"
        # reproducible generation; per-call sampling arguments cannot apply to a captured sampler
        dec.sampler.reseed(SEED)
        a = dec.generate(ids, STEPS + 1)
        dec.sampler.reseed(SEED)
        assert torch.equal(dec.generate(ids, STEPS + 1), a)
        dec.sampler.reseed(SEED + 1)
        assert not torch.equal(dec.generate(ids, STEPS + 1), a)
        for kw in ({"temperature": 0.5}, {"top_k": 3}, {"top_p": 0.5}, {"generator": torch.Generator(device=DEV)}):
            with pytest.raises(ValueError):
                dec.generate(ids, 4, **kw)
        # host-free loop: n tokens are n - 1 replays and no eager sampling
        import solvingpapers_amd.infer.graph as G

        def boom(*a, **k):
            raise AssertionError("eager sample() called with a captured sampler")
        monkeypatch.setattr(G, "sample", boom)
        dec.graph = _CountingGraph(dec.graph)
        dec.sampler.reseed(SEED)
        assert torch.equal(dec.generate(ids, STEPS + 1), a)
        assert dec.graph.replays == STEPS


def test_eager_generate_with_sampler_on_device():
    """generate(..., sampler=) outside a graph: one fused launch per token, ids in the kept set."""
    torch.manual_seed(0)
    m = _model("llama3")
    ids = torch.randint(0, m.c.vocab_size, (2, 6), device=DEV)
    a = m.generate(ids, 8, sampler=Sampler(0.8, 8, 0.95, seed=5))
    b = m.generate(ids, 8, sampler=Sampler(0.8, 8, 0.95, seed=5))
    assert a.shape == (2, 14) and torch.equal(a, b)
