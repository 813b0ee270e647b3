"""Graph decode with per-sequence positions against the uniform state, at equal lengths, in one process.

usage: python tools/bench_ragged_decode.py [--model llama3_8b] [--batches 4,16] [--prompt 1024] [--new 128]
                                           [--kv-caches bf16,fp8] [--rounds 3] [--layers N]

One model, and per (batch, cache format) two GraphDecoders: ``uniform`` (GraphDecoder(...), one position
for the batch) and ``ragged`` (GraphDecoder(..., ragged=True) fed ``prompt_lens`` all equal to the prompt
length, so both arms do the same work). Arms alternate uniform ragged ragged uniform per round; every run
is a full ``generate`` (eager prefill + ``new`` - 1 replays) timed by GenerationStats with device
synchronises; reported: the median ms per token of each arm, min / max, and ragged / uniform. One JSON line
per (batch, cache format)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench.decode import build  # noqa: E402
from solvingpapers_amd.infer import GenerationStats, GraphDecoder  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3_8b")
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--prompt", type=int, default=1024)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--kv-caches", default="bf16,fp8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=None)
    a = ap.parse_args()
    m = build(a.model, a.layers).eval()
    for B in (int(b) for b in a.batches.split(",")):
        ids = torch.randint(0, m.c.vocab_size, (B, a.prompt), device="cuda",
                            generator=torch.Generator(device="cuda").manual_seed(0))
        lens = [a.prompt] * B
        for kv in a.kv_caches.split(","):
            ckw = {} if kv == "bf16" else {"kv_cache": kv}
            arms = {"uniform": (GraphDecoder(m, B, a.prompt + a.new, **ckw), {}),
                    "ragged": (GraphDecoder(m, B, a.prompt + a.new, ragged=True, **ckw), {"prompt_lens": lens})}
            outs = {}
            for name, (dec, kw) in arms.items():          # warm-up; greedy tokens of the two arms must agree
                outs[name] = dec.generate(ids, 8, **kw)
            same = bool(torch.equal(outs["uniform"], outs["ragged"]))
            ms = {name: [] for name in arms}
            for _ in range(a.rounds):
                for name in ("uniform", "ragged", "ragged", "uniform"):
                    dec, kw = arms[name]
                    st = GenerationStats()
                    dec.generate(ids, a.new, stats=st, **kw)
                    ms[name].append(1e3 * st.decode_s / max(1, st.new_tokens // B))
            med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
            print(json.dumps({"model": a.model, "batch": B, "prompt": a.prompt, "new": a.new, "kv_cache": kv,
                              "uniform_ms_per_token": round(med["uniform"], 4),
                              "ragged_ms_per_token": round(med["ragged"], 4),
                              "ragged_vs_uniform": round(med["ragged"] / med["uniform"], 4),
                              "min_ms": {n: round(min(v), 4) for n, v in ms.items()},
                              "max_ms": {n: round(max(v), 4) for n, v in ms.items()},
                              "same_tokens": same}), flush=True)
            del arms


if __name__ == "__main__":
    main()
