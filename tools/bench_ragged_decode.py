"""Graph decode with per-sequence positions against the uniform state, at equal lengths, in one process.

usage: python tools/bench_ragged_decode.py [--model llama3_8b] [--batches 4,16] [--prompt 1024] [--new 128]
                                           [--kv-caches bf16,fp8] [--rounds 3] [--layers N]
                                           [--paged [--page-sizes 16,64]]

One model, and per (batch, cache format) two GraphDecoders: ``uniform`` (GraphDecoder(...), one position
for the batch) and ``ragged`` (GraphDecoder(..., ragged=True) fed ``prompt_lens`` all equal to the prompt
length, so both arms do the same work). Arms alternate uniform ragged ragged uniform per round; every run
is a full ``generate`` (eager prefill + ``new`` - 1 replays) timed by GenerationStats with device
synchronises; reported: the median ms per token of each arm, min / max, and ragged / uniform. One JSON line
per (batch, cache format).

``--paged`` adds the paged-cache rows (bf16 cache only): GraphDecoder(ragged=True, page_size=N) against the
contiguous ragged decoder, ``--page-sizes 16,64``, at equal prompt lengths and at lengths spread evenly
from prompt / 4 to prompt (1:4), arms alternated contiguous paged paged contiguous. In the spread case
``num_pages`` is sized to the pages the lengths need (len_b + new rows each, plus the null page): the
memory paging saves, reported as ``cache_GB`` of both arms. One JSON line per (batch, lengths, page size)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench.decode import build  # noqa: E402
from solvingpapers_amd.infer import GenerationStats, GraphDecoder  # noqa: E402


def paged_rows(m, a):
    for B in (int(b) for b in a.batches.split(",")):
        ids = torch.randint(0, m.c.vocab_size, (B, a.prompt), device="cuda",
                            generator=torch.Generator(device="cuda").manual_seed(0))
        cases = {"equal": [a.prompt] * B,
                 "spread": torch.linspace(a.prompt / 4, a.prompt, B).round().int().tolist()}
        for case, lens in cases.items():
            for ps in (int(p) for p in a.page_sizes.split(",")):
                need = sum(-(-(n + a.new) // ps) for n in lens) + 1     # the pages the lengths need + the null page
                arms = {"contiguous": GraphDecoder(m, B, a.prompt + a.new, ragged=True),
                        "paged": GraphDecoder(m, B, a.prompt + a.new, ragged=True, page_size=ps, num_pages=need)}
                outs = {n: d.generate(ids, 8, prompt_lens=lens) for n, d in arms.items()}   # warm-up
                same = bool(torch.equal(outs["contiguous"], outs["paged"]))
                ms = {n: [] for n in arms}
                for _ in range(a.rounds):
                    for name in ("contiguous", "paged", "paged", "contiguous"):
                        st = GenerationStats()
                        arms[name].generate(ids, a.new, stats=st, prompt_lens=lens)
                        ms[name].append(1e3 * st.decode_s / max(1, st.new_tokens // B))
                med = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
                print(json.dumps({"model": a.model, "batch": B, "prompt": a.prompt, "new": a.new, "lens": case,
                                  "page_size": ps, "num_pages": need,
                                  "contiguous_ms_per_token": round(med["contiguous"], 4),
                                  "paged_ms_per_token": round(med["paged"], 4),
                                  "paged_vs_contiguous": round(med["paged"] / med["contiguous"], 4),
                                  "cache_GB": {n: round(d.cache.nbytes() / 1e9, 4) for n, d in arms.items()},
                                  "min_ms": {n: round(min(v), 4) for n, v in ms.items()},
                                  "max_ms": {n: round(max(v), 4) for n, v in ms.items()},
                                  "same_tokens": same}), flush=True)
                del arms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3_8b")
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--prompt", type=int, default=1024)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--kv-caches", default="bf16,fp8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--paged", action="store_true", help="paged-cache rows instead of the uniform / ragged ones")
    ap.add_argument("--page-sizes", default="16,64")
    a = ap.parse_args()
    m = build(a.model, a.layers).eval()
    if a.paged:
        return paged_rows(m, a)
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
