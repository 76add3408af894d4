#!/usr/bin/env python
"""Cost of seeded sampling in decode at the released geometry (32 layers, H 4096, vocab 51760, synthetic weights): ms per
decode step in three modes — greedy, temperature only (the Gumbel-max draw folded into the LM head's per-block argmax) and
top-k + top-p (greedy LM head, then the filter kernel k_dec_sample on the kept row) — measured in interleaved rounds on one
engine, plus the filter kernel alone (vh_sample_rows, one 51760-entry row per launch) timed with events.

  python profiles/bench_sampling.py [--steps 64] [--rounds 3] [--prompt 1024] [--out profiles/bench_sampling.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o filter -- \
      python profiles/bench_sampling.py --filter-only --filter-mode top_k+top_p     (the filter kernel alone; its kernel_stats.csv is
                                                                                     profiles/bench_sampling_rocprof_filter.csv)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vita_amd import ops  # noqa: E402

MODES = {"greedy": dict(), "temperature": dict(temperature=0.8, top_k=0, top_p=1.0, seed=1),
         "top_k+top_p": dict(temperature=0.8, top_k=50, top_p=0.9, seed=1)}


FILTERS = {"top_k+top_p": dict(top_k=50, top_p=0.9), "top_p": dict(top_p=0.9), "top_k": dict(top_k=50), "temperature": dict()}


def filter_kernel_us(V, iters, dev, only=None):
    """vh_sample_rows on one row ~N(0, 3^2), T 0.8: mean us per launch from events around `iters` back-to-back launches"""
    g = torch.Generator(device=dev).manual_seed(0)
    row = torch.randn(V, generator=g, device=dev) * 3
    out = {}
    for name, kw in FILTERS.items():
        if only and name != only:
            continue
        for _ in range(3):
            ops.sample_rows(row, rows=1, temperature=0.8, seed=1, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for d in range(iters):
            ops.sample_rows(row, rows=1, temperature=0.8, seed=1, draw0=d, **kw)
        e1.record()
        torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) * 1e3 / iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=1024)
    ap.add_argument("--filter-only", action="store_true", help="only the filter kernel (for a kernel trace)")
    ap.add_argument("--filter-mode", choices=sorted(FILTERS), default=None, help="with --filter-only: one filter setting")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"filter_kernel_event_us_V51760": filter_kernel_us(51760, 200, dev, args.filter_mode if args.filter_only else None)}
    if args.filter_only:
        print(json.dumps(res))
        return
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.config import VitaConfig
    from vita_amd.engine import MixtralEngine
    cfg = VitaConfig()
    t = cfg.text
    packed = synth_mixtral_device(cfg, dev, seed=0)
    n = args.steps + args.warmup + 2
    eng = MixtralEngine(cfg, packed, dev, max_prefill=args.prompt, max_ctx=args.prompt + n + 64, max_new=n)
    emb = packed["embed"][torch.randint(3, t.vocab_size, (args.prompt,), device=dev)].float()
    ms = {m: [] for m in MODES}
    for r in range(args.rounds):
        for m, kw in MODES.items():
            eng.set_sampling(**kw)
            eng.prefill(emb)
            eng.decode(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.decode(args.steps)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) * 1e3 / args.steps)
            eng.check_device_flag()
    eng.set_sampling()
    med = {m: float(np.median(v)) for m, v in ms.items()}
    res.update({"decode_ms_per_step": med, "all_rounds": ms,
                "overhead_pct": {m: 100.0 * (med[m] / med["greedy"] - 1.0) for m in MODES if m != "greedy"},
                "geometry": f"{t.num_hidden_layers} layers, H {t.hidden_size}, vocab {t.vocab_size}, prompt {args.prompt}, "
                            f"{args.steps} timed steps after {args.warmup}, median of {args.rounds} interleaved rounds"})
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
