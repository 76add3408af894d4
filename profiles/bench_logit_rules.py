#!/usr/bin/env python
"""Cost of the logit rules (penalties, log-probabilities: DESIGN 5.6) in decode at the released geometry (32 layers, H 4096, vocab
51760, synthetic weights): ms per decode step of one engine in interleaved rounds —

  greedy            no rules (the kernels of an engine created without tables)
  temperature       seeded temperature-only sampling, the yardstick of 5.4 for "one more operand in the LM head's compare"
  penalties         greedy + repetition / frequency / presence penalties (the PEN LM head, the counting select)
  logprobs5 / 20    greedy + k_dec_logprobs with K = 5 / 20
  all               penalties + top-k / top-p (the filter kernel applies the penalties on load) + logprobs = 20

then one batched leg (8 sequences in one iteration, plain against mixed settings) on a paged engine over the same weights, and the
logprob kernel alone (vh_logit_rules_rows, one 51760-entry row per launch) next to the filter kernel, timed with events.

  python profiles/bench_logit_rules.py [--steps 64] [--rounds 3] [--prompt 1024] [--out profiles/bench_logit_rules.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o rules -- python profiles/bench_logit_rules.py --kernels-only

--out holds exactly what this script measures.  Figures taken another way in the same GPU visit (bench.py of the parent commit in
alternating processes, the kernel trace, the top-K variant that was measured and not kept) are in profiles/bench_logit_rules_notes.json.
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

PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.6)
TOPKP = dict(temperature=0.8, top_k=50, top_p=0.9, seed=1)
LEGS = {"greedy": (dict(), None), "temperature": (dict(temperature=0.8, top_k=0, top_p=1.0, seed=1), None),
        "penalties": (dict(), dict(PEN)), "logprobs5": (dict(), dict(logprobs=5)), "logprobs20": (dict(), dict(logprobs=20)),
        "all": (TOPKP, dict(PEN, logprobs=20))}


def kernel_us(V, iters, dev):
    """event time per launch of the logprob kernel (K = 0 / 5 / 20) and of the filter kernel on one row ~N(0, 3^2)"""
    g = torch.Generator(device=dev).manual_seed(0)
    row = (torch.randn(V, generator=g, device=dev) * 3)[None].contiguous()
    tok = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {}

    def timed(name, fn):
        for _ in range(3):
            fn(0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for d in range(iters):
            fn(d)
        e1.record()
        torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) * 1e3 / iters

    for K in (0, 5, 20):
        timed(f"logprobs_K{K}", lambda d, K=K: ops.logit_rules_rows(row, None, tokens=tok, logprobs=K, want_penalised=False))
    timed("filter_top_k+top_p", lambda d: ops.sample_rows(row[0], rows=1, temperature=0.8, seed=1, draw0=d, top_k=50, top_p=0.9))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--prompt", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kernels-only", action="store_true", help="only the row kernels (for a kernel trace)")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"row_kernel_event_us_V51760": kernel_us(51760, 200, dev)}
    if args.kernels_only:
        print(json.dumps(res))
        return
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.config import VitaConfig
    from vita_amd.engine import MixtralEngine
    cfg = VitaConfig()
    t = cfg.text
    packed = synth_mixtral_device(cfg, dev, seed=0)
    n = args.steps + args.warmup + 2
    eng = MixtralEngine(cfg, packed, dev, max_prefill=args.prompt, max_ctx=args.prompt + n + 64, max_new=n, penalty_tables=True,
                        max_logprobs=20)
    pid = torch.randint(3, t.vocab_size, (args.prompt,), device=dev)
    emb = packed["embed"][pid].float()
    prompt_ids = pid.tolist()
    ms = {m: [] for m in LEGS}
    for r in range(args.rounds):
        for m, (samp, rules) in LEGS.items():
            eng.set_sampling(**samp)
            if rules is None:
                eng.set_logit_rules()
            else:
                eng.set_logit_rules(prompt_ids=prompt_ids, **rules)
            eng.prefill(emb)
            eng.decode(args.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.decode(args.steps)
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) * 1e3 / args.steps)
            eng.check_device_flag()
    # the setter with penalties waits for the device and uploads the table with a blocking copy: host time per call on an idle engine
    t0 = time.perf_counter()
    for _ in range(20):
        eng.set_logit_rules(prompt_ids=prompt_ids, **PEN)
    setter_ms = (time.perf_counter() - t0) * 1e3 / 20
    eng.set_logit_rules()
    eng.close()
    med = {m: float(np.median(v)) for m, v in ms.items()}
    res.update({"decode_ms_per_step": med, "all_rounds": ms, "setter_with_penalties_host_ms_per_call_idle_engine": setter_ms,
                "overhead_pct": {m: 100.0 * (med[m] / med["greedy"] - 1.0) for m in LEGS if m != "greedy"},
                "geometry": f"{t.num_hidden_layers} layers, H {t.hidden_size}, vocab {t.vocab_size}, prompt {args.prompt}, "
                            f"{args.steps} timed steps after {args.warmup}, median of {args.rounds} interleaved rounds"})
    # ---- batched: B sequences per iteration on a paged engine, plain against mixed settings -------------------------------------
    B, S = args.batch, 128
    peng = MixtralEngine(cfg, packed, dev, max_prefill=S * B, max_ctx=B * (S + n + 64), max_new=n, max_seqs=B, penalty_tables=True,
                         max_logprobs=20)
    mixed = [(dict(), dict(PEN)), (TOPKP, dict(PEN, logprobs=20)), (dict(), None), (dict(), dict(logprobs=5))]
    bms = {"plain": [], "mixed": []}
    for r in range(args.rounds):
        for leg in bms:
            seqs = [peng.seq_alloc() for _ in range(B)]
            embs = []
            for i, s in enumerate(seqs):
                ids = torch.randint(3, t.vocab_size, (S,), device=dev)
                embs.append(packed["embed"][ids].float())
                samp, rules = mixed[i % len(mixed)] if leg == "mixed" else (dict(), None)
                peng.seq_set_sampling(s, **samp)
                if rules is not None:
                    peng.seq_set_logit_rules(s, prompt_ids=ids.tolist(), **rules)
            peng.seq_prefill_batch(seqs, embs)
            for _ in range(args.warmup):
                peng.seq_decode(seqs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                peng.seq_decode(seqs)
            torch.cuda.synchronize()
            bms[leg].append((time.perf_counter() - t0) * 1e3 / args.steps)
            for s in seqs:
                peng.check_device_flag(peng.seq_counters(s).tolist())
                peng.seq_free(s)
    peng.close()
    bmed = {k: float(np.median(v)) for k, v in bms.items()}
    res["batched"] = {"sequences": B, "prompt": S, "ms_per_iteration": bmed, "all_rounds": bms,
                      "overhead_pct": 100.0 * (bmed["mixed"] / bmed["plain"] - 1.0),
                      "mixed_settings": "per 4 sequences: penalties; penalties + top-k/top-p + logprobs 20; plain; logprobs 5"}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
