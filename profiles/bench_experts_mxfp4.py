#!/usr/bin/env python
"""bf16, int8 and MXFP4 experts at the released geometry (32 layers, H 4096, I 14336, synthetic weights): the three
engines live in ONE process (93.7 + ~50 + ~27 GB) and are timed in interleaved rounds —
  * TP = 1 decode, ms per step (tok/s) after a 552-token prompt,
  * the one-shot prefill at S = 552 (ms, event-timed),
  * aggregate tok/s of 4 / 8 / 16 concurrent sequences (vh_mixtral_seq_decode iterations over the paged KV cache),
the round-to-round spread of each figure, and the largest |logit| difference to the bf16 engine after the same prompt
(information: the quantised engines are different models).

  python profiles/bench_experts_mxfp4.py [--steps 64] [--rounds 3] [--out profiles/bench_experts_mxfp4.json]
  rocprofv3 --kernel-trace --output-format csv -d <dir> -o f4 -- python profiles/bench_experts_mxfp4.py --steps 16 --rounds 1 --batch 8
  python profiles/experts_mxfp4_kernel_table.py <dir>/.../f4_kernel_trace.csv > profiles/bench_experts_mxfp4_kernels.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROMPT = 552


def _decode_ms(eng, emb, warmup, steps):
    eng.reset()
    eng.prefill(emb)
    eng.decode(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.decode(steps)
    torch.cuda.synchronize()
    eng.check_device_flag()
    return (time.perf_counter() - t0) * 1e3 / steps


def _prefill_ms(eng, emb, iters=3):
    out = []
    for _ in range(iters):
        eng.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.prefill(emb)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def _batch_tok_s(eng, emb, n, iters):
    eng.reset()
    seqs = [eng.seq_alloc() for _ in range(n)]
    for i, s in enumerate(seqs):                 # a different 32-token prompt per sequence: the routing differs between them
        eng.seq_prefill(s, emb[32 * i:32 * i + 32])
    for _ in range(2):
        eng.seq_decode(seqs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        eng.seq_decode(seqs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for s in seqs:
        eng.seq_free(s)
    return n * iters / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", default="4,8,16")
    ap.add_argument("--batch-iters", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.config import VitaConfig
    from vita_amd.engine import MixtralEngine
    dev = torch.device("cuda:0")
    cfg = VitaConfig()
    t = cfg.text
    batches = [int(b) for b in args.batch.split(",") if b]
    n = args.steps + args.warmup + 4
    engines = {}
    for mode in ("bf16", "int8", "mxfp4"):
        packed = synth_mixtral_device(cfg, dev, seed=0, experts=mode)
        engines[mode] = MixtralEngine(cfg, packed, dev, max_prefill=PROMPT, max_ctx=64 * (16 * 2 + 12),
                                      max_new=max(n, args.batch_iters + 4), max_seqs=max(batches + [1]))
        torch.cuda.synchronize()
    emb = engines["bf16"].packed["embed"][torch.randint(3, t.vocab_size, (max(PROMPT, 32 * max(batches + [1])),), device=dev,
                                                        generator=torch.Generator(device=dev).manual_seed(1))].float()
    lg = {}
    for mode, eng in engines.items():
        eng.reset()
        lg[mode] = eng.prefill(emb[:PROMPT])[0].clone()
    torch.cuda.synchronize()
    logit_diff = {m: float((lg["bf16"] - lg[m]).abs().max()) for m in engines if m != "bf16"}
    dec = {m: [] for m in engines}
    pre = {m: [] for m in engines}
    agg = {m: {b: [] for b in batches} for m in engines}
    for _ in range(args.rounds):
        for m, eng in engines.items():
            dec[m].append(_decode_ms(eng, emb[:PROMPT], args.warmup, args.steps))
            pre[m].append(_prefill_ms(eng, emb[:PROMPT]))
            for b in batches:
                agg[m][b].append(_batch_tok_s(eng, emb, b, args.batch_iters))
    med = lambda v: float(np.median(v))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))       # round-to-round spread of one figure, relative to its median
    res = {
        "decode_ms_per_step": {m: med(v) for m, v in dec.items()},
        "decode_tok_s": {m: 1e3 / med(v) for m, v in dec.items()},
        "decode_speedup_vs_bf16": {m: med(dec["bf16"]) / med(dec[m]) for m in engines if m != "bf16"},
        "decode_speedup_mxfp4_vs_int8": med(dec["int8"]) / med(dec["mxfp4"]),
        "decode_round_spread": {m: spread(v) for m, v in dec.items()},
        "prefill_ms_S552": {m: med(v) for m, v in pre.items()},
        "prefill_round_spread": {m: spread(v) for m, v in pre.items()},
        "aggregate_tok_s": {m: {str(b): med(v) for b, v in d.items()} for m, d in agg.items()},
        "max_abs_logit_diff_to_bf16_S552": logit_diff,
        "all_rounds": {"decode_ms": dec, "prefill_ms": pre,
                       "aggregate_tok_s": {m: {str(b): v for b, v in d.items()} for m, d in agg.items()}},
        "geometry": f"{t.num_hidden_layers} layers, H {t.hidden_size}, I {t.intermediate_size}, prompt {PROMPT}, {args.steps} timed "
                    f"decode steps after {args.warmup}, median of {args.rounds} interleaved rounds",
    }
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
