#!/usr/bin/env python
"""The prompts of N admitted requests one by one (N vh_mixtral_seq_prefill calls: N passes over the weights) against ONE
vh_mixtral_seq_prefill_batch call, at the released geometry (32 layers, H 4096, I 14336, synthetic weights, paged
engine).  Device-synchronised wall time from the first call to the end of the last kernel; every shape is warmed up first; the two
forms alternate inside a round; medians of --rounds rounds with the spread (min .. max).

Workloads: (a) 8 x 64 rows, (b) 8 x 200 rows (audio queries), (c) 4 x 552 rows (the bench request), (d) the mixed list
[40, 97, 64, 130, 20, 75], (e) 1 x 552 through both entry points.  On a tree without seq_prefill_batch (the parent of the change)
only the one-by-one form is timed: that run is the baseline.

Per workload the JSON also holds the algorithmic weight bytes of each form, from the shapes (every expert is touched at these row
counts): N passes against one, and each time as a fraction of its byte floor at 8 TB/s.

  python profiles/bench_prefill_batch.py [--rounds 5] [--workloads a,b,c,d,e] [--out profiles/bench_prefill_batch.json]
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o pb -- python profiles/bench_prefill_batch.py --rounds 1 --workloads a
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {
    "a_8x64": [64] * 8,
    "b_8x200": [200] * 8,
    "c_4x552": [552] * 4,
    "d_mixed": [40, 97, 64, 130, 20, 75],
    "e_1x552": [552],
}
HBM_BYTES_PER_S = 8e12


def weight_bytes(t):
    """bf16 bytes ONE pass streams: per layer QKV, O, router and all experts' gate / up / down; the LM head once"""
    kv = t.num_key_value_heads * t.head_dim
    qo = t.num_attention_heads * t.head_dim
    layer = (qo + 2 * kv) * t.hidden_size + t.hidden_size * qo + t.num_local_experts * t.hidden_size
    layer += t.num_local_experts * 3 * t.intermediate_size * t.hidden_size
    return 2 * (t.num_hidden_layers * layer + t.vocab_size * t.hidden_size)


def timed(eng, lens, embs, batched):
    seqs = [eng.seq_alloc() for _ in lens]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if batched:
        eng.seq_prefill_batch(seqs, embs)
    else:
        for s, e in zip(seqs, embs):
            eng.seq_prefill(s, e)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    for s in seqs:
        eng.check_device_flag(eng.seq_counters(s).tolist())
        eng.seq_free(s)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="a,b,c,d,e")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.config import VitaConfig
    from vita_amd.engine import MixtralEngine
    dev = torch.device("cuda:0")
    cfg = VitaConfig()
    t = cfg.text
    names = [k for k in WORKLOADS if k[0] in args.workloads.split(",")]
    rows_max = max(sum(WORKLOADS[k]) for k in names)
    packed = synth_mixtral_device(cfg, dev, seed=0)
    eng = MixtralEngine(cfg, packed, dev, max_prefill=rows_max, max_ctx=64 * (sum(-(-n // 64) for n in WORKLOADS["c_4x552"]) + 8),
                        max_new=8, max_seqs=8)
    has_batch = hasattr(eng, "seq_prefill_batch")
    ids = torch.randint(3, t.vocab_size, (rows_max,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    emb = packed["embed"][ids].float()
    embs = {}
    for k in names:
        off, embs[k] = 0, []
        for n in WORKLOADS[k]:
            embs[k].append(emb[off:off + n].contiguous())
            off += n
    forms = ["one_by_one"] + (["batched"] if has_batch else [])
    for k in names:                                   # every shape once before anything is timed
        for f in forms:
            timed(eng, WORKLOADS[k], embs[k], f == "batched")
    ms = {k: {f: [] for f in forms} for k in names}
    for _ in range(args.rounds):
        for k in names:
            for f in forms:                           # alternating
                ms[k][f].append(timed(eng, WORKLOADS[k], embs[k], f == "batched"))
    wb = weight_bytes(t)
    res = {"geometry": f"{t.num_hidden_layers} layers, H {t.hidden_size}, I {t.intermediate_size}, bf16 experts, paged engine, "
                       f"max_prefill {rows_max}; median (min .. max) of {args.rounds} alternating rounds, device-synchronised wall ms",
           "has_seq_prefill_batch": has_batch, "weight_bytes_one_pass": wb, "byte_floor_ms_one_pass": wb / HBM_BYTES_PER_S * 1e3,
           "workloads": {}}
    for k in names:
        n = len(WORKLOADS[k])
        w = {"lens": WORKLOADS[k], "rows": sum(WORKLOADS[k])}
        for f in forms:
            v = ms[k][f]
            passes = n if f == "one_by_one" else 1
            floor = passes * wb / HBM_BYTES_PER_S * 1e3
            w[f] = {"ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v), "ms_all": v,
                    "weight_bytes": passes * wb, "byte_floor_ms": floor, "floor_fraction": floor / float(np.median(v))}
        # the same figures against the floor of ONE pass (what a batched pass could reach)
        for f in forms:
            w[f]["one_pass_floor_fraction"] = (wb / HBM_BYTES_PER_S * 1e3) / w[f]["ms_median"]
        if has_batch:
            w["speedup"] = w["one_by_one"]["ms_median"] / w["batched"]["ms_median"]
        res["workloads"][k] = w
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
