#!/usr/bin/env python
"""An iteration that admits requests as TWO passes over the weights (vh_mixtral_seq_prefill_batch for the prompts, then a
vh_mixtral_seq_decode iteration for the running sequences) against ONE vh_mixtral_seq_step, at the released geometry
(32 layers, H 4096, I 14336, synthetic weights, paged engine).  Device-synchronised wall time from the first call to the end of the
last kernel; every form is warmed up first; the forms alternate inside a round; medians of --rounds rounds with the spread
(min .. max).  Every timed call advances the running sequences by one token (their context grows by one key per call).

Workloads: (a) 8 running at ctx ~600 + 2 prompts x 200 rows, (b) 8 running at ctx ~4200 + 1 prompt x 552 rows, (c) 16 running at ctx
~600 + 1 prompt x 64 rows, (d) 16 running, no prompt (seq_step decode-only against seq_decode).  Forms: two_calls, seq_step, and on
(b), (c) seq_step_attn0 = vh_tune("step_attn", 0), the single rows through the segment attention.  On a tree without seq_step (the
parent of the change; --tree DIR imports vita_amd from there) only two_calls is timed: that run is the baseline.

--sched: the scheduler effect through ContinuousBatcher, chunked_prefill off (max_prefill 2344) and on (budget 512): 8 requests
run at ctx ~600 when a 2344-row prompt arrives; reported are the largest gap between two consecutive tokens of a running request
from then on and the time to the newcomer's first token.

  python profiles/bench_mixed_step.py [--rounds 5] [--workloads a,b,c,d] [--sched] [--tree DIR] [--out FILE]
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ms -- python profiles/bench_mixed_step.py --rounds 1 --workloads b
"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np
import torch

WORKLOADS = {                      # running sequences, their context, prompt lengths
    "a_8run_2x200": (8, 600, [200, 200]),
    "b_8run_ctx4200_1x552": (8, 4200, [552]),
    "c_16run_1x64": (16, 600, [64]),
    "d_16run_decode_only": (16, 600, []),
}
HBM_BYTES_PER_S = 8e12


def weight_bytes(t):
    """bf16 bytes ONE pass streams: per layer QKV, O, router and all experts' gate / up / down; the LM head once"""
    kv = t.num_key_value_heads * t.head_dim
    qo = t.num_attention_heads * t.head_dim
    layer = (qo + 2 * kv) * t.hidden_size + t.hidden_size * qo + t.num_local_experts * t.hidden_size
    layer += t.num_local_experts * 3 * t.intermediate_size * t.hidden_size
    return 2 * (t.num_hidden_layers * layer + t.vocab_size * t.hidden_size)


def rows(emb, n, off=0):
    idx = (torch.arange(n, device=emb.device) + off) % emb.shape[0]
    return emb[idx].contiguous()


def start_running(eng, emb, n, ctx):
    seqs = [eng.seq_alloc() for _ in range(n)]
    for i, s in enumerate(seqs):
        x = rows(emb, ctx, 37 * i)
        for s0 in range(0, ctx, eng.max_prefill):
            eng.seq_prefill(s, x[s0:s0 + eng.max_prefill])
    eng.seq_decode(seqs)
    torch.cuda.synchronize()
    return seqs


def timed(eng, form, run, embs):
    from vita_amd import _lib
    new = [eng.seq_alloc() for _ in embs]
    if form == "seq_step_attn0":
        _lib.tune("step_attn", 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if form == "two_calls":
        if new:
            eng.seq_prefill_batch(new, embs)
        eng.seq_decode(run)
    else:
        eng.seq_step(new, embs, run)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    if form == "seq_step_attn0":
        _lib.tune("step_attn", 1)
    for s in new + run[:1]:
        eng.check_device_flag(eng.seq_counters(s).tolist())
    for s in new:
        eng.seq_free(s)
    return ms


def scheduler_effect(eng, emb, chunked):
    """8 requests run at ctx ~600; a 2344-row prompt arrives -> (largest gap between consecutive tokens of a running request from
    then on, time to the newcomer's first token), ms"""
    from vita_amd.scheduler import ContinuousBatcher
    kw = dict(chunked_prefill=True, max_batched_tokens=512) if chunked else {}
    bt = ContinuousBatcher(eng, window=1, **kw)
    for i in range(8):
        bt.add(i, rows(emb, 600, 91 * i), max_tokens=60)
    while bt.waiting or getattr(bt, "prefilling", None):
        bt.step()
    for _ in range(3):
        bt.step()
    torch.cuda.synchronize()
    t_add = last = time.perf_counter()
    bt.add("new", rows(emb, 2344, 5), max_tokens=4)
    gap, ttft = 0.0, None
    while ttft is None or len(bt.running) > 8:
        ev = bt.step()
        now = time.perf_counter()
        if any(rid != "new" and new for rid, new, *_ in ev):
            gap, last = max(gap, now - last), now
        if ttft is None and any(rid == "new" and new for rid, new, *_ in ev):
            ttft = now - t_add
    stats = dict(bt.stats)
    for r in list(bt.running) + list(bt.waiting):
        bt.abort(r.id)
    return gap * 1e3, ttft * 1e3, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="a,b,c,d")
    ap.add_argument("--sched", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.config import VitaConfig
    from vita_amd.engine import MixtralEngine
    from vita_amd.scheduler import ContinuousBatcher
    dev = torch.device("cuda:0")
    cfg = VitaConfig()
    t = cfg.text
    names = [k for k in WORKLOADS if k[0] in args.workloads.split(",")]
    max_prefill = 2344 if args.sched else 1024
    pool = 64 * (8 * (-(-4300 // 64)) + 48 + 16)
    packed = synth_mixtral_device(cfg, dev, seed=0)
    eng = MixtralEngine(cfg, packed, dev, max_prefill=max_prefill, max_ctx=pool, max_new=128, max_seqs=18)
    has_step = hasattr(eng, "seq_step")
    ids = torch.randint(3, t.vocab_size, (2344,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    emb = packed["embed"][ids].float()
    wb = weight_bytes(t)
    res = {"geometry": f"{t.num_hidden_layers} layers, H {t.hidden_size}, I {t.intermediate_size}, bf16 experts, paged engine, "
                       f"max_prefill {max_prefill}; median (min .. max) of {args.rounds} alternating rounds, device-synchronised wall ms",
           "tree": os.path.abspath(args.tree), "has_seq_step": has_step, "weight_bytes_one_pass": wb,
           "byte_floor_ms_one_pass": wb / HBM_BYTES_PER_S * 1e3, "workloads": {}}
    for k in names:
        n_run, ctx, lens = WORKLOADS[k]
        run = start_running(eng, emb, n_run, ctx)
        embs = [rows(emb, n, 11 * i) for i, n in enumerate(lens)]
        forms = ["two_calls"] + (["seq_step"] if has_step else []) + (["seq_step_attn0"] if has_step and k[0] in "bc" else [])
        for f in forms:                               # every form once before anything is timed
            timed(eng, f, run, embs)
        ms = {f: [] for f in forms}
        for _ in range(args.rounds):
            for f in forms:                           # alternating
                ms[f].append(timed(eng, f, run, embs))
        w = {"running": n_run, "ctx": ctx, "prompts": lens}
        for f in forms:
            v = ms[f]
            w[f] = {"ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v), "ms_all": v}
        if has_step:
            w["saved_ms"] = w["two_calls"]["ms_median"] - w["seq_step"]["ms_median"]
        res["workloads"][k] = w
        for s in run:
            eng.seq_free(s)
    if args.sched:
        res["scheduler"] = {}
        modes = [False] + ([True] if has_step and "chunked_prefill" in inspect.signature(ContinuousBatcher.__init__).parameters else [])
        for chunked in modes:
            gap, ttft, stats = scheduler_effect(eng, emb, chunked)
            res["scheduler"]["chunked_prefill_on" if chunked else "chunked_prefill_off"] = {
                "max_gap_between_tokens_ms": gap, "newcomer_first_token_ms": ttft, "stats": stats}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
