#!/usr/bin/env python
"""Time to first token with the prefix cache, at the released geometry (32 layers, H 4096, I 14336, synthetic weights,
paged engine) for the two prompt shapes of the README: S = 552 (one image + audio query) and S = 2344 (8-frame video turn).

Per shape, through ContinuousBatcher(prefix_cache=True), the device-synchronised wall time from add() to the end of the step() that
admits and prefills the request (its first token is then on the device; the step's one decode iteration is part of every figure):
  cold      the cache holds nothing of the prompt
  warm      the same prompt again: (S - 1) // 64 pages adopted, the rest prefilled
  shared40  a prompt that shares all but its last 40 rows with the cached one
  batcher_off  the same add -> step through a batcher WITHOUT the cache (also timed on the parent: what cold adds is hash + copy)
Next to them, on the same engine: `prefill_full` and `prefill_suffix`, a stand-alone vh_mixtral_seq_prefill of S rows and of the warm
/ shared40 suffix lengths at position 0 (what a prompt of only that many rows costs), and `hash`, vh_hash_row_blocks over the S rows
alone.  Every figure is the median (min .. max) of --rounds rounds in which the variants alternate; every shape is warmed up first.

On a tree without the feature (the parent of the change) only prefill_full / prefill_suffix are timed: that run is the baseline the
warm figures are compared with (--out profiles/... of that run is merged with --parent).

  python profiles/bench_prefix_cache.py [--rounds 5] [--shapes 552,2344] [--parent parent.json] [--bench-lines lines.json] [--out profiles/bench_prefix_cache.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(v):
    return {"ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "ms_all": [float(x) for x in v]}


def prefill_alone(eng, emb):
    s = eng.seq_alloc()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.seq_prefill(s, emb)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    eng.check_device_flag(eng.seq_counters(s).tolist())
    eng.seq_free(s)
    return ms


def first_token(bt, rid, emb):
    """add -> the end of the step that prefills the request; the request is then aborted (its pages stay cached)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bt.add(rid, emb, max_tokens=4)
    bt.step()                                          # ends in a stream synchronise
    ms = (time.perf_counter() - t0) * 1e3
    hit = getattr(bt, "cached_tokens", {}).get(rid, 0)
    bt.abort(rid)
    return ms, hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="552,2344")
    ap.add_argument("--parent", default=None, help="JSON of this script's run on the parent commit (baseline prefill times)")
    ap.add_argument("--bench-lines", default=None, help="JSON with the alternating bench.py result lines of parent and tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vita_amd import ops, serving
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.config import VitaConfig
    from vita_amd.engine import MixtralEngine
    dev = torch.device("cuda:0")
    cfg = VitaConfig()
    t = cfg.text
    shapes = [int(x) for x in args.shapes.split(",")]
    s_max = max(shapes)
    has_cache = hasattr(serving, "PrefixCache") and hasattr(ops, "hash_row_blocks")
    packed = synth_mixtral_device(cfg, dev, seed=0)
    # pool: the cached prompt, a running copy of it and headroom
    eng = MixtralEngine(cfg, packed, dev, max_prefill=s_max, max_ctx=64 * (3 * (-(-s_max // 64) + 2)), max_new=8, max_seqs=2)
    g = torch.Generator(device=dev).manual_seed(1)
    res = {"geometry": f"{t.num_hidden_layers} layers, H {t.hidden_size}, I {t.intermediate_size}, bf16 experts, paged engine; median "
                       f"(min .. max) of {args.rounds} alternating rounds, device-synchronised wall ms",
           "has_prefix_cache": has_cache, "shapes": {}}
    for S in shapes:
        ids = torch.randint(3, t.vocab_size, (S + 40,), device=dev, generator=g)
        rows = packed["embed"][ids].float()
        base = rows[:S].contiguous()
        shared = torch.cat([rows[:S - 40], rows[S:S + 40]]).contiguous()        # all but the last 40 rows in common
        warm_suffix = S - 64 * ((S - 1) // 64)
        shared_suffix = S - 64 * ((S - 40) // 64)
        out = {"S": S, "warm_suffix_rows": warm_suffix, "shared40_suffix_rows": shared_suffix}
        alone = {"prefill_full": base, "prefill_suffix_warm": base[:warm_suffix].contiguous(),
                 "prefill_suffix_shared40": base[:shared_suffix].contiguous()}
        ms = {k: [] for k in alone}
        ms["batcher_off"] = []
        bt_off = serving.ContinuousBatcher(eng, embed_tokens=lambda i: packed["embed"][i].float())
        for e in alone.values():                                               # every shape once before anything is timed
            prefill_alone(eng, e)
        first_token(bt_off, "o", base)
        if has_cache:
            ms.update({"cold": [], "warm": [], "shared40": [], "hash": []})
            bt = serving.ContinuousBatcher(eng, embed_tokens=lambda i: packed["embed"][i].float(), prefix_cache=True)
            for rid, e in (("w0", base), ("w1", base), ("w2", shared)):
                first_token(bt, rid, e)
            ops.hash_row_blocks(base)
            bt.cache.clear()
        for r in range(args.rounds):
            for k, e in alone.items():
                ms[k].append(prefill_alone(eng, e))
            ms["batcher_off"].append(first_token(bt_off, f"o{r}", base)[0])
            if has_cache:
                a, hit_c = first_token(bt, f"c{r}", base)
                b, hit_w = first_token(bt, f"w{r}", base)
                c, hit_s = first_token(bt, f"s{r}", shared)
                assert (hit_c, hit_w, hit_s) == (0, S - warm_suffix, S - shared_suffix), (hit_c, hit_w, hit_s)
                ms["cold"].append(a); ms["warm"].append(b); ms["shared40"].append(c)
                bt.cache.clear()                                               # the next round starts cold
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.hash_row_blocks(base)
                torch.cuda.synchronize()
                ms["hash"].append((time.perf_counter() - t0) * 1e3)
        out.update({k: med(v) for k, v in ms.items()})
        if has_cache:
            out["warm_over_cold"] = out["warm"]["ms_median"] / out["cold"]["ms_median"]
            out["shared40_over_cold"] = out["shared40"]["ms_median"] / out["cold"]["ms_median"]
            out["hash_over_prefill_full"] = out["hash"]["ms_median"] / out["prefill_full"]["ms_median"]
            assert eng.pages_free() == eng.max_ctx // 64
        res["shapes"][str(S)] = out
    if args.parent:
        with open(args.parent) as f:
            par = json.load(f)
        res["parent"] = {"note": "this script on the parent commit (no prefix cache): stand-alone prefills only", "shapes": par["shapes"]}
        for S, out in res["shapes"].items():
            p = par["shapes"].get(S)
            if p and has_cache:
                out["vs_parent"] = {
                    "parent_cold_prefill_ms": p["prefill_full"]["ms_median"],
                    "parent_batcher_first_token_ms": p["batcher_off"]["ms_median"], "cold_ms": out["cold"]["ms_median"],
                    "hash_ms": out["hash"]["ms_median"],
                    "warm_ms": out["warm"]["ms_median"], "parent_suffix_prefill_ms": p["prefill_suffix_warm"]["ms_median"],
                    "shared40_ms": out["shared40"]["ms_median"], "parent_suffix_shared40_prefill_ms": p["prefill_suffix_shared40"]["ms_median"],
                    "warm_over_parent_cold": out["warm"]["ms_median"] / p["prefill_full"]["ms_median"]}
    if args.bench_lines:
        with open(args.bench_lines) as f:
            res["cache_off_regression"] = json.load(f)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    eng.close()


if __name__ == "__main__":
    main()
