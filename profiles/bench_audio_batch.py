#!/usr/bin/env python
"""The audio tower on 1, 2 and 4 clips of different lengths through the public WhaleAudioEncoder.forward(feats, lens), at the released
audio geometry (24 layers, C 1024, 16 heads, F 4096; synthetic weights).  The same script runs on a tree whose forward loops over the
clips (the parent of DESIGN 5.2's one-pass batch) and on one that runs them as one padded pass: forward's signature is the same.

Device-synchronised wall time of one forward call (host launches included: the tower is a chain of short launches); every workload is
warmed up first (scratch, index tables, the folded pos projections); median of --rounds calls with the spread (min .. max).  Run the
two trees as ALTERNATING processes in one visit and compare medians across processes: the process-to-process spread is the bar.

Workloads (frames, 10 ms each): one = [998]; two = [998, 352]; four = [998, 352, 640, 123].
--dump FILE additionally saves the outputs of `one` (bit-identity of the single-clip path across trees).

  python profiles/bench_audio_batch.py [--rounds 5] [--out profiles/bench_audio_batch.json] [--tag tree]
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ab -- python profiles/bench_audio_batch.py --rounds 1 --workloads four
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"one": [998], "two": [998, 352], "four": [998, 352, 640, 123]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="one,two,four")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    from vita_amd.checkpoint import synth_state_dict
    from vita_amd.config import VitaConfig
    from vita_amd.model.encoders import WhaleAudioEncoder
    cfg = VitaConfig()
    dev = "cuda:0"
    enc = WhaleAudioEncoder(synth_state_dict(cfg, seed=11, parts=("audio",)), acfg=cfg.audio, device=dev, llm_dim=cfg.text.hidden_size)
    res = {"tag": a.tag, "rounds": a.rounds, "geometry": {"layers": cfg.audio.num_hidden_layers, "C": cfg.audio.hidden_size},
           "one_pass": hasattr(enc, "encode_batch"), "workloads": {}}
    rng = np.random.default_rng(3)
    for name in a.workloads.split(","):
        lens = WORKLOADS[name]
        feats = np.zeros((len(lens), max(lens), cfg.audio.input_dim), np.float32)
        for b, n in enumerate(lens):
            feats[b, :n] = 4.0 * rng.standard_normal((n, cfg.audio.input_dim)).astype(np.float32)
        x, ln = torch.from_numpy(feats).to(dev), torch.tensor(lens)
        for _ in range(2):
            out = enc(x, ln)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = enc(x, ln)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        valid = out["attention_mask"].sum(1).tolist()
        res["workloads"][name] = {"frames": lens, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms),
                                  "tokens": [int(v) for v in valid]}
        if a.dump and name == "one":
            np.savez(a.dump, embeds=out["inputs_embeds"].cpu().numpy(), mask=out["attention_mask"].cpu().numpy())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
