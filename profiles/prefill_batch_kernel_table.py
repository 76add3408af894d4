#!/usr/bin/env python
"""Kernel table of profiles/bench_prefill_batch.py from a rocprofv3 --kernel-trace run of its own (workload a: 8 x 64 rows):
the trace is cut into prefill passes at the token-select launches that end a pass (one select: a vh_mixtral_seq_prefill call,
n selects: one vh_mixtral_seq_prefill_batch call of n segments); printed: GPU time per kernel of the LAST timed one-by-one
group (n passes) next to the LAST batched pass.

  python profiles/prefill_batch_kernel_table.py <dir>/pb_kernel_trace.csv > profiles/bench_prefill_batch_kernels.txt
"""
import csv
import re
import sys
from collections import OrderedDict

HEAD = ("k_dec_select", "k_decb_lmhead", "k_dec_lmhead", "k_dec_sample", "k_dec_cand")


def short(name):
    m = re.search(r"(k_\w+(?:<[^>]*>)?)", name)
    return m.group(1) if m else name[:60]


def main(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            n = short(r["Kernel_Name"])
            if n.startswith("k_") and "fill_hash" not in n:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n, r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"]))
    rows.sort()
    passes, cur, selects = [], [], 0
    for i, r in enumerate(rows):
        cur.append(r)
        if r[2].startswith("k_dec_select"):
            selects += 1
            nxt = rows[i + 1][2] if i + 1 < len(rows) else ""
            if not nxt.startswith(HEAD):
                passes.append((selects, cur))
                cur, selects = [], 0
    n = max(s for s, _ in passes)
    last_batched = max(i for i, (s, _) in enumerate(passes) if s == n)
    singles = [p for s, p in passes[:last_batched] if s == 1][-n:]
    batched = passes[last_batched][1]

    def table(ps):
        t = OrderedDict()
        for p in ps:
            for s, e, name, *_ in p:
                c = t.setdefault(name, [0, 0])
                c[0] += 1
                c[1] += e - s
        return t
    a, b = table(singles), table([batched])
    span = lambda p: (p[-1][1] - p[0][0]) / 1e6
    print(f"{n} x 64 rows, released geometry, 32 layers; GPU time of the kernels, us (launches)")
    print(f"{'kernel':44s} {'one by one (' + str(n) + ' passes)':>26s} {'one batched pass':>22s}")
    for k in list(a) + [k for k in b if k not in a]:
        ca, cb = a.get(k, [0, 0]), b.get(k, [0, 0])
        print(f"{k:44s} {ca[1] / 1e3:16.1f} ({ca[0]:5d}) {cb[1] / 1e3:14.1f} ({cb[0]:4d})")
    print(f"{'sum of kernels':44s} {sum(c[1] for c in a.values()) / 1e3:16.1f} {'':8s}{sum(c[1] for c in b.values()) / 1e3:14.1f}")
    print(f"{'first launch to last end, ms':44s} {sum(span(p) for p in singles):16.2f} {'':8s}{span(batched):14.2f}")
    g = [r for r in batched if r[2].startswith("k_attn")][0]
    print(f"attention launch of the batched pass: {g[2]}, grid ({g[3]}, {g[4]}, {g[5]}) threads")


if __name__ == "__main__":
    main(sys.argv[1])
