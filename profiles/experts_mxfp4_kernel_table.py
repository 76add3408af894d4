#!/usr/bin/env python
"""Kernel table of profiles/bench_experts_mxfp4.py from its rocprofv3 kernel trace (--kernel-trace, one round, --batch 8): median
time of the expert kernels per phase, their algorithmic bytes (weights or codes + scales; the GEMVs' activations are a few KB and
are counted) and the fraction of the 8 TB/s HBM spec.

  python profiles/experts_mxfp4_kernel_table.py <dir>/f4_kernel_trace.csv > profiles/bench_experts_mxfp4_kernels.txt

Phases, in trace order (32 calls per forward): per engine (bf16, int8, MXFP4) one S = 552 prefill for the logit difference; then the
round: the decode prefill, three timed S = 552 prefills, decode steps, 8 sequence prefills of 32 tokens, 2 + 8 batched iterations.
The batched rows count the weights of all 8 experts: an upper bound (16 routed rows touch at most 8)."""
import csv
import sys

import numpy as np

H, I, E, L = 4096, 14336, 8, 32
SPEC = 8e12
GLU_B, DOWN_B = 2 * I * H, H * I        # weights of one expert: gate|up, down (elements)


F4 = 17 / 32                            # MXFP4 bytes per weight: 16 code bytes + 1 scale byte per 32
ACT_GU, ACT_DN = 3 * H * 4 + 2 * I * 4, 2 * I * 4 + H * 4    # fp32 activations a GEMV launch reads and writes (x, delta, norm; h; y)


def main(path):
    rows = list(csv.DictReader(open(path)))
    keys = ("k_dec_gateup_mxfp4<", "k_dec_down_mxfp4<", "k_dec_gateup_i8<", "k_dec_down_i8<", "k_dec_gateup<", "k_dec_down<",
            "k_gemm_sp_mxfp4<true", "k_gemm_sp_mxfp4<false", "k_gemm_sp_i8<true", "k_gemm_sp_i8<false", "k_gemm_sp<true",
            "k_gemm_ps<true")
    by = {}
    for r in rows:
        n = r["Kernel_Name"]
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        for key in keys:
            if key in n:
                by.setdefault(key, []).append(d)
                break
    out = ["kernel | phase | calls | median us | MB / call | TB/s | of 8 TB/s"]

    def row(name, phase, v, nbytes):
        if not len(v):
            return
        v = np.asarray(v)
        med = float(np.median(v))
        out.append(f"{name} | {phase} | {len(v)} | {med:.1f} | {nbytes / 1e6:.1f} | {nbytes / med / 1e6:.2f} | {nbytes / med / 1e6 / 8:.2f}")

    g = lambda k: by.get(k, [])
    # batch-1 decode: two routed experts per layer
    row("k_dec_gateup<2,4> (bf16)", "decode", g("k_dec_gateup<"), 2 * GLU_B * 2 + ACT_GU)
    row("k_dec_gateup_i8<2,8>", "decode", g("k_dec_gateup_i8<"), 2 * GLU_B + ACT_GU)
    row("k_dec_gateup_mxfp4<2,1,2>", "decode", g("k_dec_gateup_mxfp4<"), 2 * GLU_B * F4 + ACT_GU)
    row("k_dec_down<7,2> (bf16)", "decode", g("k_dec_down<"), 2 * DOWN_B * 2 + ACT_DN)
    row("k_dec_down_i8<7,4>", "decode", g("k_dec_down_i8<"), 2 * DOWN_B + ACT_DN)
    row("k_dec_down_mxfp4<2,4>", "decode", g("k_dec_down_mxfp4<"), 2 * DOWN_B * F4 + ACT_DN)
    # prefill S = 552 (5 forwards per engine): every expert streamed once
    row("k_gemm_sp<true> (bf16 gate|up)", "prefill S=552", g("k_gemm_sp<true")[:5 * L], E * GLU_B * 2)
    row("k_gemm_sp_i8<true> (gate|up)", "prefill S=552", g("k_gemm_sp_i8<true")[:5 * L], E * GLU_B)
    row("k_gemm_sp_mxfp4<true> (gate|up)", "prefill S=552", g("k_gemm_sp_mxfp4<true")[:5 * L], E * GLU_B * F4)
    row("k_gemm_sp_i8<false> (down)", "prefill S=552", g("k_gemm_sp_i8<false")[:5 * L], E * DOWN_B)
    row("k_gemm_sp_mxfp4<false> (down)", "prefill S=552", g("k_gemm_sp_mxfp4<false")[:5 * L], E * DOWN_B * F4)
    # batched iterations of 8 sequences (16 routed rows; bytes: upper bound, all 8 experts touched)
    row("k_gemm_ps<true,4,8> (bf16 gate|up, cfg 0)", "8 seqs", g("k_gemm_ps<true")[-10 * L:], E * GLU_B * 2)
    row("k_gemm_sp_i8<true> (gate|up)", "8 seqs", g("k_gemm_sp_i8<true")[-10 * L:], E * GLU_B)
    row("k_gemm_sp_mxfp4<true> (gate|up)", "8 seqs", g("k_gemm_sp_mxfp4<true")[-10 * L:], E * GLU_B * F4)
    row("k_gemm_sp_i8<false> (down)", "8 seqs", g("k_gemm_sp_i8<false")[-10 * L:], E * DOWN_B)
    row("k_gemm_sp_mxfp4<false> (down)", "8 seqs", g("k_gemm_sp_mxfp4<false")[-10 * L:], E * DOWN_B * F4)
    print("\n".join(out))


if __name__ == "__main__":
    main(sys.argv[1])
