"""Case list of the prefill MoE GEMM tests (tests/test_moe_gemm_gpu.py) and a plain-Python restatement of the specialised kernel's tile
schedule (vh_gemm_ps_inl.h: for_each_tile under PS_SCHED 1), used by tests/test_moe_gemm_sched_cpu.py as a COVERAGE WITNESS only: it says
which schedule paths the case list reaches on a 256-CU part.  It is never a reference for what the kernel computes."""
from dataclasses import dataclass

# released widths (Mixtral-8x7B as VITA-1.5's text backbone): hidden, intermediate, experts
H, I, E = 4096, 14336, 8
# plain prefill projections on the same kernel: fused QKV rows (32 q + 2 x 8 kv heads of 128) and the O projection
NQKV = 6144
QKV_KSPLIT = -4        # vh_api.hip: -min(4, 8 H / nqkv)
O_KSPLIT = -8
PLAIN_M = (1, 17, 552, 2344, 4600)
TP_WIDTHS = (I // 2, I // 4, I // 8)       # I / TP at TP = 2, 4, 8
RTMAX = 12                                 # row tiles of one m-tile in the specialised kernel (k_gemm_sp<.., 12, ..>)
MOE_KSPLIT = -4                            # the engine's down projection: K split chosen on device, up to 4 slabs


@dataclass(frozen=True)
class Case:
    name: str
    rows: tuple        # rows per expert, experts in group order (sorted token order)
    why: str


CASES = {c.name: c for c in [
    Case("uniform", (138,) * 8,
         "the benchmark shape, S = 552 top-2: gate|up 896 tiles = 3.5 rounds with an M-split tail (9 row tiles -> 5 + 4)"),
    Case("skew", (4600, 4430, 60, 40, 30, 20, 20, 0),
         "long-context skew, S = 4600: 98 % of the entries on two experts, 24 balanced m-tiles each (12 row tiles; the second "
         "expert's last m-tile holds 1), one empty expert"),
    Case("boundary", (0, 1, 16, 17, 191, 192, 193, 385),
         "empty, one row, one full row tile, one row over, one row under / at the 192-row m-tile cap, two m-tiles (7 + 6 row "
         "tiles), three (9 + 9 + 7)"),
    Case("m512", (64,) * 8, "avg 64 rows per group: the auto selection's last ps_cfg 0 point"),
    Case("m513", (65,) + (64,) * 7, "avg 65: the auto selection's first ps_cfg 2 point (5-row-tile tiles, one with a 1-row tail)"),
    Case("one_row", (0, 0, 0, 1, 0, 0, 0, 0),
         "one expert with 1 row: 112 gate|up tiles < 256 blocks (R = 0), M-split tail whose second half is empty"),
    Case("two_rows", (1, 0, 0, 0, 0, 0, 1, 0),
         "two experts with 1 row: 224 gate|up tiles (R = 0), too many for an M-split tail (split_tail false, r > 0)"),
    Case("tall", (48, 0, 176, 30, 128, 0, 160, 0),
         "experts of 3, 11, 2, 8 and 10 row tiles in scrambled group order: with the cases above, every row-tile count 1 .. 12 of "
         "run_tile_sp runs on both projections (ps_cfg 2, auto or forced); gate|up ends in an M-split tail, down takes 3 slabs"),
]}
# Every case runs under the auto selection and with each ps_cfg forced (tests/test_moe_gemm_gpu.py): the few-row cases (avg <= 64 rows per
# group) reach the specialised kernel's schedule only through the forced ps_cfg 2.
TP_CASES = ("uniform", "skew")             # the TP shard widths and the overlap halves run on these two

# ---- the int8 and MXFP4 forms' extra cases (tests/test_moe_gemm_i8_gpu.py, tests/test_moe_gemm_mxfp4_gpu.py; both ALWAYS run the
# specialised kernel, at any row count) ---------------------------------------------------------------------------------------------
# an iteration of a few concurrent sequences at the released widths: rows per expert (tests/test_ops_gpu.py:
# test_gemm_ps_device_chosen_ksplit_few_rows)
DECODE_CNTS = ((2, 0, 1, 0, 0, 2, 0, 1), (1, 1, 1, 0, 1, 1, 0, 1), (3, 2, 4, 1, 2, 1, 2, 1), (6, 0, 0, 0, 0, 0, 0, 0))
# short and odd K: 1 .. 5 stages of 64 pin the stagers' prologue (stage 0, half each), the clamped re-load past a tile's end and the
# stage parity of the two stagers; N with a tail that is not a multiple of 4, one below the GLU / plain tile width and one above
SMALL_K = (64, 128, 192, 256, 320)
SMALL_N = (130, 390)
SMALL_ROWS = {1: (0, 1, 0), 17: (1, 0, 16), 200: (7, 0, 193)}      # M -> rows per group of the grouped form (3 groups)


def small_cases():
    """(M, N, K, glu, grouped, ksplit) of the short-K section: ksplit 1 everywhere, and for plain also the largest legal fixed
    split, K / 64 slabs of ONE stage each."""
    out = []
    for K in SMALL_K:
        for M in SMALL_ROWS:
            for N in SMALL_N:
                for grouped in (True, False):
                    out.append((M, N, K, True, grouped, 1))
                    out.append((M, N, K, False, grouped, 1))
                    if K > 64:
                        out.append((M, N, K, False, grouped, K // 64))
    return out


def ps_q_rt_cap(M, N, glu, ksplit, cus=256):
    """the row-tile cap of an UNGROUPED call with a fixed split in the launcher the int8 and the MXFP4 form share (ps_q_launch in
    vh_gemm_sp.hip): the smallest cap 3 .. 11 whose tiles still fit one round (more, shorter m-tiles while blocks would idle);
    0 = none (12)."""
    grid = max(cus & ~7, 8)
    nrt, NT = (M + 15) >> 4, (N + (127 if glu else 255)) // (128 if glu else 256)
    for c in range(3, 12):
        if ((nrt + c - 1) // c) * NT * ksplit <= grid:
            return c
    return 0


i8_rt_cap = ps_q_rt_cap      # the int8 tests' name of it


def k_slices(K, KS):
    """(k0, nk) in stages of 64 of every K slice: TileCtx k0 / nk of for_each_tile."""
    nk_total = K >> 6
    return [((nk_total * ks) // KS, (nk_total * (ks + 1)) // KS - (nk_total * ks) // KS) for ks in range(KS)]


# ---- the schedule, restated -------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Tile:
    e: int              # expert (group) index
    mi: int             # m-tile of the expert
    nt: int             # n-tile
    ks: int             # K slice
    m_begin: int
    m_end: int
    rt: int             # row tiles holding data
    half: int           # -1: whole tile, 0 / 1: half of an M-split tail tile


@dataclass
class Schedule:
    T: int
    KS: int
    R: int
    r: int
    split_tail: bool
    tiles: list         # every tile some block runs
    empty_halves: int   # M-split tail halves that are empty (skipped by `continue`)


def device_ksplit(MT, NT, nk_total, ksplit, nb):
    """the K split the kernel picks when the caller passes ksplit < 0 (PS_SCHED 1 branch: no one-row-tile credit, 512-row slab price)."""
    best, KS = 1 << 30, 1
    for ks in range(1, min(-ksplit, nk_total) + 1):
        Tx = (MT * NT * ks + 7) >> 3
        Rr, rr = Tx // nb, Tx % nb
        rounds16 = 16 * Rr + (0 if rr == 0 else (9 if 2 * rr <= nb else 16))
        est = (rounds16 * 64) // ks + 4 * rounds16 + ks * ((((48 * 64) // nk_total) * 512) >> 9)
        if est < best:
            best, KS = est, ks
    return KS


def schedule(rows, N, K, glu, ksplit=1, cus=256, cap=0):
    """for_each_tile<GLU, 12> of k_gemm_sp for grouped rows (tuple of rows per group) or a plain GEMM (rows = (M,), no groups).
    cap: VhGemmPsArgs.rt_cap (0 < cap < 12 shortens the m-tiles)."""
    NOUT = 128 if glu else 256
    NT = (N + NOUT - 1) // NOUT
    nk_total = K >> 6
    nb = (cus & ~7) // 8
    rows = list(rows)
    cap = cap if 0 < cap < RTMAX else RTMAX
    mtiles = lambda r: (((r + 15) >> 4) + cap - 1) // cap        # noqa: E731
    ordr = sorted(range(len(rows)), key=lambda e: -rows[e])        # stable, as the kernel's insertion sort
    MT = sum(mtiles(rows[e]) for e in ordr)
    KS = ksplit if ksplit > 1 else 1
    if ksplit < 0:
        KS = device_ksplit(MT, NT, nk_total, ksplit, nb)
    T = MT * NT * KS
    stride = 8 * nb
    R, r = T // stride, T % stride
    split_tail = r > 0 and 2 * r <= stride
    offs = [sum(rows[:e]) for e in range(len(rows))]
    tiles, empty = [], 0
    for jj in range(stride):            # the block -> position map is a bijection for either placement (ps_xcd)
        for it in range(R + 1):
            half = -1
            if it < R:
                g = it * stride + jj
            elif r == 0:
                break
            elif split_tail:
                if jj >= 2 * r:
                    break
                g, half = R * stride + (jj >> 1), jj & 1
            else:
                if jj >= r:
                    break
                g = R * stride + jj
            li = g
            for e in ordr:
                cnt = mtiles(rows[e]) * NT * KS
                if li < cnt:
                    break
                li -= cnt
            else:
                break
            mt = mtiles(rows[e])
            mi, li = li % mt, li // mt
            nt, ks = li % NT, li // NT
            nrt = (rows[e] + 15) >> 4
            rtper = (nrt + mt - 1) // mt
            mb = offs[e] + mi * rtper * 16
            me = min(offs[e] + rows[e], mb + rtper * 16)
            if mb >= me:
                continue
            rt = (me - mb + 15) >> 4
            if half >= 0:
                h0 = (rt + 1) >> 1
                if half == 0:
                    me = min(me, mb + h0 * 16)
                else:
                    mb += h0 * 16
                if mb >= me:
                    empty += 1
                    continue
                rt = (me - mb + 15) >> 4
            tiles.append(Tile(e, mi, nt, ks, mb, me, rt, half))
    return Schedule(T, KS, R, r, split_tail, tiles, empty)


def gateup_schedule(rows, N=I):
    return schedule(rows, N, H, glu=True)


def down_schedule(rows, K=I, N=H, ksplit=MOE_KSPLIT):
    return schedule(rows, N, K, glu=False, ksplit=ksplit)
