"""Coverage witness of the prefill MoE GEMM case list (tests/moe_gemm_cases.py) — no GPU.  The specialised kernel's tile schedule
(vh_gemm_ps_inl.h: for_each_tile, PS_SCHED 1) is restated in Python for a 256-CU part; these tests assert that the cases
tests/test_moe_gemm_gpu.py runs on that kernel reach every schedule path named below, for gate|up and for down.  If the schedule or
the case list changes and a path is no longer reached, this fails and says which."""
import pytest

from tests import moe_gemm_cases as mc


def _reached(sched_of):
    rts, halves, r0, nosplit_tail, empty_second = set(), set(), [], [], []
    for name, case in mc.CASES.items():      # every case runs on the specialised kernel: ps_cfg 2 forced, and auto where avg > 64
        s = sched_of(case.rows)
        rts |= {t.rt for t in s.tiles}
        halves |= {t.half for t in s.tiles if t.half >= 0}
        if s.R == 0:
            r0.append(name)
        if s.r > 0 and not s.split_tail:
            nosplit_tail.append(name)
        if s.empty_halves:
            empty_second.append(name)
    return rts, halves, r0, nosplit_tail, empty_second


@pytest.mark.parametrize("proj", ["gateup", "down"])
def test_case_list_reaches_every_schedule_path(proj):
    sched_of = mc.gateup_schedule if proj == "gateup" else mc.down_schedule      # down: ksplit = -4, the engine's
    rts, halves, r0, nosplit_tail, empty_second = _reached(sched_of)
    assert rts == set(range(1, mc.RTMAX + 1)), f"{proj}: row-tile counts never run: {sorted(set(range(1, 13)) - rts)}"
    assert halves == {0, 1}, f"{proj}: M-split tail halves reached: {sorted(halves)}"
    assert r0, f"{proj}: no case has fewer tiles than blocks (R = 0)"
    assert nosplit_tail, f"{proj}: no case has a partial last round that is not M-split"
    assert empty_second, f"{proj}: no case has an M-split tail whose second half is empty"


def test_named_edges_are_where_the_cases_say():
    """the edges the case descriptions promise, pinned so that a schedule change shows up by name."""
    gu = {n: mc.gateup_schedule(c.rows) for n, c in mc.CASES.items()}
    assert (gu["uniform"].T, gu["uniform"].R, gu["uniform"].r, gu["uniform"].split_tail) == (896, 3, 128, True)
    assert {t.rt for t in gu["uniform"].tiles if t.half >= 0} == {5, 4}
    assert max(t.mi for t in gu["skew"].tiles if t.e in (0, 1)) == 23                   # 24 m-tiles on each hot expert
    assert (gu["one_row"].T, gu["one_row"].R, gu["one_row"].split_tail, gu["one_row"].empty_halves) == (112, 0, True, 112)
    assert (gu["two_rows"].T, gu["two_rows"].R, gu["two_rows"].split_tail) == (224, 0, False)
    bnd = {(t.e, t.mi): t.rt for t in gu["boundary"].tiles if t.half < 0}
    assert [bnd[(6, 0)], bnd[(6, 1)]] == [7, 6] and [bnd[(7, m)] for m in range(3)] == [9, 9, 7]
    for tp_i in mc.TP_WIDTHS:                                                             # NT = 14 at TP = 8
        assert mc.gateup_schedule(mc.CASES["uniform"].rows, N=tp_i).T == 8 * tp_i // 128


@pytest.mark.parametrize("name", list(mc.CASES))
@pytest.mark.parametrize("proj,ksplit", [("gateup", 1), ("down", -4), ("down", 1), ("down", 2), ("down", 3)])
def test_restated_schedule_is_a_partition(name, proj, ksplit):
    """sanity of the restatement itself: every (row, n-tile, K slice) of the problem is in exactly one tile."""
    rows = mc.CASES[name].rows
    s = mc.gateup_schedule(rows) if proj == "gateup" else mc.down_schedule(rows, ksplit=ksplit)
    NT = mc.I // 128 if proj == "gateup" else mc.H // 256
    seen = {}
    for t in s.tiles:
        assert t.m_end - t.m_begin <= 16 * t.rt and 1 <= t.rt <= mc.RTMAX
        key = (t.nt, t.ks)
        seen.setdefault(key, []).append((t.m_begin, t.m_end))
    M = sum(rows)
    assert len(seen) == NT * s.KS
    for key, spans in seen.items():
        spans.sort()
        pos = 0
        for b, e in spans:
            assert b == pos, f"{key}: gap or overlap at row {pos}"
            pos = e
        assert pos == M


# ---- the int8 form (tests/test_moe_gemm_i8_gpu.py): ALWAYS the specialised schedule, at any row count ------------------------------
def _i8_runs():
    """(projection, Schedule, K) of every launch shape of the int8 module's sections a - d on a 256-CU part."""
    runs = []
    for case in mc.CASES.values():                                                        # a. released widths
        runs.append(("gateup", mc.gateup_schedule(case.rows), mc.H))
        runs += [("down", mc.down_schedule(case.rows, ksplit=ks), mc.I) for ks in (mc.MOE_KSPLIT, 1, 2, 3)]
    for name in mc.TP_CASES:                                                              # b. TP shards and the overlap halves
        for it in mc.TP_WIDTHS:
            runs.append(("gateup", mc.gateup_schedule(mc.CASES[name].rows, N=it), mc.H))
            runs += [("down", mc.down_schedule(mc.CASES[name].rows, K=it, N=n), it) for n in (mc.H, mc.H // 2)]
    for cnt in mc.DECODE_CNTS:                                                            # c. batched-decode shapes
        runs += [("gateup", mc.gateup_schedule(cnt), mc.H), ("down", mc.down_schedule(cnt), mc.I)]
    for (M, N, K, glu, grouped, ksplit) in mc.small_cases():                              # d. short and odd K
        rows = mc.SMALL_ROWS[M] if grouped else (M,)
        cap = 0 if grouped else mc.i8_rt_cap(M, N, glu, ksplit)
        runs.append(("gateup" if glu else "down", mc.schedule(rows, N, K, glu, ksplit=ksplit, cap=cap), K))
    return runs


@pytest.mark.parametrize("proj", ["gateup", "down"])
def test_i8_runs_reach_every_schedule_path(proj):
    runs = [(s, K) for p, s, K in _i8_runs() if p == proj]
    rts = {t.rt for s, _ in runs for t in s.tiles}
    halves = {t.half for s, _ in runs for t in s.tiles if t.half >= 0}
    assert rts == set(range(1, mc.RTMAX + 1)), f"{proj}: row-tile counts never run: {sorted(set(range(1, 13)) - rts)}"
    assert halves == {0, 1}, f"{proj}: M-split tail halves reached: {sorted(halves)}"
    assert any(s.empty_halves for s, _ in runs), f"{proj}: no run has an M-split tail whose second half is empty"
    assert any(s.R == 0 for s, _ in runs), f"{proj}: no run has fewer tiles than blocks (R = 0)"
    assert any(s.r > 0 and not s.split_tail for s, _ in runs), f"{proj}: no run has a partial last round that is not M-split"
    # stage counts of the K slices some tile runs: the two stagers alternate stages, so an odd and an even count end on different
    # stagers; a 1-stage slice is the prologue alone
    nks = {mc.k_slices(K, s.KS)[t.ks][1] for s, K in runs for t in s.tiles}
    assert any(n % 2 for n in nks) and any(n % 2 == 0 for n in nks), f"{proj}: stage counts reached: {sorted(nks)}"
    assert 1 in nks, f"{proj}: no 1-stage K slice"
    assert {1, 2, 3, 4, 5} <= nks, f"{proj}: short slices reached: {sorted(n for n in nks if n <= 5)}"


def test_i8_small_cases_reach_the_rt_cap_selection():
    """the ungrouped short-K calls take vhk_gemm_ps_i8's rt_cap branch: a cap below 12 that changes the m-tiling is reached, and
    the largest fixed split has one stage per slab."""
    caps = {(M, mc.i8_rt_cap(M, N, glu, ks)) for (M, N, K, glu, grouped, ks) in mc.small_cases() if not grouped}
    assert (200, 3) in caps                                                               # 13 row tiles -> 5 m-tiles of <= 3
    s = mc.schedule((200,), 390, 320, False, ksplit=5, cap=3)
    assert s.KS == 5 and [nk for _, nk in mc.k_slices(320, 5)] == [1] * 5 and max(t.mi for t in s.tiles) == 4


# ---- the MXFP4 form (tests/test_moe_gemm_mxfp4_gpu.py): the int8 form's launcher and schedule with the fp4 stagers -------------------
def _f4_runs():
    """(projection, Schedule, K) of every launch shape of the MXFP4 module's sections a - d on a 256-CU part.  A knob set changes the
    load form and the placement, not the tiles, and the dense and the strided (ldw = I) form of a shard's down run the same tiles."""
    runs = []
    for case in mc.CASES.values():                                                        # a. released widths
        runs.append(("gateup", mc.gateup_schedule(case.rows), mc.H))
        runs += [("down", mc.down_schedule(case.rows, ksplit=ks), mc.I) for ks in (mc.MOE_KSPLIT, 1, 2, 3)]
    for name in mc.TP_CASES:                                                              # b. TP shards and the overlap halves
        for it in mc.TP_WIDTHS:
            runs.append(("gateup", mc.gateup_schedule(mc.CASES[name].rows, N=it), mc.H))
            runs += [("down", mc.down_schedule(mc.CASES[name].rows, K=it, N=n), it) for n in (mc.H, mc.H // 2)]
    for cnt in mc.DECODE_CNTS:                                                            # c. batched-decode shapes
        runs += [("gateup", mc.gateup_schedule(cnt), mc.H), ("down", mc.down_schedule(cnt), mc.I)]
    for (M, N, K, glu, grouped, ksplit) in mc.small_cases():                              # d. short and odd K
        rows = mc.SMALL_ROWS[M] if grouped else (M,)
        cap = 0 if grouped else mc.ps_q_rt_cap(M, N, glu, ksplit)
        runs.append(("gateup" if glu else "down", mc.schedule(rows, N, K, glu, ksplit=ksplit, cap=cap), K))
    return runs


def _stager_ends(nk):
    """how each fp4 stager wave g leaves a K slice of nk stages (run_tile_sp: after the shared stage 0, wave g runs k = g, g + 2, ..
    < nk and stores stage k + 1 when there is one): 'idle' (no iteration), 'store' or 'skip' in its last iteration."""
    out = []
    for g in (0, 1):
        ks = list(range(g, nk, 2))
        out.append((g, "idle" if not ks else "store" if ks[-1] + 1 < nk else "skip"))
    return out


@pytest.mark.parametrize("proj", ["gateup", "down"])
def test_f4_runs_reach_every_schedule_path(proj):
    runs = [(s, K) for p, s, K in _f4_runs() if p == proj]
    rts = {t.rt for s, _ in runs for t in s.tiles}
    halves = {t.half for s, _ in runs for t in s.tiles if t.half >= 0}
    assert rts == set(range(1, mc.RTMAX + 1)), f"{proj}: row-tile counts never run: {sorted(set(range(1, 13)) - rts)}"
    assert halves == {0, 1}, f"{proj}: M-split tail halves reached: {sorted(halves)}"
    assert any(s.empty_halves for s, _ in runs), f"{proj}: no run has an M-split tail whose second half is empty"
    assert any(s.R == 0 for s, _ in runs), f"{proj}: no run has fewer tiles than blocks (R = 0)"
    assert any(s.r > 0 and not s.split_tail for s, _ in runs), f"{proj}: no run has a partial last round that is not M-split"
    nks = {mc.k_slices(K, s.KS)[t.ks][1] for s, K in runs for t in s.tiles}
    assert {1, 2, 3, 4, 5} <= nks, f"{proj}: short slices reached: {sorted(n for n in nks if n <= 5)}"
    # both stage parities for each stager wave: either wave ends a slice on a store and on a skipped one, wave 1 also idles (nk = 1)
    ends = {e for n in nks for e in _stager_ends(n)}
    assert ends == {(0, "store"), (0, "skip"), (1, "store"), (1, "skip"), (1, "idle")}, f"{proj}: stager endings reached: {sorted(ends)}"
    if proj == "down":                                                                    # tiles the stagers address with k0 != 0
        assert any(mc.k_slices(K, s.KS)[t.ks][0] > 0 for s, K in runs for t in s.tiles)


def test_f4_small_cases_reach_the_rt_cap_selection():
    """the ungrouped short-K calls take the shared launcher's rt_cap branch: a cap below 12 that changes the m-tiling is reached, and
    the largest fixed split has one stage per slab (every slab but the first starts at k0 != 0)."""
    caps = {(M, mc.ps_q_rt_cap(M, N, glu, ks)) for (M, N, K, glu, grouped, ks) in mc.small_cases() if not grouped}
    assert any(0 < c < mc.RTMAX for _, c in caps) and (200, 3) in caps                    # 13 row tiles -> 5 m-tiles of <= 3
    s = mc.schedule((200,), 390, 320, False, ksplit=5, cap=3)
    assert s.KS == 5 and mc.k_slices(320, 5) == [(i, 1) for i in range(5)] and max(t.mi for t in s.tiles) == 4
