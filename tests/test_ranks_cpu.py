"""tests/ranks.py itself, on the CPU (gpu=False everywhere; nothing here opens a device): rank-indexed results, every rank's own
traceback, the deadline path with its stack dumps, the decision after a deadline or a dead rank, a result larger than a pipe's
buffer, and the order of the epilogue."""
import inspect
import multiprocessing
import re
import time

import pytest

from tests.ranks import RankFailure, run_ranks, verdict


def _children():
    return {p.pid for p in multiprocessing.active_children()}


def _value_worker(ctx, base):
    return (ctx.rank, ctx.world, base + 10 * ctx.rank)


def test_results_are_indexed_by_rank_and_no_child_is_left():
    before = _children()
    assert run_ranks(_value_worker, 2, 7, deadline_s=120, gpu=False) == [(0, 2, 7), (1, 2, 17)]
    assert _children() == before


def _raising_worker(ctx):
    import torch
    import torch.distributed as dist
    if ctx.rank == 1:
        raise ValueError("boom")
    dist.all_reduce(torch.zeros(4))          # rank 0: a collective its peer never joins
    return "rank 0 got through"


def test_a_raising_rank_sends_its_own_traceback():
    before = _children()
    with pytest.raises(RankFailure) as ei:
        run_ranks(_raising_worker, 2, deadline_s=120, gpu=False)
    text = str(ei.value)
    assert "---- rank 1 ----" in text and 'ValueError: boom' in text and "in _raising_worker" in text
    if "---- rank 0 ----" in text:           # it failed on the broken collective: its own reason is there too
        assert text.count("Traceback (most recent call last)") == 2
    assert _children() == before


def _sleeping_worker(ctx):
    time.sleep(30)


def test_deadline_ends_both_ranks_and_leaves_their_stacks(tmp_path):
    before = _children()
    t0 = time.monotonic()
    with pytest.raises(RankFailure) as ei:
        run_ranks(_sleeping_worker, 2, deadline_s=2, gpu=False, dump_dir=tmp_path)
    assert time.monotonic() - t0 < 15 + 10   # "about 15 s" after the ranks are up; their start (imports) is not the deadline's
    assert _children() == before
    assert "deadline of 2 s passed" in str(ei.value)
    src, first = inspect.getsourcelines(_sleeping_worker)
    line = first + next(i for i, s in enumerate(src) if "time.sleep" in s)
    for r in range(2):
        dump = (tmp_path / f"rank{r}.stacks").read_text()
        assert dump in str(ei.value)
        assert re.search(rf'test_ranks_cpu\.py", line {line} in _sleeping_worker', dump), dump      # the frame inside time.sleep


def test_verdict():
    assert verdict((0, 0), False, True) == "ok" and verdict((0, 0), False, False) == "ok"
    assert verdict((0, -11), False, True) == "end-session"       # a rank died by a signal with the GPU open
    assert verdict((-6, 0), False, True) == "end-session" and verdict((0, -9), False, True) == "end-session"
    assert verdict((0, 1), False, True) == "fail" and verdict((0, 1), False, False) == "fail"      # a Python exception
    assert verdict((0, -11), False, False) == "fail"
    assert verdict((-15, -15), True, False) == "fail"
    assert verdict((-15, -15), True, True) == "end-session"
    assert verdict((0, 0), True, True) == "end-session"          # ended by SIGTERM's handler or just at the limit: still a deadline


def _large_worker(ctx, n):
    return bytes([ctx.rank + 1]) * n


def test_a_16_mb_result_per_rank_comes_back_whole():
    n = 16 << 20
    got = run_ranks(_large_worker, 2, n, deadline_s=120, gpu=False)
    assert [len(g) for g in got] == [n, n]
    assert got[0] == b"\x01" * n and got[1] == b"\x02" * n


def _stamping_worker(ctx, d):
    import os
    path = lambda what: os.path.join(d, f"{what}{ctx.rank}")

    def stamp(what):
        with open(path(what), "w") as f:
            f.write(repr(time.time()))
    ctx.defer(lambda: stamp("cleanup"))
    if ctx.rank == 1:
        time.sleep(1.0)                      # rank 0 waits at the barrier for this rank, its clean-up with it
    stamp("before")


def test_cleanups_run_after_every_rank_has_passed_the_barrier(tmp_path):
    run_ranks(_stamping_worker, 2, str(tmp_path), deadline_s=120, gpu=False)
    t = lambda what: [float((tmp_path / f"{what}{r}").read_text()) for r in range(2)]
    assert max(t("before")) <= min(t("cleanup")), (t("before"), t("cleanup"))


def test_more_than_8_gpu_ranks_are_refused():
    with pytest.raises(ValueError):
        run_ranks(_value_worker, 9, 0, deadline_s=120, gpu=True)
