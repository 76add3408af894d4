"""The one way a test runs ranks: `run_ranks(worker, world, *args, deadline_s=...)` starts `world` fresh processes, brings up
the gloo group in each, calls `worker(ctx, *args)` and returns the workers' results as a list indexed by rank.

Worker side.  `ctx` carries `rank`, `world` and (gpu=True) `dev`; the helper has already set MASTER_ADDR / MASTER_PORT, applied
`env` (value None: the variable is removed; "{rank}" / "{world}" in a value are filled in), selected device 0 and created
the process group.  `init_group=False` sets the environment only, for a worker whose code under test creates the group itself.

Epilogue, in this order: the worker's result is sent to the parent; dist.barrier(); sleep(0.5); the clean-ups the worker
registered with ctx.defer() run (last registered first); destroy_process_group().  The order matters twice.  A rank must not close
its engine or communicator before the barrier: until every rank has reported, a peer may still be reading this rank's IPC slots,
and unmapping them under it is a fault on a shared device.  And gloo: a rank that leaves the barrier first must not close its
sockets under the others, hence the pause.  A worker therefore never closes anything itself: it hands the closing over with
ctx.defer(eng.close).  A worker that raises sends its own traceback instead, skips the barrier and the clean-ups (its peers
fail on the broken collective; the exiting process releases the device) and exits with status 1.

Parent side.  One spawn-context pipe per rank, read while waiting, so a rank that reports 10 MB of logits never blocks on a
full pipe; no Manager process.  Every failing rank's traceback is printed and raised in one RankFailure.  Each rank arms
faulthandler.dump_traceback_later shortly before the deadline (a per-rank file; a stuck rank leaves the stacks of all its
threads).  The deadline counts from the moment the last rank finished the preamble (the bring-up before it has BRINGUP_S);
when it passes the parent sends SIGTERM to every rank, waits up to 10 s, sends SIGKILL, joins, and prints those files.  What
follows is `verdict(exit codes, timed out, gpu)`: with gpu=True a deadline or a rank killed by a signal ends the pytest SESSION
(after a hang or an abort nothing more is started on the device); everything else is an ordinary test failure.

Deadlines: 3 x the test's duration at the parent commit on an MI355X, rounded up to a multiple of 30 s, at least 120 s, and
at least 60 s below an enclosing @pytest.mark.timeout (pytest-timeout does not clean up; this helper does, so it fires first).

Parent seconds: the test's `call` duration from `pytest --durations=0` over the touched modules at the parent commit (dd09cba),
one run on an MI355X (GPU sites; profiles/ranks_durations.txt) and one on the CPU (gpu=False sites), 2026-10-19.  A GPU site's test also holds the parent's
oracle arithmetic, so each figure is an upper bound of its run_ranks call.  Every site lands on the 120 s floor, but for the two
under @pytest.mark.timeout(120), which get 60 s.

  site (test)                                                          worker               parent s   deadline s
  test_comm_gpu::test_ipc_allreduce_two_processes_one_gpu              _worker                 3.6        120
  test_comm_gpu::test_tp_engine_world_4_and_8_match_oracle[4]          _tp_worker              6.6        120
  test_comm_gpu::test_tp2_engine_over_ipc_allreduce_matches_oracle[*]  _tp_worker           3.8 - 4.6     120
  test_comm_gpu::test_tp2_engine_over_torch_allreduce_fallback         _tp_worker              3.6        120
  test_comm_gpu::test_tp_released_shard_shapes_match_oracle[4-8, 2-2]  _tp_real_worker       7.7, 5.7     120   (mark 1500)
  test_realgeom_gpu::test_tp_full_depth_omni_matches_oracle[2]         _tp8_omni_worker        6.1        120   (mark 1500)
  test_experts_realgeom_gpu::test_tp2_released_widths_...[int8, mxfp4] _tp_worker            3.3, 3.4     120
  test_sampling_gpu::test_tp2_vocab_sharded_..., test_tp2_unsharded_... _tp_sampling_worker  3.5, 3.5     120
  test_serving_gpu::test_llm_tensor_parallel_two_processes             _tp_llm_worker          6.7        120
  test_tp_gloo::test_tp2_partition_matches_unsharded_oracle            _worker (CPU)           4.7        120   (mark 300)
  test_tp_gloo::test_decode_exchange_vote_..., test_..._trial_...      _vote / _trial_worker (CPU)  3.7, 3.7   60   (mark 120)
  test_bench_cpu::test_rccl_bringup_consensus_world2 (two calls)       _bringup_worker (CPU)   7.6        120 each
"""
import faulthandler
import multiprocessing as mp
import multiprocessing.connection as mpc
import os
import socket
import sys
import tempfile
import time
import traceback
from dataclasses import dataclass
from typing import Any, Optional

import pytest

BRINGUP_S = 120.0           # process start + imports + gloo rendezvous, before the deadline's clock starts
MAX_GPU_WORLD = 8           # the parent has the device open too; the cards hold fewer engine processes than that anyway
TP_UNSET = {"VITA_AMD_TP_FUSE": None, "VITA_AMD_TP_TRIAL": None}      # env=: the ranks choose the exchange form, untimed


class RankFailure(Exception):
    """one or more ranks failed or ran into the deadline; str() holds every rank's own traceback / stack dump."""


class RankCtx:
    def __init__(self, rank, world, dev=None):
        self.rank, self.world, self.dev = rank, world, dev
        self._deferred = []

    def defer(self, fn):
        """run fn() after the barrier that follows the result (see the module docstring): engine / communicator closing."""
        self._deferred.append(fn)


def verdict(exitcodes, timed_out, gpu):
    """"ok" | "fail" | "end-session" from the ranks' exit codes (negative: killed by that signal), whether the deadline passed,
    and whether the ranks had the GPU open."""
    signalled = any(c < 0 for c in exitcodes)
    if gpu and (timed_out or signalled):
        return "end-session"
    if timed_out or any(c != 0 for c in exitcodes):
        return "fail"
    return "ok"


def _rank_main(rank, world, port, worker, args, env, init_group, gpu, conn, deadline_s, dump_path):
    dump = open(dump_path, "w")
    faulthandler.dump_traceback_later(BRINGUP_S - 5, file=dump)
    import torch.distributed as dist
    failed = False
    try:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        for k, v in (env or {}).items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v.format(rank=rank, world=world)
        ctx = RankCtx(rank, world)
        if gpu:
            import torch
            torch.cuda.set_device(0)
            ctx.dev = torch.device("cuda:0")
        if init_group:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        conn.send(("ready", None))
        faulthandler.dump_traceback_later(deadline_s - min(5, deadline_s / 2), file=dump)      # "shortly before": 5 s
        conn.send(("result", worker(ctx, *args)))
        if dist.is_initialized():
            dist.barrier()
        time.sleep(0.5)                  # gloo: a rank that leaves the barrier first must not close its sockets under the others
        for fn in reversed(ctx._deferred):
            fn()
    except BaseException:
        failed = True
        conn.send(("error", traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
        faulthandler.cancel_dump_traceback_later()
        conn.close()
    sys.exit(1 if failed else 0)


def _stop(procs):
    """SIGTERM to every rank still alive, up to 10 s for all of them, SIGKILL, join."""
    for p in procs:
        if p.is_alive():
            p.terminate()
    t_kill = time.monotonic() + 10
    for p in procs:
        p.join(max(t_kill - time.monotonic(), 0))
        if p.is_alive():
            p.kill()
        p.join()


def run_ranks(worker, world, *args, deadline_s, gpu=True, env=None, init_group=True, dump_dir=None):
    """-> [worker(ctx, *args)'s return value of rank r for r in range(world)]; see the module docstring.  dump_dir: where the
    ranks' stack files (rank<r>.stacks) go and stay; default: a temporary directory that goes with the call."""
    if gpu and world > MAX_GPU_WORLD:
        raise ValueError(f"world {world} > {MAX_GPU_WORLD} processes on one device")
    with tempfile.TemporaryDirectory() as tmp:
        return _run(worker, world, args, deadline_s, gpu, env, init_group, str(dump_dir or tmp))


def _run(worker, world, args, deadline_s, gpu, env, init_group, dump_dir):
    sp = mp.get_context("spawn")
    with socket.socket() as s:           # a free port for the gloo rendezvous
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dump_paths = [os.path.join(dump_dir, f"rank{r}.stacks") for r in range(world)]
    procs, conns = [], {}
    for r in range(world):
        rx, tx = sp.Pipe(duplex=False)
        procs.append(sp.Process(target=_rank_main, args=(r, world, port, worker, args, env, init_group, gpu, tx, deadline_s, dump_paths[r])))
        procs[r].start()
        tx.close()                       # the child holds the only write end: its exit is this pipe's end of file
        conns[rx] = r
    results, errors, ready = [None] * world, {}, set()
    limit = time.monotonic() + BRINGUP_S
    try:
        while conns and time.monotonic() < limit:
            for rx in mpc.wait(list(conns), timeout=max(limit - time.monotonic(), 0)):
                r = conns[rx]
                try:
                    kind, val = rx.recv()
                except EOFError:         # the rank has ended
                    rx.close()
                    del conns[rx]
                    continue
                if kind == "ready":
                    ready.add(r)
                    if len(ready) == world:
                        limit = time.monotonic() + deadline_s
                elif kind == "result":
                    results[r] = val
                else:
                    errors[r] = val
        for p in procs:
            p.join(max(limit - time.monotonic(), 0))
    except BaseException:                # KeyboardInterrupt, pytest-timeout: never leave a rank behind
        _stop(procs)
        raise
    timed_out = any(p.is_alive() for p in procs)
    _stop(procs)
    for rx in conns:
        rx.close()
    codes = [p.exitcode for p in procs]
    what = verdict(codes, timed_out, gpu)
    if what == "ok":
        return results
    limit_name = f"deadline of {deadline_s:g} s" if len(ready) == world else f"bring-up limit of {BRINGUP_S:g} s"
    lines = [f"run_ranks({worker.__name__}, world {world}): exit codes {codes}" + (f", {limit_name} passed" if timed_out else "")]
    lines += [f"---- rank {r} ----\n{errors[r]}" for r in sorted(errors)]
    if timed_out:
        lines += [f"---- rank {r}: stacks shortly before the limit ----\n{open(dump_paths[r]).read()}"
                  for r in range(world) if os.path.exists(dump_paths[r])]      # a rank that never started wrote none
    text = "\n".join(lines)
    print(text, flush=True)
    if what == "end-session":
        pytest.exit(f"a rank hung or died by a signal with the GPU open: nothing more is started on it\n{text}", returncode=3)
    raise RankFailure(text)


# ---- what the sharded-engine workers share --------------------------------------------------------------------------------------
@dataclass
class TpRun:
    """what one rank of a sharded engine reports"""
    collective: str                      # what setup_tensor_parallel() agreed on
    tokens: list
    logits: Any                          # [n_new, V] numpy, all-reduced over the vocabulary shards
    comm_status: Optional[int]           # the IPC communicator's spin time-out flag; None: no communicator attached
    exchange: str                        # eng.decode_exchange
    schedule: str                        # eng.decode_schedule()
    vocab_shard: Any = None              # (vocab_lo, vocab_n)
    rows: Optional[int] = None           # prompt rows after the splice
    row0: Any = None                     # what prefill(gather_logits=True) returned
    logits_bytes: Optional[bytes] = None     # logits.tobytes() where a rank sends those in place of the array
    prefill_s: float = 0.0
    decode_s: float = 0.0


def comm_status(eng):
    c = getattr(eng, "_comm", None)
    return c.status() if c is not None else None


def greedy_tp_run(eng, emb, n_new, dist, collective, gather_logits=False, timed=False):
    """prefill, n_new - 1 greedy steps, synchronise, all-reduce the kept logits (vocab-sharded head: rows hold this rank's slice,
    zeros elsewhere), read the communicator's status.  gather_logits: prefill returns the full-vocabulary row (collective inside),
    kept as row0.  timed: synchronise after the prefill too, so that prefill_s / decode_s are each phase's own time."""
    import torch
    t0 = time.time()
    row0 = None
    if gather_logits:
        row0 = eng.prefill(emb, gather_logits=True)[0].cpu().numpy()
    else:
        eng.prefill(emb)
    if timed:
        torch.cuda.synchronize()
    t1 = time.time()
    eng.decode(n_new - 1)
    torch.cuda.synchronize()
    t2 = time.time()
    lg = eng.logits_all[:n_new].cpu()
    dist.all_reduce(lg)
    return TpRun(collective, eng.generated(), lg.numpy(), comm_status(eng), eng.decode_exchange, eng.decode_schedule(),
                 vocab_shard=(eng.c.vocab_lo, eng.c.vocab_n), row0=row0, prefill_s=t1 - t0, decode_s=t2 - t1)


def require_ipc(names, what):
    """The sharded-engine tests are ABOUT the library's IPC transport: a run whose ranks agreed on another collective FAILS
    (VERDICT r04 #1d; it used to xfail, i.e. a box where the IPC bring-up loses kept the suite green).  VITA_ALLOW_GLOO_FALLBACK=1
    turns the failure back into an xfail for a box that is known not to support same-device IPC mapping."""
    if names == {"ipc"}:
        return
    msg = f"{what}: the ranks agreed on {names} instead of the IPC all-reduce: the IPC transport was NOT exercised"
    if os.environ.get("VITA_ALLOW_GLOO_FALLBACK", "") == "1":
        pytest.xfail(msg)
    pytest.fail(msg)
