"""MXFP4 experts at the RELEASED widths (H 4096, I 14336, 32 / 8 heads, vocab 51760) on 3 layers of synthetic weights
(counter-based generator: the same values on the device and in the layer-streamed oracle), against the fp32 oracle evaluated on
w' = e2m1(code) 2^(byte - 127) (tests/q4_ref.py wraps oracle.stream's weight buffers); the cases and bars of
tests/test_experts_int8_realgeom_gpu.py (one layer fewer: see LAYERS):
  * one request, S = 552 + 8 greedy steps: ids ==, every router decision of the prompt ==, logits within 1e-3;
  * six sequences through vh_mixtral_seq_decode with batch_moe_min 3 (the MXFP4 streaming MoE GEMM) and 0 (per-sequence GEMVs);
  * TP = 2: two engine processes on one GPU over the library's IPC all-reduce (w2 shards are slices of the codes and the scales, the tensor-parallel
    prefill's column halves), ids == the same oracle's, logits within 1e-3."""
import os
import time

import numpy as np
import pytest
import torch

from oracle import stream
from tests import q4_ref
from vita_amd import _lib
from vita_amd.checkpoint import synth_mixtral_device
from vita_amd.config import VitaConfig

pytestmark = pytest.mark.gpu
SEED, LAYERS, S, T_NEW = 0, 3, 552, 8       # 3 layers: quantising w' in numpy costs more than int8's, the module keeps its wall time
SEQ_LENS, SEQ_STEPS = (17, 40, 64, 9, 33, 50), 6


def _cfg():
    cfg = VitaConfig()
    cfg.text.num_hidden_layers = LAYERS
    return cfg


def _prompt_ids(V):
    rng = np.random.default_rng(5)
    return rng.integers(3, V, size=S).tolist(), [rng.integers(3, V, size=n).tolist() for n in SEQ_LENS]


@pytest.fixture(scope="module")
def run(dev):
    from vita_amd.engine import MixtralEngine
    cfg = _cfg()
    t = cfg.text
    ids, prompts = _prompt_ids(t.vocab_size)
    packed = synth_mixtral_device(cfg, dev, seed=SEED, experts="mxfp4")
    emb = lambda x: packed["embed"][torch.tensor(x, device=dev)].float()
    eng = MixtralEngine(cfg, packed, dev, max_prefill=S, max_new=T_NEW + 4, logit_rows=T_NEW + 4)
    assert eng.experts == "mxfp4"
    eng.prefill(emb(ids), want_route=True)
    route = eng.route_ids.cpu().numpy()
    eng.decode(T_NEW - 1)
    torch.cuda.synchronize()
    out = dict(cfg=cfg, ids=ids, prompts=prompts, toks=eng.generated(), logits=eng.logits_all[:T_NEW].cpu().numpy(), route=route)
    eng.close()
    lib = _lib.load()
    seq_toks = {}
    try:
        for bmm in (3, 0):
            _lib.check(lib.vh_tune(b"batch_moe_min", bmm), "vh_tune")
            eng = MixtralEngine(cfg, packed, dev, max_prefill=64, max_ctx=64 * 8, max_new=SEQ_STEPS + 4, max_seqs=len(prompts))
            seqs = [eng.seq_alloc() for _ in prompts]
            for s, p in zip(seqs, prompts):
                eng.seq_prefill(s, emb(p))
            for _ in range(SEQ_STEPS - 1):
                eng.seq_decode(seqs)
            torch.cuda.synchronize()
            seq_toks[bmm] = [eng.seq_tokens(s)[:SEQ_STEPS].tolist() for s in seqs]
            eng.check_device_flag()
            eng.close()
    finally:
        lib.vh_tune(b"batch_moe_min", 3)
    out["seq_toks"] = seq_toks
    del packed
    torch.cuda.empty_cache()
    return out


@pytest.fixture(scope="module")
def oracle(run):
    """ONE teacher-forced pass of the streamed oracle on w' over the request and the six sequences (prompt + the device's tokens)."""
    t = run["cfg"].text
    rows = lambda x: stream.embed_rows(t, x, SEED)
    embs = [np.concatenate([rows(run["ids"]), rows(run["toks"][:-1])], 0)]
    embs += [np.concatenate([rows(p), rows(st[:-1])], 0) for p, st in zip(run["prompts"], run["seq_toks"][3])]
    t0 = time.time()
    with q4_ref.streamed_experts_wprime():
        ref = stream.forward_many(t, SEED, embs, n_layers=LAYERS, logits_from=[S - 1] + [len(p) - 1 for p in run["prompts"]])
    print(f"[mxfp4 realgeom] oracle ({LAYERS} layers, {sum(e.shape[0] for e in embs)} rows) in {time.time() - t0:.1f}s")
    return ref


def test_released_widths_request_vs_oracle_on_wprime(run, oracle):
    ref = oracle[0]
    r_dev, r_ref = np.sort(run["route"], -1), np.sort(ref["route"][:, :S], -1)
    mism = np.argwhere((r_dev != r_ref).any(-1))
    print(f"router top-2 sets: {r_dev.shape[0] * S} decisions, {len(mism)} differ", mism[:5].tolist())
    assert r_dev.shape == (LAYERS, S, 2) and len(mism) == 0
    ref_ids = ref["logits"].argmax(-1).tolist()
    err = float(np.abs(run["logits"] - ref["logits"]).max())
    print("device ids", run["toks"], "oracle ids", ref_ids, f"max |logit diff| {err:.2e}")
    assert run["toks"] == ref_ids
    assert err < 1e-3


def test_released_widths_six_sequences_vs_oracle_on_wprime(run, oracle):
    for i, ref in enumerate(oracle[1:]):
        ref_ids = ref["logits"].argmax(-1).tolist()
        assert run["seq_toks"][3][i] == ref_ids, (i, run["seq_toks"][3][i], ref_ids)   # the streamed MXFP4 MoE GEMM (n >= 3)
        assert run["seq_toks"][0][i] == ref_ids, (i, run["seq_toks"][0][i], ref_ids)   # per-sequence MXFP4 GEMVs


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tp_worker(rank, world, port, ret):
    """one rank of TP = 2 at the released shard widths (16 q + 4 KV heads, 7168 columns of every expert, half the vocabulary)"""
    import torch.distributed as dist
    from vita_amd.engine import MixtralEngine
    from vita_amd.parallel import setup_tensor_parallel
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.pop("VITA_AMD_TP_FUSE", None)
    os.environ.pop("VITA_AMD_TP_TRIAL", None)
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = _cfg()
        ids, _ = _prompt_ids(cfg.text.vocab_size)
        packed = synth_mixtral_device(cfg, dev, seed=SEED, rank=rank, world=world, experts="mxfp4")
        eng = MixtralEngine(cfg, packed, dev, max_prefill=S, max_new=T_NEW + 4, logit_rows=T_NEW + 4, rank=rank, world=world)
        assert eng.experts == "mxfp4" and eng.c.inter == 14336 // world
        name = setup_tensor_parallel(eng, rank, world, dev, backend="gloo", collective="ipc")
        eng.prefill(packed["embed"][torch.tensor(ids, device=dev)].float())
        eng.decode(T_NEW - 1)
        torch.cuda.synchronize()
        lg = eng.logits_all[:T_NEW].cpu()
        dist.all_reduce(lg)                      # vocab-sharded head: rows hold this rank's slice, zeros elsewhere
        c = getattr(eng, "_comm", None)
        ret[rank] = (name, eng.generated(), lg.numpy(), c.status() if c is not None else None)
        dist.barrier()
        time.sleep(0.5)
        eng.close()
    finally:
        dist.destroy_process_group()


def test_tp2_released_widths_vs_oracle_on_wprime(run, oracle):
    import torch.multiprocessing as mp
    world = 2
    ret = mp.Manager().dict()
    mp.spawn(_tp_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert {ret[r][0] for r in range(world)} == {"ipc"}, {r: ret[r][0] for r in range(world)}
    assert all(ret[r][3] == 0 for r in range(world))
    assert ret[1][1] == ret[0][1] and np.array_equal(ret[1][2], ret[0][2]), "ranks differ"
    ref = oracle[0]
    err = float(np.abs(ret[0][2] - ref["logits"]).max())
    print(f"TP = 2 ids {ret[0][1]}, TP = 1 {run['toks']}, oracle {ref['logits'].argmax(-1).tolist()}, max |logit diff| {err:.2e}")
    assert ret[0][1] == ref["logits"].argmax(-1).tolist()
    assert err < 1e-3
