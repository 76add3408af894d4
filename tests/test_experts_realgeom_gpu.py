"""Quantised experts — int8 and MXFP4 — at the RELEASED widths (H 4096, I 14336, 32 / 8 heads, vocab 51760)
on a few layers of synthetic weights (counter-based generator: the same values on the device and in the layer-streamed oracle),
against the fp32 oracle evaluated on the dequantised weights w' (int8: w' = q s, tests/q8_ref.py; MXFP4: w' = e2m1(code) 2^(byte - 127),
tests/q4_ref.py; both wrap oracle.stream's weight buffers).  The same cases and bars for each format:
  * one request, S = 552 + 8 greedy steps: ids ==, every router decision of the prompt ==, logits within 1e-3;
  * six sequences through vh_mixtral_seq_decode with batch_moe_min 3 (the format's streaming MoE GEMM) and 0 (per-sequence GEMVs);
  * TP = 2: two engine processes on one GPU over the library's IPC all-reduce (int8: w2 shards under full-row scales; MXFP4: w2
    shards are slices of the codes and the scales; the tensor-parallel prefill's column halves), ids == the same oracle's, logits
    within 1e-3."""
import time
from typing import Any, NamedTuple

import numpy as np
import pytest
import torch

from oracle import stream
from tests import q4_ref, q8_ref
from tests.ranks import TP_UNSET, greedy_tp_run, run_ranks
from vita_amd import _lib
from vita_amd.checkpoint import synth_mixtral_device
from vita_amd.config import VitaConfig

pytestmark = pytest.mark.gpu
SEED, S, T_NEW = 0, 552, 8
SEQ_LENS, SEQ_STEPS = (17, 40, 64, 9, 33, 50), 6


class Format(NamedTuple):
    name: str            # the engine's `experts` value
    ref: Any             # the module whose streamed_experts_wprime() puts w' into the oracle
    layers: int


# MXFP4 has 3 layers: quantising w' in numpy costs more than int8's, that format keeps its wall time
FORMATS = [Format("int8", q8_ref, 4), Format("mxfp4", q4_ref, 3)]


@pytest.fixture(scope="module", params=FORMATS, ids=lambda f: f.name)
def fmt(request):
    """module scope: pytest runs every test of one format, tears its `run` and `oracle` down, then builds the next format's."""
    return request.param


def _cfg(layers):
    cfg = VitaConfig()
    cfg.text.num_hidden_layers = layers
    return cfg


def _prompt_ids(V):
    rng = np.random.default_rng(5)
    return rng.integers(3, V, size=S).tolist(), [rng.integers(3, V, size=n).tolist() for n in SEQ_LENS]


@pytest.fixture(scope="module")
def run(dev, fmt):
    from vita_amd.engine import MixtralEngine
    cfg = _cfg(fmt.layers)
    t = cfg.text
    ids, prompts = _prompt_ids(t.vocab_size)
    packed = synth_mixtral_device(cfg, dev, seed=SEED, experts=fmt.name)
    emb = lambda x: packed["embed"][torch.tensor(x, device=dev)].float()
    eng = MixtralEngine(cfg, packed, dev, max_prefill=S, max_new=T_NEW + 4, logit_rows=T_NEW + 4)
    assert eng.experts == fmt.name
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
def oracle(run, fmt):
    """ONE teacher-forced pass of the streamed oracle on w' over the request and the six sequences (prompt + the device's tokens)."""
    t = run["cfg"].text
    rows = lambda x: stream.embed_rows(t, x, SEED)
    embs = [np.concatenate([rows(run["ids"]), rows(run["toks"][:-1])], 0)]
    embs += [np.concatenate([rows(p), rows(st[:-1])], 0) for p, st in zip(run["prompts"], run["seq_toks"][3])]
    t0 = time.time()
    with fmt.ref.streamed_experts_wprime():
        ref = stream.forward_many(t, SEED, embs, n_layers=fmt.layers, logits_from=[S - 1] + [len(p) - 1 for p in run["prompts"]])
    print(f"[{fmt.name} realgeom] oracle ({fmt.layers} layers, {sum(e.shape[0] for e in embs)} rows) in {time.time() - t0:.1f}s")
    return ref


def test_released_widths_request_vs_oracle_on_wprime(run, oracle, fmt):
    ref = oracle[0]
    r_dev, r_ref = np.sort(run["route"], -1), np.sort(ref["route"][:, :S], -1)
    mism = np.argwhere((r_dev != r_ref).any(-1))
    print(f"router top-2 sets: {r_dev.shape[0] * S} decisions, {len(mism)} differ", mism[:5].tolist())
    assert r_dev.shape == (fmt.layers, S, 2) and len(mism) == 0
    ref_ids = ref["logits"].argmax(-1).tolist()
    err = float(np.abs(run["logits"] - ref["logits"]).max())
    print("device ids", run["toks"], "oracle ids", ref_ids, f"max |logit diff| {err:.2e}")
    assert run["toks"] == ref_ids
    assert err < 1e-3


def test_released_widths_six_sequences_vs_oracle_on_wprime(run, oracle):
    for i, ref in enumerate(oracle[1:]):
        ref_ids = ref["logits"].argmax(-1).tolist()
        assert run["seq_toks"][3][i] == ref_ids, (i, run["seq_toks"][3][i], ref_ids)   # the format's streamed MoE GEMM (n >= 3)
        assert run["seq_toks"][0][i] == ref_ids, (i, run["seq_toks"][0][i], ref_ids)   # per-sequence GEMVs of the format


def _tp_worker(ctx, experts, layers):
    """one rank of TP = 2 at the released shard widths (16 q + 4 KV heads, 7168 columns of every expert, half the vocabulary)"""
    import torch.distributed as dist
    from vita_amd.engine import MixtralEngine
    from vita_amd.parallel import setup_tensor_parallel
    rank, world, dev = ctx.rank, ctx.world, ctx.dev
    cfg = _cfg(layers)
    ids, _ = _prompt_ids(cfg.text.vocab_size)
    packed = synth_mixtral_device(cfg, dev, seed=SEED, rank=rank, world=world, experts=experts)
    eng = MixtralEngine(cfg, packed, dev, max_prefill=S, max_new=T_NEW + 4, logit_rows=T_NEW + 4, rank=rank, world=world)
    ctx.defer(eng.close)
    assert eng.experts == experts and eng.c.inter == 14336 // world
    name = setup_tensor_parallel(eng, rank, world, dev, backend="gloo", collective="ipc")
    return greedy_tp_run(eng, packed["embed"][torch.tensor(ids, device=dev)].float(), T_NEW, dist, name)


def test_tp2_released_widths_vs_oracle_on_wprime(run, oracle, fmt):
    world = 2
    ret = run_ranks(_tp_worker, world, fmt.name, fmt.layers, env=TP_UNSET, deadline_s=120)
    assert {ret[r].collective for r in range(world)} == {"ipc"}, {r: ret[r].collective for r in range(world)}
    assert all(ret[r].comm_status == 0 for r in range(world))
    assert ret[1].tokens == ret[0].tokens and np.array_equal(ret[1].logits, ret[0].logits), "ranks differ"
    ref = oracle[0]
    err = float(np.abs(ret[0].logits - ref["logits"]).max())
    print(f"TP = 2 ids {ret[0].tokens}, TP = 1 {run['toks']}, oracle {ref['logits'].argmax(-1).tolist()}, max |logit diff| {err:.2e}")
    assert ret[0].tokens == ref["logits"].argmax(-1).tolist()
    assert err < 1e-3
