"""GPU parity of the Mixtral engine (prefill + greedy decode through the C ABI) against the fp32
numpy oracle on the same seeded synthetic weights.  North-star bar (BASELINE.json): greedy token
ids bit-exact, logits within 1e-3 (fp32)."""
import numpy as np
import pytest
import torch

from oracle import mixtral as om
from tests.util import assert_close, to_np
from vita_amd.checkpoint import pack_mixtral, synth_state_dict
from vita_amd.config import TextConfig, VitaConfig

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3


def _run(dev, cfg, S, n_new, seed=0, nsplit=0, max_ctx=None, chunked=False, hid_scaled=False):
    from vita_amd.engine import MixtralEngine
    sd = synth_state_dict(cfg, seed=seed, parts=("text",))
    rng = np.random.default_rng(seed + 100)
    ids_in = rng.integers(3, cfg.text.vocab_size, size=S)
    emb = sd["model.embed_tokens.weight"][ids_in]
    orc = om.MixtralOracle(sd, cfg.text)
    ref_ids, ref_lg = orc.greedy(emb, n_new)
    orc.reset()
    _, ref_hid = orc.forward(emb, want_hidden=True)

    eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_ctx=max_ctx or (S + n_new + 8), max_prefill=S,
                        max_new=n_new + 4, nsplit=nsplit, logit_rows=(n_new + 4) if chunked else 0)
    logits, hid = eng.prefill(torch.from_numpy(emb).to(dev), want_hidden=True)
    torch.cuda.synchronize()
    for l in range(cfg.text.num_hidden_layers):
        # hidden states reach |x| ~ 12 at the real width; the prefill attention runs on bf16 x 3 MFMAs (products exact to 2^-17
        # like the GEMMs): max error 2.0-2.8e-4 against 1.2-1.5e-4 with the fp32-MFMA kernel (profiles/debug_tol.py)
        # hid_scaled: longer prompts / deeper stacks at the real width (|x| ~ 17 after two layers): the bar of tests/test_realgeom_gpu.py,
        # 3e-4 of the tensor's largest magnitude + 1e-3 relative (r05: 6.6e-4 at S = 300, layer 1, against atol 4e-4)
        atol, rtol = (3e-4 * float(np.abs(ref_hid[l]).max()), 1e-3) if hid_scaled else (4e-4, 1e-4)
        assert_close(f"prefill hidden after layer {l}", to_np(hid[l]), ref_hid[l], atol=atol, rtol=rtol)
    got_lg = [to_np(logits).copy()]
    if chunked:
        eng.decode(n_new - 1)  # one C call, no host interaction; scores come from the logits history
        torch.cuda.synchronize()
        got_lg = [to_np(eng.logits_all[i]).copy() for i in range(n_new)]
    else:
        for _ in range(n_new - 1):
            eng.decode(1)
            torch.cuda.synchronize()
            got_lg.append(to_np(eng.logits).copy())
    torch.cuda.synchronize()
    got_ids = eng.generated()
    print("oracle ids:", ref_ids)
    print("device ids:", got_ids)
    for i, lg in enumerate(got_lg):
        assert_close(f"logits step {i}", lg, ref_lg[i], atol=LOGIT_TOL)
    assert got_ids == ref_ids, "greedy token ids differ from the oracle"
    assert int(eng.counters[0].item()) == S + n_new - 1
    eng.close()


def test_tiny_prefill_decode(dev):
    _run(dev, VitaConfig.tiny(), S=40, n_new=16)


def test_tiny_multi_split_and_long_ctx(dev):
    """context crosses several 64-key tiles and several KV splits."""
    _run(dev, VitaConfig.tiny(), S=150, n_new=12, nsplit=4, max_ctx=400)


def test_tiny_decode_batch_call(dev):
    """all decode steps enqueued by a single vh_mixtral_decode call."""
    _run(dev, VitaConfig.tiny(), S=17, n_new=24, chunked=True)


@pytest.mark.parametrize("fused", [0, 1])
def test_decode_schedules_vs_oracle(dev, fused):
    """both forms of a decode layer's attention block against the oracle on the GQA 4 : 1 / 8-expert geometry: 1 = ONE launch
    (k_dec_ablk: fused-QKV rows, attention tiles and O rows as blocks of one grid, tagged granules between them — the default), 0 =
    three launches (the kernels of r01-r05)."""
    from vita_amd import _lib
    cfg = VitaConfig.tiny()
    cfg.text = TextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                          intermediate_size=1024, num_local_experts=8, vocab_size=2000)
    _lib.tune("dec_fused", fused)
    try:
        _run(dev, cfg, S=130, n_new=12, seed=4, chunked=True)
    finally:
        _lib.tune("dec_fused", -1)


def test_group4_experts8(dev):
    """GQA group of 4 and 8 experts (the released model's ratios) at reduced width."""
    cfg = VitaConfig.tiny()
    cfg.text = TextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                          intermediate_size=1024, num_local_experts=8, vocab_size=2000)
    _run(dev, cfg, S=70, n_new=10, seed=3)


@pytest.mark.parametrize("fuse_rows", [1, 0])
def test_real_width_one_layer(dev, fuse_rows):
    """Real Mixtral-8x7B layer geometry (4096 / 32 heads / 8 kv / 14336 / 8 experts), 1 layer,
    reduced vocab: exercises the exact kernel instantiations the benchmark runs.  fuse_rows = 0: the separate slab-sum /
    combine / plane-split launches — the path EVERY tensor-parallel rank takes — at the real width, where the k_gemm_sp
    instantiations differ from the H = 512 geometry of test_alternative_paths."""
    from vita_amd import _lib
    cfg = VitaConfig.tiny()
    cfg.text = TextConfig(num_hidden_layers=1, vocab_size=4096)
    _lib.tune("prefill_fuse_rows", fuse_rows)
    try:
        _run(dev, cfg, S=48, n_new=6, seed=5)
    finally:
        _lib.tune("prefill_fuse_rows", 1)


@pytest.mark.parametrize("fuse_rows", [0, 1])
def test_real_width_two_layers_longer_prompt(dev, fuse_rows):
    """both row-update paths at a row count that takes the two-m-tile streaming GEMM and a K split chosen on the device
    (S = 300: ~75 rows per expert), two layers so that layer 1 consumes what layer 0's launches wrote (0 = the separate
    slab-sum / combine / plane-split launches of every tensor-parallel rank)."""
    from vita_amd import _lib
    cfg = VitaConfig.tiny()
    cfg.text = TextConfig(num_hidden_layers=2, vocab_size=4096)
    _lib.tune("prefill_fuse_rows", fuse_rows)
    try:
        _run(dev, cfg, S=300, n_new=4, seed=6, hid_scaled=True)
    finally:
        _lib.tune("prefill_fuse_rows", 1)



@pytest.mark.parametrize("shard_vocab", [True, False])
def test_tp2_two_ranks_on_one_gpu(dev, shard_vocab):
    """(restored in r05: ADVICE r04 — nothing else covers vh_mixtral_set_allreduce, the callback collective that
    setup_tensor_parallel falls back to when IPC and RCCL bring-up lose.)
    Tensor parallel without a second GPU: both ranks' engines live on this GPU and
    run in lock-step from two host threads; the all-reduce hook sums the two partial buffers.
    Checks the sharded packing, the per-rank kernels at sliced shapes (1 kv head, I/2) and the
    placement of the two collectives per layer against the unsharded oracle.  shard_vocab: the LM head holds half
    of the vocabulary per rank and the (max, index) candidates take one more all-reduce per forward
    (ParallelLMHead + logits gather of the reference's vLLM flavour, vllm_file/mixtral.py:939-951)."""
    import ctypes as C
    import threading
    from vita_amd import _lib
    from vita_amd.engine import MixtralEngine
    cfg = VitaConfig.tiny()
    S, n_new, world = 37, 9, 2
    sd = synth_state_dict(cfg, seed=11, parts=("text",))
    rng = np.random.default_rng(111)
    emb = sd["model.embed_tokens.weight"][rng.integers(3, cfg.text.vocab_size, size=S)]
    ref_ids, ref_lg = om.MixtralOracle(sd, cfg.text).greedy(emb, n_new)

    engs = [MixtralEngine(cfg, pack_mixtral(sd, cfg, dev, rank=r, world=world, shard_vocab=shard_vocab), dev, max_ctx=S + n_new + 8,
                          max_prefill=S, max_new=n_new + 4, rank=r, world=world, logit_rows=n_new + 4)
            for r in range(world)]
    bar = threading.Barrier(world)
    slots, n_calls, errs = [None] * world, [0] * world, []

    def make_cb(r):
        eng = engs[r]
        base = eng.workspace.data_ptr()

        def cb(_user, ptr, count, _stream):
            try:
                torch.cuda.synchronize()
                slots[r] = eng.workspace[ptr - base: ptr - base + 4 * count].view(torch.float32)
                n_calls[r] += 1
                bar.wait(timeout=60)
                if r == 0:
                    tot = slots[0] + slots[1]
                    slots[0].copy_(tot); slots[1].copy_(tot)
                    torch.cuda.synchronize()
                bar.wait(timeout=60)
                return 0
            except Exception as e:  # a broken barrier must not hang the other rank
                errs.append(repr(e))
                bar.abort()
                return -1
        return _lib.ALLREDUCE_FN(cb)

    cbs = [make_cb(r) for r in range(world)]
    for r in range(world):
        _lib.check(_lib.load().vh_mixtral_set_allreduce(engs[r].h, cbs[r], None), "set_allreduce")
    x = torch.from_numpy(emb).to(dev)

    def work(r):
        try:
            engs[r].prefill(x, gather_logits=False)    # threads, no process group: the rows are summed below
            engs[r].decode(n_new - 1)
        except Exception as e:
            errs.append(repr(e))
            bar.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    torch.cuda.synchronize()
    assert not errs, errs
    L = cfg.text.num_hidden_layers
    assert n_calls == [(2 * L + (1 if shard_vocab else 0)) * n_new] * world   # 2 collectives per layer (+ candidates) per forward
    for r in range(world):
        assert engs[r].generated() == ref_ids, f"rank {r} tokens differ from the unsharded oracle"
    for i in range(n_new):
        if shard_vocab:      # each rank kept its slice of the row (zeros elsewhere): the sum is the full row
            assert_close(f"logits step {i}", to_np(engs[0].logits_all[i] + engs[1].logits_all[i]), ref_lg[i], atol=LOGIT_TOL)
            half = (cfg.text.vocab_size + 1) // 2
            assert float(engs[0].logits_all[i][half:].abs().max()) == 0.0 and float(engs[1].logits_all[i][:half].abs().max()) == 0.0
        else:
            for r in range(world):
                assert_close(f"rank {r} logits step {i}", to_np(engs[r].logits_all[i]), ref_lg[i], atol=LOGIT_TOL)
    [e.close() for e in engs]


def test_rccl_binding_single_rank(dev):
    """(restored in r05: ADVICE r04 — the only test of vh_rccl_unique_id / vh_mixtral_init_rccl, setup_tensor_parallel's second choice.)
    The native RCCL path (dlopen'ed librccl, ncclCommInitRank by-value id, ncclAllReduce on the
    engine's stream) exercised with a 1-rank communicator: an all-reduce over one rank is the
    identity, so tokens must still match the oracle."""
    import ctypes as C
    from vita_amd import _lib
    from vita_amd.engine import MixtralEngine
    cfg = VitaConfig.tiny()
    S, n_new = 21, 5
    sd = synth_state_dict(cfg, seed=12, parts=("text",))
    emb = sd["model.embed_tokens.weight"][np.random.default_rng(5).integers(3, cfg.text.vocab_size, size=S)]
    ref_ids, _ = om.MixtralOracle(sd, cfg.text).greedy(emb, n_new)
    eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev), dev, max_ctx=S + n_new + 8, max_prefill=S, max_new=n_new + 4)
    uid = C.create_string_buffer(128)
    _lib.check(_lib.load().vh_rccl_unique_id(uid), "vh_rccl_unique_id")
    eng.use_rccl(bytes(uid.raw))
    _lib.tune("force_allreduce", 1)
    try:
        eng.prefill(torch.from_numpy(emb).to(dev))
        eng.decode(n_new - 1)
        torch.cuda.synchronize()
        assert eng.generated() == ref_ids
    finally:
        _lib.tune("force_allreduce", 0)
        eng.close()



@pytest.mark.parametrize("knob,value", [("prefill_attn_gemm", 1), ("prefill_fuse_rows", 0), ("attn_impl", 2), ("attn_fa", 2), ("attn_fa", 0)])
def test_alternative_paths(dev, knob, value):
    """the non-default code paths a caller can still reach stay correct: the general GEMM kernel under the attention
    projections (the automatic fallback for geometries the streaming kernel does not take), the separate slab-sum / combine /
    plane-split launches (what runs under tensor parallelism; default on one rank: folded into the norm and attention kernels),
    the fp32-MFMA attention kernel, the flash-form prefill attention forced at this small geometry (8 : 2 heads) and switched off.  (r04 removed the variants that had lost their measurements.)"""
    from vita_amd import _lib
    cfg = VitaConfig.tiny()
    cfg.text = TextConfig(hidden_size=512, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                          intermediate_size=1024, num_local_experts=8, vocab_size=2000)
    default = {"prefill_attn_gemm": 0, "prefill_fuse_rows": 1, "attn_impl": 0, "attn_fa": 1}[knob]
    _lib.tune(knob, value)
    try:
        _run(dev, cfg, S=200, n_new=8, seed=9)
    finally:
        _lib.tune(knob, default)


def test_attention_rows_wider_than_moe_rows(dev):
    """nq * head_dim (32 x 128 = 4096) wider than the MoE's 2 x intermediate (2048): the prefill's bf16 plane buffers carry both the
    attention output rows (O projection input) and the expert h rows, and must be sized for the wider of the two (they were sized for
    the MoE alone: the attention planes ran over into the residual rows; every hidden state wrong by O(1))."""
    cfg = VitaConfig.tiny()
    cfg.text = TextConfig(hidden_size=1024, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=8,
                          intermediate_size=1024, num_local_experts=8, vocab_size=2000)
    _run(dev, cfg, S=70, n_new=4, seed=2)
