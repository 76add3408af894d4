"""The logit rules contract without a GPU: its numpy restatement (tests/logit_rules_ref.py) against third parties — the penalty
arithmetic against transformers' RepetitionPenaltyLogitsProcessor and vLLM's apply_penalties formula, the log-probabilities against
torch.log_softmax in float64 —, SamplingParams' ranges and mapping, the ctypes mirrors, and what the C layer refuses before a launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import logit_rules_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def _rows(V, seed):
    rng = np.random.default_rng(seed)
    row = (rng.standard_normal(V) * 3).astype(np.float32)
    row[rng.integers(0, V, 9)] = 0.0
    row[rng.integers(0, V, 3)] = -0.0
    row[rng.integers(0, V, 3)] = np.inf
    row[rng.integers(0, V, 3)] = -np.inf
    return row, rng


@pytest.mark.parametrize("r", [0.5, 1.0, 1.3, 2.0])
def test_repetition_penalty_equals_transformers_bit_for_bit(r):
    import torch
    import transformers as tf          # a missing library fails the test: it is what the restatement is pinned to
    for V in (7, 1000, 4001):
        row, rng = _rows(V, V)
        hist = rng.integers(0, V, 60)
        exp = tf.RepetitionPenaltyLogitsProcessor(penalty=float(r))(torch.from_numpy(hist)[None], torch.from_numpy(row.copy())[None])[0].numpy()
        # HF penalises every id of input_ids alike: prompt ids, output ids, or both
        for seen in (ref.seen_table(V, prompt_ids=hist), ref.seen_table(V, output_ids=hist),
                     ref.seen_table(V, prompt_ids=hist[:40], output_ids=hist[30:])):
            got = ref.penalise(row, seen, r=r)
            assert np.array_equal(_bits(got), _bits(exp)), (V, r)
        assert np.array_equal(_bits(ref.penalise(row, ref.seen_table(V), r=r)), _bits(row))      # no history: untouched


def test_frequency_and_presence_equal_the_vllm_formula():
    """vLLM apply_penalties after the repetition step: logits -= frequency * counts; logits -= presence * (counts > 0), evaluated
    one fp32 operation at a time (presence >= 0 here: with a negative one vLLM's `- p * 0` turns a -0 logit into +0)."""
    for V in (5, 1000):
        row, rng = _rows(V, 100 + V)
        out = np.concatenate([rng.integers(0, V, 80), np.full(300, 3), np.full(17, 4)])
        prompt = rng.integers(0, V, 30)
        seen = ref.seen_table(V, prompt, out)
        cnt = np.bincount(out, minlength=V).astype(np.float32)
        assert np.array_equal(seen & np.uint32(0x7FFFFFFF), cnt.astype(np.uint32)) and int(seen[3] & np.uint32(0x7FFFFFFF)) >= 300
        for r in (1.0, 1.3):
            for f in (-0.5, 0.0, 0.7):
                for p in (0.0, 1.1):
                    with np.errstate(all="ignore"):
                        x = ref.penalise(row, seen, r=r)                       # step 1 alone (pinned to HF above)
                        x = (x - (np.float32(f) * cnt).astype(np.float32)).astype(np.float32)
                        x = (x - (np.float32(p) * (cnt > 0).astype(np.float32)).astype(np.float32)).astype(np.float32)
                    got = ref.penalise(row, seen, r=r, f=f, p=p)
                    assert np.array_equal(_bits(got), _bits(x)), (V, r, f, p)
    nan = ref.penalise(np.array([np.nan, 1.0], np.float32), ref.seen_table(2, [0], [0, 1]), r=1.3, f=0.7, p=1.1)
    assert np.isnan(nan[0]) and nan[1] == np.float32(np.float32(np.float32(1.0) / np.float32(1.3)) - np.float32(0.7)) - np.float32(1.1)


def test_logprobs_equal_torch_log_softmax_in_float64():
    import torch
    for V in (1, 2, 65, 1025, 51760):
        rng = np.random.default_rng(V)
        for scale in (0.3, 3.0, 30.0):
            row = (rng.standard_normal(V) * scale).astype(np.float32)
            exp = torch.log_softmax(torch.from_numpy(row).double(), dim=0).float().numpy()
            got = ref.log_softmax(row)
            assert np.array_equal(got, exp), (V, scale, np.abs(got - exp).max())
            tok = int(rng.integers(0, V))
            lp, ids, top = ref.logprobs(row, tok, 5)
            k = min(5, V)
            order = np.argsort(-row.astype(np.float64), kind="stable")[:k]
            assert lp == exp[tok] and ids[:k].tolist() == order.tolist() and np.array_equal(top[:k], exp[order])
            assert (ids[k:] == -1).all() and np.isneginf(top[k:]).all()


def test_logprob_restatement_degenerate_rows():
    row = np.array([1.0, np.nan, 2.0, 2.0, -np.inf, -0.0, 0.0], np.float32)
    lp, ids, top = ref.logprobs(row, 1, 20)
    assert np.isneginf(lp) and ids[:7].tolist() == [2, 3, 0, 5, 6, 1, 4] and (ids[7:] == -1).all()      # ties by id, NaN as -inf
    assert top[0] == top[1] and np.isneginf(top[5:]).all()
    for fill in (np.nan, -np.inf):
        lp, ids, top = ref.logprobs(np.full(9, fill, np.float32), 0, 3)
        assert np.isneginf(lp) and ids.tolist() == [0, 1, 2] and np.isneginf(top).all()
    lp, ids, top = ref.logprobs(np.array([0.5], np.float32), 0, 0)
    assert lp == 0.0 and ids.shape == (0,) and top.shape == (0,)


def test_sampling_params_ranges_and_mapping():
    from vita_amd.serving import CompletionOutput, SamplingParams, completion, rules_of
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=2.5), dict(repetition_penalty=float("nan")),
               dict(presence_penalty=2.1), dict(presence_penalty=-2.1), dict(frequency_penalty=3.0), dict(frequency_penalty=float("inf")),
               dict(logprobs=-1), dict(logprobs=21)):
        with pytest.raises(ValueError):
            SamplingParams(**kw)
    assert rules_of(SamplingParams()) is None and rules_of(None) is None
    assert rules_of(SamplingParams(temperature=0.7, seed=1, top_k=5)) is None          # sampling alone arms no rules
    assert rules_of(SamplingParams(repetition_penalty=1.3)) == dict(repetition_penalty=1.3, presence_penalty=0.0, frequency_penalty=0.0,
                                                                    logprobs=-1)
    assert rules_of(SamplingParams(presence_penalty=-2.0, frequency_penalty=2.0, repetition_penalty=2.0, logprobs=20)) == dict(
        repetition_penalty=2.0, presence_penalty=-2.0, frequency_penalty=2.0, logprobs=20)
    assert rules_of(SamplingParams(logprobs=0)) == dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logprobs=0)
    c = CompletionOutput(0, "", [1])
    assert c.logprobs is None and c.cumulative_logprob is None
    c = completion(0, "ab", [4, 9], "stop", [{4: -0.5, 7: -1.0}, {2: -0.25, 9: -2.0}, {1: 0.0}])
    assert c.logprobs == [{4: -0.5, 7: -1.0}, {2: -0.25, 9: -2.0}] and c.cumulative_logprob == -2.5


def test_engine_keywords_reach_the_struct():
    from vita_amd import _lib
    from vita_amd.engine import MixtralEngine
    r, ids, n_p, n_o = MixtralEngine._rules_args(1.3, 0.4, 0.6, 5, [7, 8, 9], [1, 1])
    assert (r.repetition_penalty, r.presence_penalty, r.frequency_penalty, r.logprobs) == (
        np.float32(1.3), np.float32(0.4), np.float32(0.6), 5)
    assert list(ids) == [7, 8, 9, 1, 1] and (n_p, n_o) == (3, 2)
    r = _lib.logit_rules()
    assert (r.repetition_penalty, r.presence_penalty, r.frequency_penalty, r.logprobs) == (1.0, 0.0, 0.0, -1)


def test_logit_rules_struct_matches_the_header(tmp_path):
    from vita_amd import _lib
    cls = _lib.LogitRules
    lines = ['printf("%zu", sizeof(vh_logit_rules));'] + [f'printf(" %zu", offsetof(vh_logit_rules, {f}));' for f, _ in cls._fields_]
    lines += ['printf(" %zu %zu %zu", offsetof(vh_mixtral_cfg, penalty_tables), offsetof(vh_mixtral_cfg, max_logprobs), sizeof(vh_mixtral_cfg));']
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vita_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, *offs = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert ctypes.sizeof(cls) == int(size)
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == [int(o) for o in offs[:4]]
    cfg = _lib.MixtralCfg
    assert [cfg.penalty_tables.offset, cfg.max_logprobs.offset, ctypes.sizeof(cfg)] == [int(o) for o in offs[4:]]
    assert cfg._fields_[-2:] == [("penalty_tables", ctypes.c_int), ("max_logprobs", ctypes.c_int)]      # at the END of the struct


def _cfg(**kw):
    from vita_amd import _lib
    base = dict(hidden=128, n_layers=2, n_q_heads=2, n_kv_heads=1, head_dim=128, inter=128, n_experts=4, top_k=2, vocab=1000,
                rms_eps=1e-5, max_ctx=256, max_prefill=64, max_new=32, tp_rank=0, tp_world=1)
    base.update(kw)
    return _lib.MixtralCfg(**base)


def test_workspace_grows_only_with_the_new_fields():
    from vita_amd import _lib
    lib = _lib.load()
    size = lambda **kw: lib.vh_mixtral_workspace_bytes(ctypes.byref(_cfg(**kw)))
    base = size()
    assert base > 0 and size(penalty_tables=0, max_logprobs=0) == base
    assert base + 4 * 1000 <= size(penalty_tables=1) <= base + 4 * 1000 + 1024
    lp = size(max_logprobs=5)
    assert base + 32 * 4 * (1 + 2 * 5) <= lp <= base + 32 * 4 * (1 + 2 * 5) + 1024
    assert size(max_seqs=3, penalty_tables=1) - size(max_seqs=3) >= 4 * 4 * 1000          # one table per slot + the engine's
    assert size(max_logprobs=21) == 0 and b"max_logprobs" in lib.vh_last_error()
    assert size(max_logprobs=-1) == 0


def test_c_layer_refuses_bad_arguments_before_any_launch():
    """what is checked before a launch needs no GPU: a null engine, non-finite or non-positive penalties, K outside [0, 20], missing
    buffers.  The pointers below are never dereferenced."""
    from vita_amd import _lib
    lib = _lib.load()
    VH_E_ARG = -2
    r = _lib.logit_rules(1.3, 0.0, 0.0, 5)
    ids = (ctypes.c_int * 1)(0)
    assert lib.vh_mixtral_set_logit_rules(None, ctypes.byref(r), ids, 1, 0) == VH_E_ARG and b"null engine" in lib.vh_last_error()
    assert lib.vh_mixtral_seq_set_logit_rules(None, 0, ctypes.byref(r), ids, 1, 0) == VH_E_ARG and b"null engine" in lib.vh_last_error()
    for fn in ("vh_mixtral_logprobs_token", "vh_mixtral_logprobs_top_ids", "vh_mixtral_logprobs_top", "vh_mixtral_seen"):
        assert getattr(lib, fn)(None) is None
    for fn in ("vh_mixtral_seq_logprobs_token", "vh_mixtral_seq_logprobs_top_ids", "vh_mixtral_seq_logprobs_top", "vh_mixtral_seq_seen"):
        assert getattr(lib, fn)(None, 0) is None
    fake = ctypes.c_void_p(4096)

    def rows(rules, K=0, logits=fake, lp=None, tokens=None, pen=fake, n=1, V=8):
        return lib.vh_logit_rules_rows(logits, V, n, V, ctypes.byref(rules) if rules is not None else None, None, pen, tokens, lp, None,
                                       None, K, None)

    for bad in (dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")), dict(repetition_penalty=0.0),
                dict(repetition_penalty=-1.0), dict(presence_penalty=float("inf")), dict(frequency_penalty=float("nan"))):
        assert rows(_lib.logit_rules(**bad)) == VH_E_ARG, bad
        assert b"penalty" in lib.vh_last_error()
    ok = _lib.logit_rules(1.3, 0.1, 0.2, -1)
    assert rows(ok, K=21) == VH_E_ARG and b"K 21" in lib.vh_last_error()
    assert rows(ok, K=-1) == VH_E_ARG
    assert rows(ok, logits=None) == VH_E_ARG
    assert rows(None) == VH_E_ARG                                     # penalised_out without rules
    assert rows(ok, K=5, lp=fake, tokens=fake) == VH_E_ARG            # K > 0 without the top-K buffers
    assert rows(ok, K=0, lp=fake, tokens=None) == VH_E_ARG            # logprobs without tokens
    assert rows(ok, n=0) == -1 and rows(ok, V=0) == -1                # VH_E_SHAPE


def test_async_engine_carries_logprobs_and_releases_them(monkeypatch):
    """AsyncLLMEngine on a scripted engine: cumulative .logprobs / .cumulative_logprob per event, the rules and the prompt set reach
    seq_set_logit_rules, and ContinuousBatcher.logprobs is empty once every request has finished, failed or been left early."""
    import asyncio
    import time
    from tests.scripted_engine import FakeLLM, ScriptedEngine, _expected, no_cuda_sync
    from vita_amd.serving import AsyncLLMEngine, SamplingParams, rules_of
    no_cuda_sync(monkeypatch)
    K = ScriptedEngine.K              # its logprobs(): top-K ids token + 1 .. token + K at -(id + 1/2), the chosen id at -(token + 1/4)
    llm = FakeLLM()
    llm.model.engine = eng = ScriptedEngine(64 * 16, 3, max_new=64, batch=False, sharing=False)
    prepare = llm._prepare

    def _prepare(inputs, sp):
        req = prepare(inputs, sp)
        if len(req["ids"]) > 90:
            raise ValueError("too long")
        req.update(rules=rules_of(sp), prompt_set=sorted(set(req["ids"])))
        return req
    llm._prepare = _prepare
    engine = AsyncLLMEngine(llm, max_num_seqs=3, window=1)
    sp = SamplingParams(max_tokens=9, logprobs=K, frequency_penalty=0.5)

    async def full(rid, ids):
        seen = []
        async for out in engine.generate({"prompt_token_ids": ids}, sp, request_id=rid):
            seen.append(out.outputs[0])
        return seen

    async def early(rid, ids):
        async for out in engine.generate({"prompt_token_ids": ids}, SamplingParams(max_tokens=60, logprobs=K), request_id=rid):
            return len(out.outputs[0].logprobs)

    async def failing():
        with pytest.raises(ValueError):
            async for _ in engine.generate({"prompt_token_ids": [1] * 91}, sp, request_id="bad"):
                pass

    async def main():
        return await asyncio.gather(full("a", [1, 2, 3]), full("b", [4, 5]), early("c", [6, 7]), failing())

    a, b, n_c, _ = asyncio.run(main())
    for seen, ids in ((a, [1, 2, 3]), (b, [4, 5])):
        last = seen[-1]
        assert last.token_ids == _expected(ids, 9) and len(last.logprobs) == 9
        for o in seen:                                                                          # cumulative, aligned with the ids
            assert len(o.logprobs) == len(o.token_ids)
            for t, d in zip(o.token_ids, o.logprobs):
                assert list(d) == [t + 1, t + 2, t + 3, t] and d[t] == -t - 0.25 and d[t + 1] == -(t + 1.5)
            assert o.cumulative_logprob == sum(-t - 0.25 for t in o.token_ids)
    assert n_c >= 1
    armed = [(s, list(prompt), list(out), kw) for _, s, prompt, out, kw in eng.trace("set_logit_rules")]
    assert {tuple(x[1]) for x in armed} >= {(1, 2, 3), (4, 5)} and all(x[2] == [] for x in armed)
    assert all(x[3] == dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.5, logprobs=K) for x in armed[:2])
    for _ in range(200):
        if not engine.batcher.has_work() and not eng.seqs:
            break
        time.sleep(0.01)
    assert not engine.batcher.has_work()
    assert engine.batcher.logprobs == {}, list(engine.batcher.logprobs)
    engine.shutdown()
