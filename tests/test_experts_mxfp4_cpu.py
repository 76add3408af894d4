"""MXFP4 experts without a GPU: the quantisation contract of tests/q4_ref.py on hand-written edge blocks, that w' is
bf16, the error bound, tensor-parallel shards, the argument checks that run before any device work, and the precondition of the
GPU engine tests (the oracle's top-2 gaps on their inputs)."""
import ctypes as C

import numpy as np
import pytest

from tests import mxfp4_cases as mx
from tests import q4_ref
from vita_amd.checkpoint import round_bf16, synth_state_dict

F32 = np.float32


def _block(vals, fill=0.0):
    b = np.full(32, fill, F32)
    b[:len(vals)] = vals
    return b


def _codes(b):
    code, byte = q4_ref.quant_codes(b[None])
    return code[0].tolist(), int(byte[0, 0])


def test_zero_block():
    code, byte = _codes(np.zeros(32, F32))
    assert code == [0] * 32 and byte == 127
    code, byte = _codes(_block([0.0, -0.0]))                           # -0 is a zero: no sign bit, no code 8
    assert code == [0] * 32 and byte == 127


@pytest.mark.parametrize("n", [-20, 0, 3])
def test_ties_to_the_even_code(n):
    X = F32(2.0) ** n                                                  # amax = 4 X -> floor(log2) - 2 = n
    v = [4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 0.5, 1.0, 1.5, 2.0, 3.0]
    b = _block([x * X for x in v] + [-x * X for x in v])
    code, byte = _codes(b)
    assert byte == n + 127
    pos = [6, 0, 2, 2, 4, 4, 6, 1, 2, 3, 4, 5]                        # .25 -> 0, .75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4
    assert code[:12] == pos
    assert code[12:24] == [c | 8 if c else 0 for c in pos]             # the same magnitudes with the sign bit; -0.25 X -> code 0
    assert code[24:] == [0] * 8
    b[0] = 6 * X                                                       # amax = 6 X keeps the scale: 5 X is the tie between 4 and 6
    b[1], b[13] = 5 * X, -5 * X
    code, byte = _codes(b)
    assert byte == n + 127 and code[0] == 7 and code[1] == 6 and code[13] == 14


@pytest.mark.parametrize("n", [-7, 0, 5])
def test_saturation(n):
    X = F32(2.0) ** n
    code, byte = _codes(_block([7 * X, -7 * X, 6.5 * X, 5.5 * X, -5 * X, 4.5 * X]))
    assert byte == n + 127                                             # floor(log2(7 2^n)) = n + 2
    assert code[:6] == [7, 15, 7, 7, 14, 6]                            # 7 and 6.5 saturate at 6; 5.5 -> 6, 5 -> 4 (tie), 4.5 -> 4


@pytest.mark.parametrize("n", [-9, 0, 4])
def test_amax_power_of_two(n):
    a = F32(2.0) ** n                                                  # amax = 2^n -> se = n - 2, amax / X = 4
    code, byte = _codes(_block([a, -a, a / 2, a / 4, a / 8, a / 16, a * F32(0.75)]))
    assert byte == n - 2 + 127
    assert code[:7] == [6, 14, 4, 2, 1, 0, 5]                          # 4, -4, 2, 1, .5, .25 -> 0 (tie to even), 3


def test_clamp_block():
    tiny = F32(2.0) ** -126                                            # the smallest normal bf16: floor(log2) - 2 = -128 -> -125
    code, byte = _codes(_block([tiny, -tiny, 2 * tiny, 3 * tiny]))
    assert byte == 2                                                   # se = -125
    assert code[:4] == [1, 9, 2, 3]                                    # v = .5, -.5, 1, 1.5
    wp = q4_ref.dequant(q4_ref.pack(np.array([code], np.uint8)), np.array([[byte]], np.uint8))[0]
    assert wp[0] == tiny and wp[3] == 3 * tiny
    code, byte = _codes(_block([F32(2.0) ** -124]))                    # just above the clamp: se = -126 -> -125 as well
    assert byte == 2 and code[0] == 4
    nz = np.abs(wp[wp != 0]).view(np.uint32) >> 23
    assert (nz >= 1).all(), "every non-zero w' is a normal number"


def test_outlier_flushes_its_block():
    rng = np.random.default_rng(1)
    b = (rng.standard_normal(64) * 0.02).astype(F32)
    b = round_bf16(b)
    b[5] = 8.0                                                         # X = 2: everything below .5 (= .25 X) becomes 0
    code, byte = q4_ref.quant_codes(b[None])
    assert byte[0, 0] == 1 + 127 and code[0, 5] == 6
    assert (np.delete(code[0, :32], 5) == 0).all()
    assert byte[0, 1] < 127 and (code[0, 32:] & 7).max() >= 6          # the neighbouring block keeps its own scale


def test_no_code_8_and_wprime_is_bf16_and_error_bound():
    rng = np.random.default_rng(3)
    w = round_bf16((rng.standard_normal((64, 4096)) * 0.02).astype(F32))
    w[5, 7] = 0.9
    w[9, 64:96] = 0
    w[11, :32] = -np.abs(w[11, :32])                               # an all-negative block
    code, byte = q4_ref.quant_codes(w)
    assert (code != 8).all() and code.max() <= 15
    codes, scales = q4_ref.quant(w)
    assert codes.dtype == np.uint8 and scales.dtype == np.uint8 and codes.shape == (64, 2048) and scales.shape == (64, 128)
    assert np.array_equal(q4_ref.unpack(codes), code)
    assert (codes[:, 0] & 15 == code[:, 0]).all() and (codes[:, 0] >> 4 == code[:, 1]).all()   # low nibble: the even element
    wp = q4_ref.dequant(codes, scales)
    assert np.array_equal(round_bf16(wp), wp), "w' round-trips through bfloat16"
    # Error bound, element by element (X the block's scale, amax / X in [4, 8) by construction): the magnitudes up to 4 are at most
    # 1 apart, so |w| <= 4 X errs by at most X / 2; between 4 and 6 the step is 2 (5 X -> 4 X is in the contract), at most X; above
    # 6 X the value saturates, less than 2 X.  Block by block this is X / 2 when no element exceeds 4 X, X when amax <= 6 X and 2 X
    # otherwise (the issue's "X / 2 for amax < 6 X" cannot hold for an element between 4 X and 6 X: its own tie 5 -> 4 errs by X).
    X = np.ldexp(F32(1), scales.astype(np.int32) - 127)[..., None]
    a = np.abs(w).reshape(64, 128, 32)
    err = np.abs(w - wp).reshape(64, 128, 32)
    amax = a.max(-1, keepdims=True)
    nz = amax[..., 0] > 0
    assert ((amax[nz] >= 4 * X[nz]) & (amax[nz] < 8 * X[nz])).all()
    low, mid, sat = a <= 4 * X, (a > 4 * X) & (a <= 6 * X), a > 6 * X
    assert low.any() and mid.any() and sat.any()
    assert (err[low] <= np.broadcast_to(X / 2, a.shape)[low]).all()
    assert (err[mid] <= np.broadcast_to(X, a.shape)[mid]).all()
    assert (err[sat] < np.broadcast_to(2 * X, a.shape)[sat]).all()
    assert (err <= 2 * X).all()
    assert (np.sign(wp) * np.sign(w) >= 0).all()


def test_fast_wprime_is_the_contract():
    rng = np.random.default_rng(8)
    w = round_bf16((rng.standard_normal((40, 512)) * 0.02).astype(F32))
    w[0, :32] = 0
    w[1, :32] = _block([x * F32(0.125) for x in (6, 5, -5, 3.5, -2.5, 1.75, 1.25, -0.75, 0.25, -0.25, 7.5, -7)])
    w[2, :32] = _block([F32(2.0) ** -126, -(F32(2.0) ** -125)])
    assert np.array_equal(q4_ref.wprime(w), q4_ref.dequant(*q4_ref.quant(w)))


def test_w2_shards_are_slices():
    rng = np.random.default_rng(4)
    w2 = round_bf16((rng.standard_normal((16, 14336 // 8)) * 0.02).astype(F32))
    w2[3, 1500] = 0.5
    codes, scales = q4_ref.quant(w2)
    wp = q4_ref.dequant(codes, scales)
    I = w2.shape[1]
    for world in (2, 4, 8):
        n = I // world
        assert n % 32 == 0
        parts = []
        for r in range(world):
            c, s = q4_ref.quant(w2[:, r * n:(r + 1) * n])
            assert np.array_equal(c, codes[:, r * n // 2:(r + 1) * n // 2])
            assert np.array_equal(s, scales[:, r * n // 32:(r + 1) * n // 32])
            parts.append(q4_ref.dequant(c, s))
        assert np.array_equal(np.concatenate(parts, 1), wp)


def test_contract_refuses_bad_input():
    with pytest.raises(ValueError):
        q4_ref.quant(np.zeros((2, 48), F32))
    with pytest.raises(ValueError):
        q4_ref.quant(np.full((1, 32), np.inf, F32))


def _cfg():
    from vita_amd._lib import MixtralCfg
    c = MixtralCfg()
    c.hidden, c.n_layers, c.n_q_heads, c.n_kv_heads, c.head_dim = 128, 2, 4, 2, 128
    c.inter, c.n_experts, c.top_k, c.vocab, c.rms_eps = 256, 4, 2, 512, 1e-5
    c.max_ctx, c.max_prefill, c.max_new = 128, 64, 16
    return c


def _lib():
    from vita_amd import _lib
    return _lib.load()                                       # no GPU needed; an unbuilt library or a missing symbol fails the test


def test_create_mxfp4_argument_checks():
    from vita_amd._lib import MixtralExpertsMxfp4, MixtralLayer
    lib = _lib()
    c = _cfg()
    fake = 0x1000                                            # never dereferenced: every case fails before device work
    layers = (MixtralLayer * 2)()
    for L in layers:
        for f, _ in MixtralLayer._fields_:
            if f not in ("w1", "w3", "w2"):
                setattr(L, f, fake)
    ex = (MixtralExpertsMxfp4 * 2)()
    for q in ex:
        for f, _ in MixtralExpertsMxfp4._fields_:
            setattr(q, f, fake)
    args = (fake, fake, fake, fake, fake, fake, 1 << 30)

    def create(ex_arg, cfg=c):
        return lib.vh_mixtral_create_mxfp4(C.byref(cfg), layers, ex_arg, *args)

    assert not create(None)
    assert b"vh_mixtral_create_mxfp4" in lib.vh_last_error() and b"null" in lib.vh_last_error()
    layers[1].w1 = fake                                      # a bf16 expert pointer next to MXFP4 experts
    assert not create(ex)
    assert b"layers[1]" in lib.vh_last_error()
    layers[1].w1 = None
    ex[0].s2 = None                                          # a null scale
    assert not create(ex)
    assert b"experts[0]" in lib.vh_last_error()
    ex[0].s2 = fake
    ex[1].w3 = None                                          # a null code pointer
    assert not create(ex)
    assert b"experts[1]" in lib.vh_last_error()
    ex[1].w3 = fake
    for field, v in (("hidden", 96), ("inter", 224)):        # multiples of 32 but not of 64
        bad = _cfg()
        setattr(bad, field, v)
        assert not create(ex, bad)
        assert b"multiples of 64" in lib.vh_last_error(), lib.vh_last_error()


def test_quant_mxfp4_null_pointers():
    lib = _lib()
    fake = 0x1000
    assert lib.vh_quant_mxfp4(None, 1, 64, 64, 0, 64, fake, 32, fake, 2, None) == -2
    assert lib.vh_quant_mxfp4(fake, 1, 64, 64, 0, 64, None, 32, fake, 2, None) == -2
    assert lib.vh_quant_mxfp4(fake, 1, 64, 64, 0, 64, fake, 32, None, 2, None) == -2
    assert b"vh_quant_mxfp4" in lib.vh_last_error()


def test_gemm_ps_mxfp4_refusals():
    """vh_gemm_ps_mxfp4 refuses these before any device work (VH_E_SHAPE, the reason in vh_last_error).  M = 0 throughout: every
    check runs before the launcher's no-rows return, so a check that stopped refusing would show as rc 0 here without a launch on
    the fake pointers."""
    from vita_amd._lib import GemmPsArgs
    lib = _lib()
    fake = 0x1000

    def call(glu=False, **kw):
        a = GemmPsArgs()
        a.A_hi, a.A_lo, a.lda, a.ldw, a.C, a.ldc = fake, fake, 256, 256, fake, 256
        a.M, a.N, a.K, a.ksplit, a.c_split_stride = 0, 256, 256, 1, 32 * 256
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.vh_gemm_ps_mxfp4(C.byref(a), fake, fake, fake if glu else None, fake if glu else None, None)

    def refused(why, glu=False, **kw):
        rc = call(glu, **kw)
        assert rc == -1, (kw, rc)
        msg = lib.vh_last_error()
        assert msg.startswith(b"vh_gemm_ps_mxfp4: ") and why in msg, (kw, msg)

    refused(b"multiple of 64", K=96)
    refused(b"multiple of 64", K=32)
    refused(b"ldw % 64", ldw=288)                                     # a multiple of 32 only: scale rows would hold half a stage
    refused(b"ldw % 64", ldw=264)
    refused(b"w_group_stride % 64", w_group_stride=256 * 256 + 32)
    refused(b"ldw below K", ldw=128)
    refused(b"above K / 64", ksplit=5)
    refused(b"below -8", ksplit=-9, nslab_out=fake)
    refused(b"needs nslab_out", ksplit=-4)
    for ks in (2, -2):
        split = b"a K split takes a plain GEMM"
        refused(split, glu=True, ksplit=ks, nslab_out=fake)
        for term in ("bias", "scale", "resid"):
            refused(split, ksplit=ks, nslab_out=fake, **{term: fake})
        refused(split, ksplit=ks, nslab_out=fake, act=3)
        refused(split, ksplit=ks, nslab_out=fake, C_hi=fake, C_lo=fake, ldc_split=256)
        refused(split, ksplit=ks, nslab_out=fake, C=None, C_hi=fake, C_lo=fake, ldc_split=256)
    refused(b"more than 8 groups", group_off=fake, ngroups=9)
    refused(b"2^32", ldw=1 << 20, N=4096)
    assert call(W=fake) == -2                                          # args->W next to the MXFP4 weights
    a = GemmPsArgs()
    a.A_hi, a.A_lo, a.lda, a.ldw, a.C, a.ldc, a.N, a.K = fake, fake, 256, 256, fake, 256, 256, 256
    assert lib.vh_gemm_ps_mxfp4(C.byref(a), fake, None, None, None, None) == -2        # codes without scales
    assert lib.vh_gemm_ps_mxfp4(C.byref(a), fake, fake, fake, None, None) == -2        # W_up without S_up


def test_quantization_strings():
    from vita_amd.checkpoint import EXPERT_MODES, pack_mixtral
    from vita_amd.model.builder import load_pretrained_model
    from vita_amd.serving import LLM, AsyncEngineArgs
    assert "mxfp4" in EXPERT_MODES
    for q in ("awq", "fp8", "mxfp4", "experts_fp4"):
        with pytest.raises(ValueError):
            LLM("/nonexistent", quantization=q)
    with pytest.raises(ValueError):
        pack_mixtral({}, mx.VitaConfig.tiny(), "cpu", experts="fp4")
    with pytest.raises(ValueError, match="one"):                       # int8 and MXFP4 together
        load_pretrained_model("/nonexistent", None, "vita", "mixtral-8x7b", load_8bit=True, experts_mxfp4=True)
    with pytest.raises(ValueError, match="one"):
        load_pretrained_model("/nonexistent", None, "vita", "mixtral-8x7b", experts_int8=True, experts_mxfp4=True)
    with pytest.raises(NotImplementedError, match="experts_mxfp4"):   # load_4bit stays refused and says where the 4-bit mode is
        load_pretrained_model("/nonexistent", None, "vita", "mixtral-8x7b", load_4bit=True)
    assert AsyncEngineArgs(model="/nonexistent", quantization="experts_mxfp4").quantization == "experts_mxfp4"


def test_engine_test_inputs_have_a_top2_gap():
    """the precondition of the GPU engine tests: with logits within LOGIT_TOL of the oracle's, ids == is only well posed when the
    oracle's two best logits are at least 2 LOGIT_TOL apart at every generated step (a condition on the inputs, not a measurement)"""
    need = 2 * mx.LOGIT_TOL
    cfg, sd = mx.tiny_text_sd(mx.ENGINE_SEED)
    orc = mx.oracle_on_wprime(sd, cfg)
    gap = mx.greedy(orc, mx.engine_prompt(sd, cfg), mx.ENGINE_NEW)[2]
    print(f"one request (seed {mx.ENGINE_SEED}, S {mx.ENGINE_S}, {mx.ENGINE_NEW} tokens): smallest top-2 gap {gap:.4f}")
    assert gap >= need
    assert mx.SEQ_SEED == mx.ENGINE_SEED
    for i, p in enumerate(mx.seq_prompts(sd, cfg)):
        gap = mx.greedy(orc, p, mx.SEQ_NEW)[2]
        print(f"sequence {i} ({p.shape[0]} rows, {mx.SEQ_NEW} tokens): smallest top-2 gap {gap:.4f}")
        assert gap >= need, i
    sd = synth_state_dict(cfg, seed=mx.CKPT_SEED, rich=True, parts=("text",))      # the text part of tests/tiny_ckpt.py's checkpoint
    orc = mx.oracle_on_wprime(sd, cfg)
    E = sd["model.embed_tokens.weight"]
    for ids, n in ((mx.CKPT_LOAD_IDS, mx.CKPT_LOAD_NEW), (mx.CKPT_LLM_IDS, mx.CKPT_LLM_NEW)):
        gap = mx.greedy(orc, E[ids], n)[2]
        print(f"checkpoint seed {mx.CKPT_SEED}, prompt {ids}: smallest top-2 gap {gap:.4f}")
        assert gap >= need, ids
