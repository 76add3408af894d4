"""int8 experts without a GPU: the quantisation formula on edge rows, its error bound, and the argument checks
of vh_mixtral_create_i8 that run before any device work."""
import ctypes as C

import numpy as np
import pytest

from tests import q8_ref


def test_formula_edge_rows():
    w = np.zeros((6, 8), np.float32)
    w[1] = [1.0, -1.0, 0.5, -0.5, 0.25, 0.0, 127.0, -127.0]            # +-absmax -> +-127
    w[2] = [127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.0]                # s = 1: ties to even, negative ties
    w[3] = [-254.0, 1.0, 3.0, -3.0, 5.0, 0.0, 0.0, 0.0]                 # s = 2: w / s on .5 (both signs)
    w[4] = [1e-30, -1e-30, 0, 0, 0, 0, 0, 0]                           # tiny but nonzero
    w[5] = [-3.0, 1.0, 0, 0, 0, 0, 0, 0]                               # negative absmax
    q, s = q8_ref.quant_rows(w)
    assert s[0] == 0 and (q[0] == 0).all(), "a zero row has scale 0 and q 0"
    assert s[1] == np.float32(127.0) / np.float32(127)
    assert q[1, 6] == 127 and q[1, 7] == -127
    assert list(q[2]) == [127, 0, 2, 2, 0, -2, -2, 3]
    assert s[3] == np.float32(2.0)
    assert list(q[3][:5]) == [-127, 0, 2, -2, 2]
    assert q[4, 0] == 127 and q[4, 1] == -127
    assert q[5, 0] == -127 and abs(int(q[5, 1])) == 42
    assert q.dtype == np.int8 and s.dtype == np.float32


def test_error_bound():
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((64, 4096)) * 0.02).astype(np.float32)
    w[5, 7] = 0.9                                                      # an outlier sets its row's scale
    q, s = q8_ref.quant_rows(w)
    wp = q8_ref.dequant(q, s)
    assert (np.abs(q.astype(np.int32)) <= 127).all()
    assert (np.abs(w - wp) <= s[:, None] / 2 * (1 + 1e-6)).all()
    assert np.abs(q).max(axis=1).min() == 127                          # every row reaches its absmax


def test_w2_shard_scales_are_full_row():
    """a TP rank's w2 shard is the column slice of q under the FULL row's scale, so every degree computes the same w'.
    Re-quantising the slice on its own would give other scales (and another model): this is what the engine must not do."""
    rng = np.random.default_rng(4)
    w2 = (rng.standard_normal((16, 256)) * 0.02).astype(np.float32)
    w2[3, 200] = 0.5                                          # row 3's absmax lies in the last quarter of its columns
    q, s = q8_ref.quant_rows(w2)
    wp = q8_ref.dequant(q, s)
    for world in (2, 4, 8):
        n = 256 // world
        shards = [q8_ref.dequant(q[:, r * n:(r + 1) * n], s) for r in range(world)]
        assert np.array_equal(np.concatenate(shards, 1), wp)
        own = [q8_ref.quant_rows(w2[:, r * n:(r + 1) * n]) for r in range(world)]
        assert any((ss != s).any() for _, ss in own), "a shard's own scales differ from the full row's"
        assert not np.array_equal(np.concatenate([q8_ref.dequant(qq, ss) for qq, ss in own], 1), wp)
        assert own[0][1][3] < s[3]                             # the first shard does not hold row 3's absmax


def _cfg():
    from vita_amd._lib import MixtralCfg
    c = MixtralCfg()
    c.hidden, c.n_layers, c.n_q_heads, c.n_kv_heads, c.head_dim = 128, 2, 4, 2, 128
    c.inter, c.n_experts, c.top_k, c.vocab, c.rms_eps = 256, 4, 2, 512, 1e-5
    c.max_ctx, c.max_prefill, c.max_new = 128, 64, 16
    return c


def _lib():
    from vita_amd import _lib
    try:
        return _lib.load()
    except _lib.VitaHipError as e:
        pytest.skip(str(e))


def test_create_i8_argument_checks():
    from vita_amd._lib import MixtralExpertsI8, MixtralLayer
    lib = _lib()
    c = _cfg()
    fake = 0x1000                                            # never dereferenced: every case fails before device work
    layers = (MixtralLayer * 2)()
    for L in layers:
        for f, _ in MixtralLayer._fields_:
            if f not in ("w1", "w3", "w2"):
                setattr(L, f, fake)
    ex = (MixtralExpertsI8 * 2)()
    for q in ex:
        for f, _ in MixtralExpertsI8._fields_:
            setattr(q, f, fake)
    args = (fake, fake, fake, fake, fake, fake, 1 << 30)

    def create(ex_arg):
        return lib.vh_mixtral_create_i8(C.byref(c), layers, ex_arg, *args)

    assert not create(None)
    assert b"null" in lib.vh_last_error()
    layers[1].w1 = fake                                      # a bf16 expert pointer next to int8 experts
    assert not create(ex)
    assert b"layers[1]" in lib.vh_last_error()
    layers[1].w1 = None
    ex[0].s2 = None                                          # a null scale
    assert not create(ex)
    assert b"experts[0]" in lib.vh_last_error()
    ex[0].s2 = fake
    ex[1].w3 = None                                          # a null int8 weight
    assert not create(ex)
    assert b"experts[1]" in lib.vh_last_error()


def test_quant_rows_i8_null_pointers():
    lib = _lib()
    assert lib.vh_quant_rows_i8(None, 1, 64, 64, 0, 64, None, 64, None, None) == -2


def test_gemm_ps_i8_refusals():
    """vh_gemm_ps_i8 refuses these before any device work (VH_E_SHAPE, the reason in vh_last_error).  M = 0 throughout: every check
    runs before the launcher's no-rows return, so a check that stopped refusing would show as rc 0 here without a launch on the
    fake pointers.  That a refused call with rows writes nothing is checked on the GPU:
    tests/test_moe_gemm_i8_gpu.py::test_refusals_write_nothing."""
    from vita_amd._lib import GemmPsArgs
    lib = _lib()
    fake = 0x1000

    def refused(why, glu=False, **kw):
        a = GemmPsArgs()
        a.A_hi, a.A_lo, a.lda, a.ldw, a.C, a.ldc = fake, fake, 256, 256, fake, 256
        a.M, a.N, a.K, a.ksplit, a.c_split_stride = 0, 256, 256, 1, 32 * 256
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.vh_gemm_ps_i8(C.byref(a), fake, fake, fake if glu else None, fake if glu else None, 256, None)
        assert rc == -1, (kw, rc)
        msg = lib.vh_last_error()
        assert msg.startswith(b"vh_gemm_ps_i8: ") and why in msg, (kw, msg)

    refused(b"multiple of 64", K=96)                                  # lda, ldw % 8 == 0: K is what is refused
    refused(b"multiple of 64", K=32)
    refused(b"above K / 64", ksplit=5)                                # more slabs than K stages (K / 64 = 4)
    refused(b"below -8", ksplit=-9, nslab_out=fake)
    refused(b"needs nslab_out", ksplit=-4)
    for ks in (2, -2):                                                # a K split with GLU, an epilogue term or planes
        split = b"a K split takes a plain GEMM"
        refused(split, glu=True, ksplit=ks, nslab_out=fake)
        for term in ("bias", "scale", "resid"):
            refused(split, ksplit=ks, nslab_out=fake, **{term: fake})
        refused(split, ksplit=ks, nslab_out=fake, act=3)
        refused(split, ksplit=ks, nslab_out=fake, C_hi=fake, C_lo=fake, ldc_split=256)
        refused(split, ksplit=ks, nslab_out=fake, C=None, C_hi=fake, C_lo=fake, ldc_split=256)
    refused(b"more than 8 groups", group_off=fake, ngroups=9)         # the tile list holds 8 groups
    refused(b"2^32", ldw=1 << 20, N=4096)                             # 32-bit per-lane byte offsets inside a group
    a = GemmPsArgs()
    a.A_hi, a.A_lo, a.lda, a.ldw, a.C, a.ldc, a.N, a.K, a.W = fake, fake, 256, 256, fake, 256, 256, 256, fake
    assert lib.vh_gemm_ps_i8(C.byref(a), fake, fake, None, None, 256, None) == -2       # args->W next to the int8 weights


def test_unknown_quantization_raises():
    from vita_amd.serving import LLM
    with pytest.raises(ValueError):
        LLM("/nonexistent", quantization="awq")
