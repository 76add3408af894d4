"""vh_attn_rows (k_attn_rows_part + k_attn_rows_merge): split-KV paged attention for single query rows whose q is already rotated —
the attention of the decode rows of a mixed pass (vh_mixtral_seq_step) — as an operator, against fp64 at the 5e-5 that
tests/test_ops_gpu.py holds vh_attn_decode* to."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_ops_gpu import _dev, _steer
from tests.util import assert_close, to_np

pytestmark = pytest.mark.gpu

D = 128
# a single key; a tile boundary from both sides; a partial last tile behind two full ones; 66 tiles (a second 64-lane round of the
# merge, one key in its last tile) next to 1-tile neighbours, so that most blocks of the (66, nkv, 6) grid leave at once.  Six rows:
# more than the VH_BMAX = 4 lanes of the batched decode attention
KLENS = [1, 63, 64, 65, 129, 4161]
LONG = 5                       # the row that carries the score pattern
# score patterns of the long row (those of test_attn_decode_long_context, moved to where THIS row's tiles are): (key of the high score,
# its value, the value of every key from tile 64 on)
PATTERNS = {"random": None,
            "late-max-100": (65 * 64, 100.0, None),            # the only key of tile 65: the global max lives in the second merge round
            "late-splits-underflow": (5, 60.0, -60.0)}         # max in tile 0; tiles 64, 65 weigh exp(-120) = 0 exactly and must drop out


def _setup(dev, nq, nkv, pattern):
    rng = np.random.default_rng(nq * 100 + nkv + 7 * len(pattern))
    G, scale = nq // nkv, D ** -0.5
    need = [(k + 63) // 64 for k in KLENS]
    n_pages = sum(need) + 3
    perm = rng.permutation(n_pages)
    pages = [perm[sum(need[:b]):sum(need[:b + 1])] for b in range(len(KLENS))]
    assert not np.array_equal(pages[LONG], np.arange(pages[LONG][0], pages[LONG][0] + need[LONG]))      # shuffled, interleaved
    q = rng.standard_normal((len(KLENS), nq * D), dtype=np.float32)
    # every pool row that no row's klen covers is NaN: the stale tail of a last page, the pages of nobody
    kp = np.full((nkv, n_pages * 64, D), np.nan, np.float32)
    vp = np.full((nkv, n_pages * 64, D), np.nan, np.float32)
    refs = []
    for b, klen in enumerate(KLENS):
        pat = PATTERNS[pattern] if b == LONG else None
        kl = (rng.standard_normal((nkv, klen, D), dtype=np.float32) * (0.1 if pat else 1.0)).astype(np.float32)
        vl = rng.standard_normal((nkv, klen, D), dtype=np.float32)
        qb = q[b].reshape(nq, D).astype(np.float64)
        if pat:
            hi_key, hi, lo = pat
            for h in range(nkv):
                Qg = qb[h * G:(h + 1) * G]
                if lo is not None:
                    kl[h, 64 * 64:] = (_steer(Qg, lo / scale)[None, :] + 0.1 * rng.standard_normal((klen - 64 * 64, D))).astype(np.float32)
                kl[h, hi_key] = _steer(Qg, hi / scale).astype(np.float32)
        for p, pg in enumerate(pages[b]):
            n = min(64, klen - p * 64)
            kp[:, pg * 64:pg * 64 + n] = kl[:, p * 64:p * 64 + n]
            vp[:, pg * 64:pg * 64 + n] = vl[:, p * 64:p * 64 + n]
        ref = np.empty((nq, D))
        for hq in range(nq):
            sc = kl[hq // G].astype(np.float64) @ qb[hq] * scale
            if pat and pat[2] is not None:
                assert sc.max() - sc[64 * 64:].max() > 110               # the late tiles' weights are exactly 0 in fp32
            elif pat:
                assert np.argmax(sc) == pat[0] and sc[pat[0]] - np.delete(sc, pat[0]).max() > 80
            w = np.exp(sc - sc.max())
            ref[hq] = (w / w.sum()) @ vl[hq // G].astype(np.float64)
        refs.append(ref.reshape(-1))
    return dict(q=_dev(q, dev), kc=_dev(kp, dev), vc=_dev(vp, dev), tables=[_dev(pg, dev, torch.int32) for pg in pages],
                ref=np.stack(refs), scale=scale)


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("nq,nkv", [(4, 2), (8, 2)], ids=["G2", "G4"])
def test_attn_rows_vs_fp64(dev, nq, nkv, pattern):
    """six rows of key counts 1 ... 4161 over ONE shuffled pool in one call, G = 2 and G = 4 query heads per KV head; every pool row
    that no row covers is NaN, so an unmasked key or a stale row read as data shows as a non-finite output.  Both output forms — fp32
    rows, and the bf16 hi / lo planes whose sum is held to the same 5e-5 — and a second call on the same scratch gives the same bits."""
    from vita_amd import ops
    t = _setup(dev, nq, nkv, pattern)
    scratch = ops.attn_rows_scratch(len(KLENS), nq, max(KLENS), dev)
    args = (t["q"], t["kc"], t["vc"], KLENS, t["tables"], nq, nkv, t["scale"])
    out = ops.attn_rows(*args, scratch=scratch)
    hi, lo = ops.attn_rows(*args, scratch=scratch, planes=True)
    again = ops.attn_rows(*args, scratch=scratch)
    torch.cuda.synchronize()
    for b, klen in enumerate(KLENS):
        assert_close(f"attn_rows fp32 row {b} ({klen} keys, {pattern})", to_np(out[b]), t["ref"][b], atol=5e-5)
        assert_close(f"attn_rows hi + lo row {b} ({klen} keys, {pattern})", to_np(hi[b]).astype(np.float64) + to_np(lo[b]), t["ref"][b],
                     atol=5e-5)
    assert torch.equal(out, again), "a second call on the same scratch differs"


def test_attn_rows_in_several_launches(dev):
    """a scratch that holds the long row only alone: the rows run in several launch pairs, same results as in one."""
    from vita_amd import _lib, ops
    nq, nkv = 8, 2
    t = _setup(dev, nq, nkv, "random")
    args = (t["q"], t["kc"], t["vc"], KLENS, t["tables"], nq, nkv, t["scale"])
    one = ops.attn_rows(*args)
    small = torch.empty(_lib.load().vh_attn_rows_scratch_bytes(1, nq, max(KLENS)) + 256, dtype=torch.uint8, device=dev)
    assert small.numel() < ops.attn_rows_scratch(len(KLENS), nq, max(KLENS), dev).numel() // 4
    several = ops.attn_rows(*args, scratch=small)
    torch.cuda.synchronize()
    assert torch.equal(one, several)
    assert_close("attn_rows in several launches", to_np(several), t["ref"], atol=5e-5)


def test_attn_rows_refuses_bad_arguments(dev):
    """null pointers, a key count of 0 or past the pool, a misaligned q, heads the kernel has no form for and a scratch too small
    for one row are refused before anything is launched: the output stays as it was."""
    from vita_amd import _lib, ops
    nq, nkv = 8, 2
    t = _setup(dev, nq, nkv, "random")
    lib = _lib.load()
    n, max_ctx = len(KLENS), t["kc"].shape[1]
    scratch = ops.attn_rows_scratch(n, nq, max(KLENS), dev)
    out = torch.full((n, nq * D), float("nan"), dtype=torch.float32, device=dev)
    qpad = torch.zeros(n * nq * D + 4, dtype=torch.float32, device=dev)
    base = dict(n=n, q=t["q"].data_ptr(), ldq=nq * D, kc=t["kc"].data_ptr(), vc=t["vc"].data_ptr(), klens=(C.c_int * n)(*KLENS),
                tables=(C.c_void_p * n)(*[x.data_ptr() for x in t["tables"]]), nq=nq, nkv=nkv, max_ctx=max_ctx, scratch=scratch.data_ptr(),
                scratch_bytes=scratch.numel(), out=out.data_ptr(), hi=None, lo=None)

    def raw(**over):
        a = dict(base)
        a.update(over)
        return lib.vh_attn_rows(a["n"], a["q"], a["ldq"], a["kc"], a["vc"], a["klens"], a["tables"], a["nq"], a["nkv"], a["max_ctx"],
                                t["scale"], a["scratch"], a["scratch_bytes"], a["out"], a["hi"], a["lo"], nq * D, None)

    def klens(i, v):
        k = list(KLENS)
        k[i] = v
        return (C.c_int * n)(*k)

    for name in ("q", "kc", "vc", "klens", "tables", "scratch", "out"):
        assert raw(**{name: None}) == -2 and b"null pointer" in lib.vh_last_error(), name                 # VH_E_ARG
    tb = [x.data_ptr() for x in t["tables"]]
    tb[2] = None
    assert raw(tables=(C.c_void_p * n)(*tb)) == -2 and b"null page table" in lib.vh_last_error()
    assert raw(out=None, hi=out.data_ptr()) == -2                                                          # one plane without the other
    for i, v in ((0, 0), (3, -5), (5, max_ctx + 1), (1, 1 << 30)):
        assert raw(klens=klens(i, v)) == -1 and b"outside [1," in lib.vh_last_error(), (i, v)             # VH_E_SHAPE
    assert raw(q=qpad.data_ptr() + 4) == -2 and b"misaligned" in lib.vh_last_error()
    assert raw(ldq=nq * D + 1) == -1 and raw(ldq=nq * D - 4) == -1
    assert raw(n=0) == -1 and raw(nq=10, nkv=2) == -1 and raw(nq=7, nkv=2) == -1
    assert raw(scratch_bytes=4096) == -1 and b"scratch" in lib.vh_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote an output"
    assert raw() == 0                                                   # and the same arguments, all valid, are accepted
    torch.cuda.synchronize()
    assert_close("attn_rows after the refusals", to_np(out), t["ref"], atol=5e-5)
