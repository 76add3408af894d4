"""MXFP4 experts on the GPU: the quantiser bit for bit against tests/q4_ref.py, the MXFP4 decode GEMVs and the MXFP4
streaming MoE GEMM against fp64 references on w' = e2m1(code) 2^(byte - 127), the conversion bit for bit through a one-hot GEMM,
and the MXFP4 engine against the fp32 oracle evaluated on w' (inputs: tests/mxfp4_cases.py, whose top-2 gaps the CPU suite checks)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import moe_gemm_cases as mc
from tests import moe_gemm_util as mu
from tests import mxfp4_cases as mx
from tests import q4_ref
from tests.util import assert_close, to_np
from vita_amd import _lib, ops
from vita_amd.checkpoint import pack_mixtral, quant_mxfp4
from vita_amd.config import VitaConfig

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bf16(dev, shape, seed, std=0.02):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16).to(dev)


_dq = mu.dq_mxfp4              # w' in fp64 on the device: packed codes [.., K / 2], scale bytes [.., K / 32] -> [.., K]


def _planted(dev, rows, cols):
    """random bf16 rows with the contract's edge blocks planted (tests/test_experts_mxfp4_cpu.py checks what q4_ref makes of them)"""
    w = _bf16(dev, (rows, cols), seed=cols).float()
    w[3, 64:96] = 0                                                            # a zero block
    w[5, 11] = 8.0                                                             # an outlier: the rest of its block flushes to 0
    ties = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0], device=dev)
    for r, n in ((7, -6), (8, 0), (9, 3)):
        X = 2.0 ** n
        w[r, 32:64] = 0
        w[r, 32:41] = ties * X
        w[r, 41:50] = -ties * X                                                # every tie in both signs (amax = 6 X keeps the scale)
        w[r, 96:128] = 0
        w[r, 96:100] = torch.tensor([7.0, -7.0, 6.5, -5.5], device=dev) * X    # a saturating block
        w[r, 128:160] = 0
        w[r, 128:130] = torch.tensor([1.0, -0.0], device=dev) * X              # amax a power of two; -0
    w[11, 160:192] = 0
    w[11, 160:164] = torch.tensor([2.0 ** -126, -(2.0 ** -126), 2.0 ** -125, 3 * 2.0 ** -126], device=dev)   # the -125 clamp
    wb = w.to(torch.bfloat16)
    assert torch.equal(wb.float(), w)
    return wb


@pytest.mark.parametrize("rows,cols", [(64, 4096), (32, 14336)])
def test_quantiser_bit_exact(dev, rows, cols):
    w = _planted(dev, rows, cols)
    codes, scales = quant_mxfp4(w)
    torch.cuda.synchronize()
    rc, rs = q4_ref.quant(w.float().cpu().numpy())
    assert rs[11, 5] == 2 and rs[3, 2] == 127 and (q4_ref.unpack(rc) != 8).all()
    assert np.array_equal(to_np(scales), rs)
    assert np.array_equal(to_np(codes), rc)
    for world in (2, 4, 8):                                       # col0 / ncols slices into guarded buffers
        n = cols // world
        for r in (0, world - 1):
            cbuf = torch.full((rows + 2, n // 2 + 4), 0xEE, dtype=torch.uint8, device=dev)
            sbuf = torch.full((rows + 2, n // 32 + 4), 0xEE, dtype=torch.uint8, device=dev)
            quant_mxfp4(w, col0=r * n, ncols=n, codes=cbuf[1:-1, :n // 2], scales=sbuf[1:-1, :n // 32])
            torch.cuda.synchronize()
            assert np.array_equal(to_np(cbuf[1:-1, :n // 2]), rc[:, r * n // 2:(r + 1) * n // 2]), (world, r)
            assert np.array_equal(to_np(sbuf[1:-1, :n // 32]), rs[:, r * n // 32:(r + 1) * n // 32]), (world, r)
            for buf, k in ((cbuf, n // 2), (sbuf, n // 32)):
                assert (buf[0] == 0xEE).all() and (buf[-1] == 0xEE).all() and (buf[:, k:] == 0xEE).all(), "guards"


def _experts(dev, E, I, H, seed, I_full=None, col0=0):
    """MXFP4 experts from random bf16 weights; w2 is the column slice [col0, col0 + I) of [H, I_full] rows"""
    I_full = I_full or I
    w1, w3 = _bf16(dev, (E, I, H), seed), _bf16(dev, (E, I, H), seed + 1)
    w2 = _bf16(dev, (E, H, I_full), seed + 2)
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    out = {"w1": u8(E, I, H // 2), "s1": u8(E, I, H // 32), "w3": u8(E, I, H // 2), "s3": u8(E, I, H // 32),
           "w2": u8(E, H, I // 2), "s2": u8(E, H, I // 32)}
    for e in range(E):
        quant_mxfp4(w1[e], codes=out["w1"][e], scales=out["s1"][e])
        quant_mxfp4(w3[e], codes=out["w3"][e], scales=out["s3"][e])
        quant_mxfp4(w2[e], col0=col0, ncols=I, codes=out["w2"][e], scales=out["s2"][e])
    return out


# (H, I) by the form pick_f4 takes.  Down by I: 1792 <1,1>, 3584 <1,2> (the TP = 4 shard: 112 chunks on 128 threads), 7168 <1,4> (TP = 2:
# 224 on 256), 14336 <2,4>.  Gate|up by H: 2048 <1,1,1> at its upper edge, 4096 <2,1,2>, 8192 <4,1,4>, 14336 <7,2,4>; I = 128 is the
# smallest with I % rows_it == 0 for every form and I % 64 == 0.
DECODE_SHAPES = [(4096, 14336), (4096, 1792), (4096, 3584), (4096, 7168), (2048, 128), (8192, 128), (14336, 128)]


@pytest.mark.parametrize("H,I", DECODE_SHAPES)
@pytest.mark.parametrize("with_delta", [False, True])
def test_moe_decode_mxfp4(dev, H, I, with_delta):
    E = 8
    # w2 is a column slice of wider rows where that is what the engine has: the released rows' last I columns for the two shapes
    # this test began with, the upper half of [H, 2 I] rows for the other shard widths (the bf16 rows are drawn on the host)
    I_full = I if H != 4096 else 14336 if I in (14336, 1792) else 2 * I
    ex = _experts(dev, E, I, H, seed=I + with_delta, I_full=I_full, col0=I_full - I)
    wg = _bf16(dev, (E, H), 7)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(H, generator=g).to(dev)
    delta = (torch.randn(H, generator=g) * 0.5).to(dev) if with_delta else None
    nw = (1 + 0.1 * torch.randn(H, generator=g)).to(dev)
    _check_moe_decode(dev, ex, wg, x, delta, nw, E, I, H, f"H {H} I {I} delta {with_delta}")


def _check_moe_decode(dev, ex, wg, x, delta, nw, E, I, H, what):
    """vh_moe_decode_mxfp4 against fp64 on w': route ==, y within the int8 test's bound"""
    lib = _lib.load()
    with_delta = delta is not None
    y = torch.empty(H + 16, device=dev).fill_(7.0); xo = torch.empty(H, device=dev)
    route = torch.zeros(4, dtype=torch.int32, device=dev); hbuf = torch.empty(2 * I, device=dev)
    rc = lib.vh_moe_decode_mxfp4(_p(x), _p(delta), _p(nw), 1e-5, _p(wg), _p(ex["w1"]), _p(ex["s1"]), _p(ex["w3"]), _p(ex["s3"]),
                                 _p(ex["w2"]), _p(ex["s2"]), E, I, H, _p(xo), _p(y), _p(route), _p(hbuf), _stream())
    _lib.check(rc, "vh_moe_decode_mxfp4")
    torch.cuda.synchronize()
    assert (y[H:] == 7.0).all(), "rows past H are not written"
    y = y[:H]
    xs = x.double() + (delta.double() if with_delta else 0)
    xn = xs * torch.rsqrt((xs * xs).mean() + 1e-5) * nw.double()
    p = torch.softmax(wg.double() @ xn, 0)
    top = torch.topk(p, 2).indices.tolist()
    p3 = torch.topk(p, 3).values.tolist()
    gaps = [(p3[i] - p3[i + 1]) / p3[i] for i in range(2)]
    print(f"{what}: relative gaps of the reference's router probabilities, first / second and second / third: {gaps[0]:.3g} {gaps[1]:.3g}")
    assert min(gaps) >= 1e-6, f"{what}: the reference's own top-2 is not separated ({gaps}): `route ==` would say nothing; pick another seed"
    assert route[:2].tolist() == top
    wts = p[top] / p[top].sum()
    ref = torch.zeros(H, dtype=torch.float64, device=dev)
    for k, e in enumerate(top):
        gte = _dq(ex["w1"][e], ex["s1"][e]) @ xn
        up = _dq(ex["w3"][e], ex["s3"][e]) @ xn
        h = torch.nn.functional.silu(gte) * up
        ref += wts[k] * (_dq(ex["w2"][e], ex["s2"][e]) @ h)
    assert torch.equal(xo, x + delta) if with_delta else torch.equal(xo, x)
    err = (y.double() - ref).abs().max().item()
    print(f"{what}: max |y - ref| {err:.3e}, max |ref| {ref.abs().max().item():.3e}")
    assert torch.isfinite(y).all() and torch.isfinite(ref).all()
    assert err <= 1e-5 * ref.abs().max().item() + 1e-6, err
    return ref


@pytest.mark.parametrize("I", [1792, 3584, 7168, 14336])
def test_moe_decode_mxfp4_hand_packed(dev, I):
    """The decode GEMVs convert with the f32 form of the instruction, and the quantiser never gives them code 8 (-0) or a scale
    byte far from 127.  Hand-packed experts do: every one of the 16 codes, drawn uniformly, and the scale bytes 2, 127 and 252 in
    neighbouring blocks of every row.  The inputs keep every product a normal fp32 number so that the fp64 reference on w' is the
    bar and not overflow: |x| in [1, 2) and norm_w = 2^(127 - byte) in a w1 / w3 block's columns (the kernel multiplies x by norm_w
    before the weights), the router reads only the byte-127 columns, and the w2 columns under byte 252 meet h = 0, made by w3 rows of
    codes 0 and 8 alone: the result there is 0 whatever silu(gate) is, unless a kernel reads code 8 as anything but a zero."""
    H, E = 4096, 8
    g = torch.Generator(device="cpu").manual_seed(I)
    u8 = lambda *s, hi=256: torch.randint(0, hi, s, generator=g, dtype=torch.int32).to(torch.uint8).to(dev)
    ring1 = torch.tensor([127, 2, 252, 127, 252, 2, 127, 127], dtype=torch.uint8, device=dev)
    b1 = ring1[torch.arange(H // 32, device=dev) % 8]                               # the scale byte of a column block of w1 / w3
    ring2 = torch.tensor([110, 2, 252, 110], dtype=torch.uint8, device=dev)
    b2 = ring2[torch.arange(I // 32, device=dev) % 4]                               # and of w2
    ex = {"w1": u8(E, I, H // 2), "w3": u8(E, I, H // 2), "w2": u8(E, H, I // 2),
          "s1": b1.expand(E, I, -1).contiguous(), "s3": b1.expand(E, I, -1).contiguous(), "s2": b2.expand(E, H, -1).contiguous()}
    dead = (b2 == 252).repeat_interleave(32)                                        # rows of w3 = columns of w2 under byte 252
    nd = int(dead.sum())
    ex["w3"][:, dead] = (u8(E, nd, H // 2, hi=2) * 0x08) | (u8(E, nd, H // 2, hi=2) * 0x80)    # each nibble 0 or 8
    for k in ("w1", "w3", "w2"):
        assert ((ex[k] & 15) == 8).any() and ((ex[k] >> 4) == 8).any()
    plain = (b1 == 127).repeat_interleave(32)
    wg = _bf16(dev, (E, H), 7) * plain.to(torch.bfloat16)
    x = ((1 + torch.rand(H, generator=g)) * (1 - 2 * torch.randint(0, 2, (H,), generator=g))).to(dev)
    nw = torch.ldexp(torch.ones(H, device=dev), (127 - b1.int()).repeat_interleave(32))
    ref = _check_moe_decode(dev, ex, wg, x, None, nw, E, I, H, f"hand-packed I {I}")
    assert ref.abs().max().item() > 1.0, "the case says nothing if everything cancels"


def _planes(x):
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo, hi.double() + lo.double()


@pytest.mark.parametrize("case", ["uniform", "boundary", "tall", "m513"])
def test_gemm_ps_mxfp4_glu_and_down(dev, case):
    lib = _lib.load()
    H, I, E = 1024, 1792, 8                                       # a TP = 8 shard's expert width; every row-tile count of run_tile_sp
    rows = mc.CASES[case].rows
    M = sum(rows)
    goff = torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int32, device=dev)
    ex = _experts(dev, E, I, H, seed=len(case))
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(M, H, generator=g).to(dev)
    a_hi, a_lo, a = _planes(x)
    C1 = torch.zeros(M, I, device=dev)
    args = _lib.GemmPsArgs()
    args.A_hi, args.A_lo, args.lda = a_hi.data_ptr(), a_lo.data_ptr(), H
    args.ldw, args.w_group_stride = H, I * H
    args.group_off, args.ngroups = goff.data_ptr(), E
    args.C, args.ldc, args.M, args.N, args.K, args.ksplit = C1.data_ptr(), I, M, I, H, 1
    _lib.check(lib.vh_gemm_ps_mxfp4(C.byref(args), _p(ex["w1"]), _p(ex["s1"]), _p(ex["w3"]), _p(ex["s3"]), _stream()), "glu")
    h_hi, h_lo, hq = _planes(C1)
    nslab = torch.zeros(1, dtype=torch.int32, device=dev)
    slabs = torch.zeros(4, M, H, device=dev)
    d = _lib.GemmPsArgs()
    d.A_hi, d.A_lo, d.lda = h_hi.data_ptr(), h_lo.data_ptr(), I
    d.ldw, d.w_group_stride = I, H * I
    d.group_off, d.ngroups = goff.data_ptr(), E
    d.C, d.ldc, d.M, d.N, d.K = slabs.data_ptr(), H, M, H, I
    d.ksplit, d.c_split_stride, d.nslab_out = mc.MOE_KSPLIT, M * H, nslab.data_ptr()
    _lib.check(lib.vh_gemm_ps_mxfp4(C.byref(d), _p(ex["w2"]), _p(ex["s2"]), None, None, _stream()), "down")
    torch.cuda.synchronize()
    ns = int(nslab.item())
    assert 1 <= ns <= 4
    y = slabs[:ns].sum(0).double()
    for e in range(E):
        r0, r1 = int(goff[e]), int(goff[e + 1])
        if r0 == r1:
            continue
        ref_h = torch.nn.functional.silu(a[r0:r1] @ _dq(ex["w1"][e], ex["s1"][e]).T) * (a[r0:r1] @ _dq(ex["w3"][e], ex["s3"][e]).T)
        err = (C1[r0:r1].double() - ref_h).abs().max().item()
        assert err <= 1e-5 * ref_h.abs().max().item() + 1e-7, (case, e, "glu", err)
        ref_y = hq[r0:r1] @ _dq(ex["w2"][e], ex["s2"][e]).T
        err = (y[r0:r1] - ref_y).abs().max().item()
        assert err <= 1e-5 * ref_y.abs().max().item() + 1e-7, (case, e, "down", err)


def test_conversion_probe_bit_exact(dev):
    """C = I W'^T through the plain MXFP4 GEMM: with one-hot activation planes every output is ONE product 1 * w', so C must equal
    the dequantised weights exactly.  K = 192 is three stages; row n holds code (n + k) % 16 at element k, so over 16 rows every code
    sits at every nibble position of a stage; the scale bytes 2, 127 and 252 alternate over neighbouring blocks of every row.  N is a
    full 256-row n-tile plus a tail of 8, under both load forms (ps_nt).  The GLU form of the probe: tests/test_moe_gemm_mxfp4_gpu.py."""
    K, N, G = 192, 256 + 8, 3
    codes, scales = mu.mxfp4_probe(dev, N, K, 0, (2, 127, 252, 127, 2, 252, 252, 2))
    assert {int(v) for v in scales[0].tolist()} == {2, 127, 252}
    a_hi = torch.eye(K, device=dev).to(torch.bfloat16)
    a_lo = torch.zeros_like(a_hi)
    ref = torch.from_numpy(q4_ref.dequant(to_np(codes), to_np(scales))).to(dev)     # fp32 [N, K]
    assert torch.isfinite(ref).all() and float(ref.abs().max()) == 6 * 2.0 ** 125 and float(ref[ref != 0].abs().min()) == 2.0 ** -126
    for nt in (-1, 1):
        big = torch.full((K + 2 * G, N + 8), 123.0, device=dev)
        out = big[G:G + K, :N]
        with mu.Knobs(-1, -1, nt):
            ops.gemm_ps_mxfp4(a_hi, a_lo, codes, scales, out=out)
            torch.cuda.synchronize()
        bad = out != ref.T
        if bool(bad.any()):
            m, n = (int(v) for v in torch.nonzero(bad)[0])
            raise AssertionError(f"conversion probe [nt {nt}]: {int(bad.sum())} of {bad.numel()} differ; first at n {n}, k {m} (stage "
                                 f"{m // 64}, block {m // 32}): got {float(out[m, n]):.9g}, want {float(ref[n, m]):.9g}")
        assert (big[:G] == 123.0).all() and (big[G + K:] == 123.0).all() and (big[:, N:] == 123.0).all(), f"guard rows / columns [nt {nt}]"


def _engine(dev, cfg, packed, **kw):
    from vita_amd.engine import MixtralEngine
    eng = MixtralEngine(cfg, packed, dev, **kw)
    assert eng.experts == "mxfp4"
    return eng


@pytest.fixture(scope="module")
def tiny(dev):
    cfg, sd = mx.tiny_text_sd(mx.ENGINE_SEED)
    return cfg, sd, mx.oracle_on_wprime(sd, cfg), pack_mixtral(sd, cfg, dev, experts="mxfp4")


@pytest.mark.parametrize("chunked", [False, True])
def test_tiny_engine_mxfp4_vs_oracle_on_wprime(dev, tiny, chunked):
    cfg, sd, orc, packed = tiny
    S, n_new = mx.ENGINE_S, mx.ENGINE_NEW
    emb = mx.engine_prompt(sd, cfg)
    ref_ids, ref_lg, gap = mx.greedy(orc, emb, n_new)
    assert gap >= 2 * mx.LOGIT_TOL
    eng = _engine(dev, cfg, packed, max_ctx=S + n_new + 8, max_prefill=S, max_new=n_new + 4, logit_rows=n_new + 4)
    if chunked:
        half = S // 2
        eng.prefill(torch.from_numpy(emb[:half]).to(dev))
        eng.prefill(torch.from_numpy(emb[half:]).to(dev), pos0=half)
    else:
        eng.prefill(torch.from_numpy(emb).to(dev))
    eng.decode(n_new - 1)
    torch.cuda.synchronize()
    got = eng.generated()
    for i in range(n_new):
        assert_close(f"logits step {i}", to_np(eng.logits_all[i]), ref_lg[i], atol=mx.LOGIT_TOL)
    assert got == ref_ids
    eng.close()


@pytest.fixture(scope="module")
def seq_refs(tiny):
    cfg, sd, orc, _ = tiny
    prompts = mx.seq_prompts(sd, cfg)
    return prompts, [mx.greedy(orc, p, mx.SEQ_NEW) for p in prompts]


def test_tiny_engine_mxfp4_seq_decode_batched(dev, tiny, seq_refs):
    """six sequences through vh_mixtral_seq_decode: the streamed MoE GEMM (batch_moe_min 3) and the per-sequence GEMVs (0)."""
    cfg, _, _, packed = tiny
    prompts, refs = seq_refs
    lib = _lib.load()
    try:
        for bmm in (3, 0):
            _lib.check(lib.vh_tune(b"batch_moe_min", bmm), "vh_tune")
            eng = _engine(dev, cfg, packed, max_ctx=64 * 12, max_prefill=32, max_new=16, max_seqs=6)
            seqs = [eng.seq_alloc() for _ in prompts]
            for s, p, ref in zip(seqs, prompts, refs):
                lg = eng.seq_prefill(s, torch.from_numpy(p).to(dev), want_logits=True)
                assert_close(f"sequence {s} prefill scores", to_np(lg), ref[1][0], atol=mx.LOGIT_TOL)
            for _ in range(mx.SEQ_NEW - 1):
                eng.seq_decode(seqs)
            torch.cuda.synchronize()
            for s, ref in zip(seqs, refs):
                assert eng.seq_tokens(s)[:mx.SEQ_NEW].tolist() == ref[0], (bmm, s)
            eng.close()
    finally:
        lib.vh_tune(b"batch_moe_min", 3)


def test_tiny_engine_mxfp4_seq_prefill_batch(dev, tiny, seq_refs):
    cfg, _, _, packed = tiny
    prompts, refs = seq_refs
    pick = list(mx.SEQ_BATCH)
    eng = _engine(dev, cfg, packed, max_ctx=64 * 12, max_prefill=64, max_new=16, max_seqs=4)
    seqs = [eng.seq_alloc() for _ in pick]
    lg = eng.seq_prefill_batch(seqs, [torch.from_numpy(prompts[i]).to(dev) for i in pick], want_logits=True)
    for _ in range(mx.SEQ_NEW - 1):
        eng.seq_decode(seqs)
    torch.cuda.synchronize()
    for j, i in enumerate(pick):
        assert_close(f"segment {j} prefill scores", to_np(lg[j]), refs[i][1][0], atol=mx.LOGIT_TOL)
        assert eng.seq_tokens(seqs[j])[:mx.SEQ_NEW].tolist() == refs[i][0], i
    eng.close()


@pytest.fixture(scope="module")
def tiny_ckpt_dir(tmp_path_factory):
    from tests import tiny_ckpt
    d = str(tmp_path_factory.mktemp("vita_tiny_ckpt_mxfp4"))
    sd = tiny_ckpt.write(d, seed=mx.CKPT_SEED)
    return d, {k: np.asarray(v, np.float32) for k, v in sd.items()}


def _oracle_ids(sd, ids, n):
    cfg = VitaConfig.tiny()
    return mx.oracle_on_wprime(sd, cfg).greedy(sd["model.embed_tokens.weight"][ids], n)[0]


def test_load_pretrained_mxfp4_generate(tiny_ckpt_dir, dev):
    from vita_amd.model import load_pretrained_model
    d, sd = tiny_ckpt_dir
    with pytest.raises(NotImplementedError, match="experts_mxfp4"):
        load_pretrained_model(d, None, "vita-tiny", "mixtral-8x7b", load_4bit=True)
    with pytest.raises(ValueError):
        load_pretrained_model(d, None, "vita-tiny", "mixtral-8x7b", load_8bit=True, experts_mxfp4=True)
    _, model, _, _ = load_pretrained_model(d, None, "vita-tiny", "mixtral-8x7b", experts_mxfp4=True)
    try:
        assert model.engine.experts == "mxfp4"
        ids = mx.CKPT_LOAD_IDS
        t = torch.tensor([ids], device=dev)
        emb = model.model.embed_tokens(t[0])
        out = model.generate(t, inputs_embeds=emb[None], max_new_tokens=mx.CKPT_LOAD_NEW)
        got = out[0, len(ids):].tolist()
        exp = _oracle_ids(sd, ids, mx.CKPT_LOAD_NEW)
        n = mx.CKPT_LOAD_NEW
        assert 1 <= len(got) <= n and got == exp[:len(got)] and (len(got) == n or got[-1] == 2), (got, exp)
    finally:
        model.engine.close()
        del model
        torch.cuda.empty_cache()


def test_llm_experts_mxfp4_generate(tiny_ckpt_dir, dev):
    from vita_amd.serving import LLM, SamplingParams
    d, sd = tiny_ckpt_dir
    for q in ("fp8", "awq"):
        with pytest.raises(ValueError):
            LLM(model=d, quantization=q)
    llm = LLM(model=d, dtype="float16", tensor_parallel_size=1, quantization="experts_mxfp4", max_new_tokens=16)
    try:
        assert llm.model.engine.experts == "mxfp4"
        ids, n = mx.CKPT_LLM_IDS, mx.CKPT_LLM_NEW
        out = llm.generate({"prompt_token_ids": ids}, sampling_params=SamplingParams(max_tokens=n))
        got = out[0].outputs[0].token_ids
        exp = _oracle_ids(sd, ids, n)
        assert 1 <= len(got) <= n and got == exp[:len(got)] and (len(got) == n or got[-1] == 2), (got, exp)
    finally:
        llm.model.engine.close()
        del llm
        torch.cuda.empty_cache()
