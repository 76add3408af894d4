"""int8 experts on the GPU: the quantiser bit for bit against tests/q8_ref.py, the int8 decode GEMVs and the int8
streaming MoE GEMM against fp64 references on w' = q s, and the int8 engine against the fp32 oracle evaluated on w'."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mixtral as om
from tests import moe_gemm_cases as mc
from tests import q8_ref
from tests.util import assert_close, to_np
from vita_amd import _lib
from vita_amd.checkpoint import pack_mixtral, quant_rows_i8, synth_state_dict
from vita_amd.config import VitaConfig

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bf16(dev, shape, seed, std=0.02):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16).to(dev)


def _dq(q, s):
    return q.double() * s.double().unsqueeze(-1)


@pytest.mark.parametrize("rows,cols", [(64, 4096), (32, 14336)])
def test_quantiser_bit_exact(dev, rows, cols):
    w = _bf16(dev, (rows, cols), seed=cols)
    w[3] = 0                                                       # a zero row
    w[5, 11] = 0.75                                                # an outlier row
    q, s = quant_rows_i8(w)
    torch.cuda.synchronize()
    rq, rs = q8_ref.quant_rows(w.float().cpu().numpy())
    assert np.array_equal(to_np(s), rs) and np.array_equal(to_np(q), rq)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_quantiser_w2_slices_full_row_scales(dev, world):
    H, I = 256, 14336
    w2 = _bf16(dev, (H, I), seed=world)
    rq, rs = q8_ref.quant_rows(w2.float().cpu().numpy())
    n = I // world
    for r in range(world):
        q, s = quant_rows_i8(w2, col0=r * n, ncols=n)
        torch.cuda.synchronize()
        assert np.array_equal(to_np(s), rs), "the shard's scales are the full rows'"
        assert np.array_equal(to_np(q), rq[:, r * n:(r + 1) * n])


def _experts(dev, E, I, H, seed, I_full=None):
    I_full = I_full or I
    w1, w3 = _bf16(dev, (E, I, H), seed), _bf16(dev, (E, I, H), seed + 1)
    w2 = _bf16(dev, (E, H, I_full), seed + 2)
    out = {}
    for nm, w in (("1", w1), ("3", w3)):
        q = torch.empty(E, I, H, dtype=torch.int8, device=dev); s = torch.empty(E, I, dtype=torch.float32, device=dev)
        for e in range(E):
            quant_rows_i8(w[e], q=q[e], s=s[e])
        out["w" + nm], out["s" + nm] = q, s
    q = torch.empty(E, H, I, dtype=torch.int8, device=dev); s = torch.empty(E, H, dtype=torch.float32, device=dev)
    for e in range(E):
        quant_rows_i8(w2[e], col0=0, ncols=I, q=q[e], s=s[e])
    out["w2"], out["s2"] = q, s
    return out


@pytest.mark.parametrize("H,I", [(4096, 14336), (4096, 1792)])
@pytest.mark.parametrize("with_delta", [False, True])
def test_moe_decode_i8(dev, H, I, with_delta):
    lib = _lib.load()
    E = 8
    ex = _experts(dev, E, I, H, seed=I + with_delta, I_full=14336)
    wg = _bf16(dev, (E, H), 7)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(H, generator=g).to(dev)
    delta = (torch.randn(H, generator=g) * 0.5).to(dev) if with_delta else None
    nw = (1 + 0.1 * torch.randn(H, generator=g)).to(dev)
    y = torch.empty(H, device=dev); xo = torch.empty(H, device=dev)
    route = torch.zeros(4, dtype=torch.int32, device=dev); hbuf = torch.empty(2 * I, device=dev)
    rc = lib.vh_moe_decode_i8(_p(x), _p(delta), _p(nw), 1e-5, _p(wg), _p(ex["w1"]), _p(ex["s1"]), _p(ex["w3"]), _p(ex["s3"]),
                              _p(ex["w2"]), _p(ex["s2"]), E, I, H, _p(xo), _p(y), _p(route), _p(hbuf), _stream())
    _lib.check(rc, "vh_moe_decode_i8")
    torch.cuda.synchronize()
    # fp64 reference on w'
    xs = x.double() + (delta.double() if with_delta else 0)
    xn = xs * torch.rsqrt((xs * xs).mean() + 1e-5) * nw.double()
    p = torch.softmax(wg.double() @ xn, 0)
    top = torch.topk(p, 2).indices.tolist()
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
    assert err <= 1e-5 * ref.abs().max().item() + 1e-6, err


def _planes(x):
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo, hi.double() + lo.double()


@pytest.mark.parametrize("case", ["uniform", "boundary", "tall", "m513"])
def test_gemm_ps_i8_glu_and_down(dev, case):
    lib = _lib.load()
    H, I, E = 1024, 1792, 8                                       # a TP = 8 shard's expert width; every row-tile count of run_tile_sp
    rows = mc.CASES[case].rows
    M = sum(rows)
    goff = torch.tensor(np.concatenate([[0], np.cumsum(rows)]), dtype=torch.int32, device=dev)
    ex = _experts(dev, E, I, H, seed=len(case))
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(M, H, generator=g).to(dev)
    a_hi, a_lo, a = _planes(x)
    # gate|up (GLU) into fp32 C
    C1 = torch.zeros(M, I, device=dev)
    args = _lib.GemmPsArgs()
    args.A_hi, args.A_lo, args.lda = a_hi.data_ptr(), a_lo.data_ptr(), H
    args.ldw, args.w_group_stride = H, I * H
    args.group_off, args.ngroups = goff.data_ptr(), E
    args.C, args.ldc, args.M, args.N, args.K, args.ksplit = C1.data_ptr(), I, M, I, H, 1
    _lib.check(lib.vh_gemm_ps_i8(C.byref(args), _p(ex["w1"]), _p(ex["s1"]), _p(ex["w3"]), _p(ex["s3"]), I, _stream()), "glu")
    # down from h's planes, K split chosen on the device (slabs summed here)
    h_hi, h_lo, hq = _planes(C1)
    nslab = torch.zeros(1, dtype=torch.int32, device=dev)
    slabs = torch.zeros(4, M, H, device=dev)
    d = _lib.GemmPsArgs()
    d.A_hi, d.A_lo, d.lda = h_hi.data_ptr(), h_lo.data_ptr(), I
    d.ldw, d.w_group_stride = I, H * I
    d.group_off, d.ngroups = goff.data_ptr(), E
    d.C, d.ldc, d.M, d.N, d.K = slabs.data_ptr(), H, M, H, I
    d.ksplit, d.c_split_stride, d.nslab_out = mc.MOE_KSPLIT, M * H, nslab.data_ptr()
    _lib.check(lib.vh_gemm_ps_i8(C.byref(d), _p(ex["w2"]), _p(ex["s2"]), None, None, H, _stream()), "down")
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


def _tiny_engine_vs_oracle(dev, S, n_new, chunked=False, seed=0):
    from vita_amd.engine import MixtralEngine
    cfg = VitaConfig.tiny()
    sd = synth_state_dict(cfg, seed=seed, parts=("text",))
    rng = np.random.default_rng(seed + 100)
    emb = sd["model.embed_tokens.weight"][rng.integers(3, cfg.text.vocab_size, size=S)]
    ref_ids, ref_lg = om.MixtralOracle(q8_ref.dequant_state_dict(sd), cfg.text).greedy(emb, n_new)
    eng = MixtralEngine(cfg, pack_mixtral(sd, cfg, dev, experts="int8"), dev, max_ctx=S + n_new + 8, max_prefill=S,
                        max_new=n_new + 4, logit_rows=n_new + 4)
    assert eng.experts == "int8"
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
        assert_close(f"logits step {i}", to_np(eng.logits_all[i]), ref_lg[i], atol=LOGIT_TOL)
    assert got == ref_ids
    eng.close()


@pytest.mark.parametrize("chunked", [False, True])
def test_tiny_engine_int8_vs_oracle_on_wprime(dev, chunked):
    _tiny_engine_vs_oracle(dev, S=37, n_new=17, chunked=chunked)


def test_tiny_engine_int8_seq_decode_batched(dev):
    """six sequences through vh_mixtral_seq_decode: the streamed MoE GEMM (batch_moe_min 3) and the per-sequence GEMVs (0)."""
    from vita_amd.engine import MixtralEngine
    cfg = VitaConfig.tiny()
    sd = synth_state_dict(cfg, seed=3, parts=("text",))
    orc = om.MixtralOracle(q8_ref.dequant_state_dict(sd), cfg.text)
    rng = np.random.default_rng(7)
    prompts = [sd["model.embed_tokens.weight"][rng.integers(3, cfg.text.vocab_size, size=5 + 3 * i)] for i in range(6)]
    refs = []
    for p in prompts:
        orc.reset()
        refs.append(orc.greedy(p, 6)[0])
    lib = _lib.load()
    packed = pack_mixtral(sd, cfg, dev, experts="int8")
    try:
        for bmm in (3, 0):
            _lib.check(lib.vh_tune(b"batch_moe_min", bmm), "vh_tune")
            eng = MixtralEngine(cfg, packed, dev, max_ctx=64 * 12, max_prefill=32, max_new=16, max_seqs=6)
            seqs = [eng.seq_alloc() for _ in prompts]
            for s, p in zip(seqs, prompts):
                eng.seq_prefill(s, torch.from_numpy(p).to(dev))
            for _ in range(5):
                eng.seq_decode(seqs)
            torch.cuda.synchronize()
            for s, ref in zip(seqs, refs):
                assert eng.seq_tokens(s)[:6].tolist() == ref, (bmm, s)
            eng.close()
    finally:
        lib.vh_tune(b"batch_moe_min", 3)


@pytest.fixture(scope="module")
def tiny_ckpt_dir(tmp_path_factory):
    from tests import tiny_ckpt
    d = str(tmp_path_factory.mktemp("vita_tiny_ckpt_i8"))
    sd = tiny_ckpt.write(d, seed=21)
    return d, {k: np.asarray(v, np.float32) for k, v in sd.items()}


def _oracle_ids(sd, ids, n):
    cfg = VitaConfig.tiny()
    return om.MixtralOracle(q8_ref.dequant_state_dict(sd), cfg.text).greedy(sd["model.embed_tokens.weight"][ids], n)[0]


def test_load_pretrained_8bit_generate(tiny_ckpt_dir, dev):
    from vita_amd.model import load_pretrained_model
    d, sd = tiny_ckpt_dir
    with pytest.raises(NotImplementedError):
        load_pretrained_model(d, None, "vita-tiny", "mixtral-8x7b", load_4bit=True)
    _, model, _, _ = load_pretrained_model(d, None, "vita-tiny", "mixtral-8x7b", load_8bit=True)
    try:
        assert model.engine.experts == "int8"
        ids = [1, 5, 6, 7, 8, 9, 10, 11, 12]
        t = torch.tensor([ids], device=dev)
        emb = model.model.embed_tokens(t[0])                  # text only: the prompt's embeddings [S, H] (no image / audio placeholders)
        out = model.generate(t, inputs_embeds=emb[None], max_new_tokens=6)
        got = out[0, len(ids):].tolist()
        exp = _oracle_ids(sd, ids, 6)
        assert 1 <= len(got) <= 6 and got == exp[:len(got)] and (len(got) == 6 or got[-1] == 2), (got, exp)
    finally:
        model.engine.close()
        del model
        torch.cuda.empty_cache()


def test_llm_experts_int8_generate(tiny_ckpt_dir, dev):
    from vita_amd.serving import LLM, SamplingParams
    d, sd = tiny_ckpt_dir
    with pytest.raises(ValueError):
        LLM(model=d, quantization="fp8")
    llm = LLM(model=d, dtype="float16", tensor_parallel_size=1, quantization="experts_int8", max_new_tokens=16)
    try:
        assert llm.model.engine.experts == "int8"
        ids = [1, 5, 6, 7, 8]
        out = llm.generate({"prompt_token_ids": ids}, sampling_params=SamplingParams(max_tokens=4))
        got = out[0].outputs[0].token_ids
        exp = _oracle_ids(sd, ids, 4)
        assert 1 <= len(got) <= 4 and got == exp[:len(got)] and (len(got) == 4 or got[-1] == 2), (got, exp)
    finally:
        llm.model.engine.close()
        del llm
        torch.cuda.empty_cache()
