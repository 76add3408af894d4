"""The MXFP4 streaming MoE GEMM (vh_gemm_ps_mxfp4 / k_gemm_sp_mxfp4 in vh_gemm_sp.hip) at the released widths — H = 4096,
I = 14336, E = 8 and the TP shards of I — and across its schedule, against float64 references of the same operation on
w' = e2m1(code) 2^(byte - 127).  Under MXFP4 this one kernel serves the prefill MoE, seq_prefill_batch, every TP branch and the batched
decode iterations, so what tests/test_moe_gemm_i8_gpu.py pins for the int8 stagers is pinned here for the fp4 ones (4 bytes of codes
plus one scale byte per piece, two scale blocks per 64-wide stage, two stager waves by stage parity), with that module's machinery
(tests/moe_gemm_util.py) and case list (tests/moe_gemm_cases.py; which schedule paths and stage parities the lists reach:
tests/test_moe_gemm_sched_cpu.py).

Operands: the bf16 module's seeded W recipe, with one row holding an all-zero block and one row holding an outlier planted in expert
0 of w1, w3 and w2, quantised on the device one expert at a time (quant_mxfp4); activations N(0, 1) fp32 split into planes.
References: float64 matmuls on w' (dequantised in float64 from the codes and bytes: moe_gemm_util.dq_mxfp4), one expert at a time, on
the fp32 activations; every output element is compared.  A TP shard is a slice of the codes and of the scales, never requantised,
so the reference is always the full tensor's w'.

Tolerance: the int8 module's bounds unchanged.  The conversion to bf16 is exact and the MFMA stream is the bf16 kernel's, so the
bf16 module's bounds hold with rms(w') in the place of rms(w): atol(K, rms(w')) for down and plain, the GEMM bound through
d(SiLU(g) u) plus 2^-16 |h| for gate|up (glu_tol).  rms(w') is always taken from the dequantised reference weights of the case.  The
plain conversion probe (tests/test_experts_mxfp4_gpu.py) is bit-exact.  Worst |diff| / tol per section as measured: DESIGN 5.8,
"kernel-level parity"."""
import pytest
import torch

from tests import moe_gemm_cases as mc
from tests import moe_gemm_util as mu
from tests.moe_gemm_util import SENT, Knobs, atol, close, guard, randn

pytestmark = pytest.mark.gpu

H, I, E = mc.H, mc.I, mc.E

# (row with the zero block [64, 96), row with the outlier at element 11) planted in expert 0.  w1 and w3 get DIFFERENT rows, so that
# a dead block of one meets live weights of the partner.  The outlier is 2.0 = 100 sigma: its block's scale is 2^-1 and every other
# element of the block (|w| < 6 sigma = 0.12 < 0.125 = X / 4) flushes to 0.  It stays small enough for the bound, which is derived
# from rms(w'): the activation planes carry x to 2^-18 |x|, so the outlier's product adds at most 2.0 * 2^-18 |x| < 4e-5 at |x| < 5,
# a third of atol(4096) and half of the smallest bound it meets, atol(1792) of the TP = 8 shard that holds it (rank 0 of down).
PLANT = {"w1": (3, 5), "w3": (6, 9), "w2": (3, 5)}
OUTLIER = 2.0


def _knobs():
    """default knobs (device-side default placement, plain weight loads) and the other tile placement with non-temporal loads: both
    NTW instantiations of the kernel.  Tile placement is code shared with the bf16 and int8 forms and pinned there under every
    combination, so the int8 module's four sets are two here."""
    return [Knobs(-1, -1, -1), Knobs(-1, 0, 1)]


def _sumsq(t):
    return float(t.double().pow(2).sum())


def _rms(t):
    return (_sumsq(t) / t.numel()) ** 0.5


# ---- data ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def Q(dev):
    """c1, c3 [E, I, H / 2], c2 [E, H, I / 2] codes with s1, s3 [E, I, H / 32], s2 [E, H, I / 32] scale bytes (~0.75 GB), and the
    float64 w' they stand for as p1, p3, p2 (~11.3 GB: every reference of the module reads them), with rms13 = the larger rms of
    p1 and p3 and rms2 = rms(p2).  The bf16 weights are freed once quantised."""
    from vita_amd.checkpoint import quant_mxfp4
    w = mu.make_weights(dev, plain=False)
    q = {}
    ss = {}
    for k in ("w1", "w3", "w2"):
        zr, outl = PLANT[k]
        w[k][0, zr, 64:96] = 0                                         # a zero block: byte 127, codes 0
        w[k][0, outl, 11] = OUTLIER                                    # an outlier: the rest of its block flushes to 0
        rows, cols = w[k].shape[1:]
        c = q["c" + k[1]] = torch.empty((E, rows, cols // 2), dtype=torch.uint8, device=dev)
        s = q["s" + k[1]] = torch.empty((E, rows, cols // 32), dtype=torch.uint8, device=dev)
        p = q["p" + k[1]] = torch.empty((E, rows, cols), dtype=torch.float64, device=dev)
        ss[k] = 0.0
        for e in range(E):
            quant_mxfp4(w[k][e], codes=c[e], scales=s[e])
            p[e] = mu.dq_mxfp4(c[e], s[e])
            ss[k] += _sumsq(p[e])
        assert int(s[0, zr, 2]) == 127 and not bool(c[0, zr, 32:48].any()) and not bool(p[0, zr, 64:96].any())
        assert int(s[0, outl, 0]) == 126 and int(c[0, outl, 5]) == 0x60 and int(c[0, outl, :16].sum()) == 0x60   # 4 * 2^-1, alone
        assert float(p[0, outl, 11]) == OUTLIER
        del w[k]
        ss[k] = (ss[k] / p.numel()) ** 0.5
    q["rms13"], q["rms2"] = max(ss["w1"], ss["w3"]), ss["w2"]
    print(f"rms(w'): w1 {ss['w1']:.6g}, w3 {ss['w3']:.6g}, w2 {ss['w2']:.6g}")
    torch.cuda.empty_cache()
    yield q
    q.clear()
    torch.cuda.empty_cache()


_CACHE = {}


def _build(dev, Q, rows, seed):
    return mu.build_case(dev, rows, seed, lambda e: (Q["p1"][e], Q["p3"][e]), gemm_tol=atol(H, Q["rms13"]))


@pytest.fixture(scope="module")
def cases(dev, Q):
    """lazily built per-case operands and float64 references on w' (the bf16 module's seeds: the same activations)."""
    def get(name):
        if name not in _CACHE:
            _CACHE[name] = _build(dev, Q, mc.CASES[name].rows, 1000 + list(mc.CASES).index(name))
        return _CACHE[name]
    yield get
    _CACHE.clear()
    torch.cuda.empty_cache()


# ---- runners ---------------------------------------------------------------------------------------------------------------------
def _run_gateup(c, what, c1, s1, c3, s3, n0=0, n1=I):
    """gate|up as the engine calls it: gathered through a_rowidx, written as guarded bf16 planes.  c1 / c3 [E, N, H / 2] and s1 / s3
    [E, N, H / 32] are the operands of columns [n0, n1) (dense: a rank's own tensors)."""
    from vita_amd import ops
    N = n1 - n0
    mu.run_gateup(c, what, lambda hi, lo: ops.gemm_ps_mxfp4(c.x_hi, c.x_lo, c1, s1, w_up=c3, s_up=s3, a_rowidx=c.tok, group_off=c.goff,
                                                            ngroups=E, w_group_stride=N * H, m=c.M, out_split=True,
                                                            out_planes=(hi, lo)), n0, n1)


def _run_down(c, Q, what, ksplit, c2=None, s2=None, k0=0, k1=I, n0=0, n1=H, tol=None):
    """down as the engine calls it: scattered through c_rowidx into guarded slabs.  c2 [E, H, K / 2] / s2 [E, H, K / 32]: a rank's K
    range [k0, k1) of the codes and scales, dense or a strided view of the full tensors (ldw = I > K: the row and group strides are
    taken from the tensor); output columns [n0, n1) are passed as moe_down_gemm passes an overlap half: the codes from row n0, the
    scales from row n0.  The reference is ALWAYS the full tensor's w'."""
    from vita_amd import ops
    K = k1 - k0
    c2, s2 = (Q["c2"], Q["s2"]) if c2 is None else (c2, s2)
    assert c2.stride(0) == 16 * s2.stride(0) and c2.shape[-1] == K // 2
    a_hi, a_lo = (c.h_hi, c.h_lo) if K == I else (c.h_hi[:, k0:k1], c.h_lo[:, k0:k1])
    ref = mu.down_ref(c, k0, k1, lambda e: Q["p2"][e, :, k0:k1])
    return mu.run_down(c, what, ksplit, K, ref,
                       lambda out, nslab: ops.gemm_ps_mxfp4(a_hi, a_lo, c2[:, n0:n1], s2[:, n0:n1], group_off=c.goff, ngroups=E,
                                                            w_group_stride=2 * c2.stride(0), c_rowidx=c.slot, m=c.M, out=out,
                                                            ksplit=ksplit, nslab_out=nslab), n0, n1,
                       tol=atol(K, Q["rms2"]) if tol is None else tol)


# ---- a. released widths, whole schedule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.CASES))
def test_gateup_released_width(dev, Q, cases, name):
    c = cases(name)
    for k in _knobs():
        with k:
            _run_gateup(c, f"{name} [{k}]", Q["c1"], Q["s1"], Q["c3"], Q["s3"])


@pytest.mark.parametrize("name", list(mc.CASES))
def test_down_released_width(dev, Q, cases, name):
    """the engine's device-chosen split (ksplit = -4, count through nslab_out) and fixed splits of 1, 2, 3 (tiles with k0 != 0 at
    slab boundaries of nk = 224) under both knob sets."""
    c = cases(name)
    for k in _knobs():
        with k:
            for ksplit in (mc.MOE_KSPLIT, 1, 2, 3):
                _run_down(c, Q, f"{name} [{k}]", ksplit)


# ---- b. TP shards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tp", [2, 4, 8])
@pytest.mark.parametrize("name", mc.TP_CASES)
def test_tp_shards(dev, Q, cases, name, tp):
    """every rank's shard of I: gate|up on the rank's rows [k0, k1) of w1 / w3 (N = I / TP) under both knob sets; down on the rank's
    K range, once on a dense copy of the code and scale slices (what a rank stores; default knobs) and once on the strided view of
    the full tensors (ldw = I > K: code row stride I / 2 != K / 2, scale row stride I / 32 != K / 32; the other knob set), each as the
    whole N and as the two overlap column halves (N = 2048).  The bound of a shard's down uses the rms of ITS columns of w'."""
    c = cases(name)
    it = I // tp
    dense, strided = _knobs()
    for r in range(tp):
        k0, k1 = r * it, (r + 1) * it
        c1, c3 = Q["c1"][:, k0:k1].contiguous(), Q["c3"][:, k0:k1].contiguous()
        s1, s3 = Q["s1"][:, k0:k1].contiguous(), Q["s3"][:, k0:k1].contiguous()
        v2, t2 = Q["c2"][:, :, k0 // 2:k1 // 2], Q["s2"][:, :, k0 // 32:k1 // 32]
        d2, e2 = v2.contiguous(), t2.contiguous()
        tol = atol(it, _rms(Q["p2"][:, :, k0:k1]))
        for k in (dense, strided):
            with k:
                _run_gateup(c, f"{name} tp{tp} rank {r} [{k}]", c1, s1, c3, s3, k0, k1)
        for k, form, w2, s2 in ((dense, "dense", d2, e2), (strided, "ldw = I", v2, t2)):
            with k:
                _run_down(c, Q, f"{name} tp{tp} rank {r} {form} [{k}]", mc.MOE_KSPLIT, w2, s2, k0, k1, tol=tol)
                for hh in range(2):
                    _run_down(c, Q, f"{name} tp{tp} rank {r} {form} half {hh} [{k}]", mc.MOE_KSPLIT, w2, s2, k0, k1,
                              hh * (H // 2), (hh + 1) * (H // 2), tol=tol)
        del c1, c3, s1, s3, d2, e2
        c.y_ref.pop((k0, k1), None)


# ---- c. batched-decode shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cnt", mc.DECODE_CNTS, ids=lambda c: "-".join(map(str, c)))
def test_decode_iteration_shapes(dev, Q, cnt):
    """an iteration of a few concurrent sequences (n >= batch_moe_min runs this kernel under MXFP4): a handful of rows per expert at
    the released widths, gate|up into planes and down with the device-chosen split; the checks of the released-width tests."""
    c = _build(dev, Q, tuple(cnt), 2000 + mc.DECODE_CNTS.index(tuple(cnt)))
    for k in _knobs():
        with k:
            _run_gateup(c, f"decode {cnt} [{k}]", Q["c1"], Q["s1"], Q["c3"], Q["s3"])
            _run_down(c, Q, f"decode {cnt} [{k}]", mc.MOE_KSPLIT)


# ---- d, e, f: small problems with their own weights --------------------------------------------------------------------------------
def _quant(w):
    """bf16 [G, N, K] -> codes uint8 [G, N, K / 2], scale bytes uint8 [G, N, K / 32], w' float64"""
    from vita_amd.checkpoint import quant_mxfp4
    c = torch.empty(w.shape[:2] + (w.shape[2] // 2,), dtype=torch.uint8, device=w.device)
    s = torch.empty(w.shape[:2] + (w.shape[2] // 32,), dtype=torch.uint8, device=w.device)
    for e in range(w.shape[0]):
        quant_mxfp4(w[e], codes=c[e], scales=s[e])
    torch.cuda.synchronize()
    return c, s, mu.dq_mxfp4(c, s)


class CaseOps:
    pass


def _guarded(rows, N, dtype, dev, lead=()):
    """SENT-filled buffer with 16 guard rows and guard columns up to a row stride that is a multiple of 4 (so that the 4-wide stores
    run on the full chunks and the element-wise ones on the N tail), and its [rows, N] view."""
    b = torch.full(tuple(lead) + (rows + mu.GUARD_ROWS, N + 64 - N % 4), SENT, dtype=dtype, device=dev)
    return b, b[..., :rows, :N]


def _guards(what, b, rows, N, live=None):
    guard(f"{what} guard rows", b[..., rows:, :] if live is None else b[..., ~live, :])
    guard(f"{what} guard columns", b[..., N:])


@pytest.mark.parametrize("K", mc.SMALL_K)
def test_short_and_odd_k(dev, K):
    """1 .. 5 K stages: the fp4 stagers' prologue (stage 0, half each), the clamped re-load past the tile's end (kc = nk - 1) and the
    two stagers' stage parity, under both load forms (ps_nt); K = 64 and 192 give rows with an odd number of stages, where the second
    scale block of the last stage ends the row.  M of one row, one row tile + 1 and 13 row tiles; N with a tail that is no multiple
    of 16 or 4, below and above the tile width (the row clamp n > N - 1 of the code load and of the scale-byte load, GLU's interleaved
    rows and plain); grouped (gathered and scattered) and ungrouped (the launcher's rt_cap selection); GLU into planes, plain into
    fp32, and for plain the largest fixed split: one stage per slab, every tile but the first with k0 != 0.  One quantised
    [3, 390, K] gate and up tensor per K; a case takes its first G groups and N rows (row stride K, group strides of the whole
    tensor).  The smallest shapes at which the prologue, the clamp and the parity can fail."""
    from vita_amd import ops
    gen = torch.Generator(device=dev).manual_seed(3000 + K)
    cg = torch.Generator().manual_seed(3000 + K)
    GM, NM = 3, max(mc.SMALL_N)
    q1, s1, wp1 = _quant(randn(gen, (GM, NM, K), dev, mu.W_STD).to(torch.bfloat16))
    q3, s3, wp3 = _quant(randn(gen, (GM, NM, K), dev, mu.W_STD).to(torch.bfloat16))
    tol_plain, tol_glu = atol(K, _rms(wp1)), atol(K, max(_rms(wp1), _rms(wp3)))
    acts = {}

    def operands(M, grouped):
        if (M, grouped) not in acts:
            o = CaseOps()
            o.rows = mc.SMALL_ROWS[M] if grouped else (M,)
            o.goff = [0]
            for r in o.rows:
                o.goff.append(o.goff[-1] + r)
            o.R = M + mu.GUARD_ROWS
            o.kw, o.live = {}, None
            if grouped:
                tok = (torch.randperm(M, generator=cg) // 2).to(dev)
                slots = torch.randperm(o.R, generator=cg).to(dev)
                o.slot = slots[mu.GUARD_ROWS:]
                o.live = torch.ones(o.R, dtype=torch.bool, device=dev)
                o.live[slots[:mu.GUARD_ROWS]] = False
                x = randn(gen, ((M + 1) // 2, K), dev)
                o.xr = x[tok].double()
                o.kw = dict(a_rowidx=tok.to(torch.int32), c_rowidx=o.slot.to(torch.int32), m=M, ngroups=len(o.rows),
                            w_group_stride=NM * K, group_off=torch.tensor(o.goff, dtype=torch.int32, device=dev))
            else:
                x = randn(gen, (M, K), dev)
                o.xr = x.double()
                o.slot = torch.arange(M, device=dev)
            o.xh, o.xl = ops.split_planes(x)
            o.ok = o.live if grouped else slice(0, M)
            acts[(M, grouped)] = o
        return acts[(M, grouped)]

    for (M, N, Kc, glu, grouped, ksplit) in mc.small_cases():
        if Kc != K:
            continue
        o = operands(M, grouped)
        G = len(o.rows)

        def ref_of(w):
            y = torch.zeros((o.R, N), dtype=torch.float64, device=dev)
            for e in range(G):
                y[o.slot[o.goff[e]:o.goff[e + 1]].long()] = o.xr[o.goff[e]:o.goff[e + 1]] @ w[e, :N].T
            return y

        wq, ws = (q1[:G, :N], s1[:G, :N]) if grouped else (q1[0, :N], s1[0, :N])
        if glu:
            wq3, ws3 = (q3[:G, :N], s3[:G, :N]) if grouped else (q3[0, :N], s3[0, :N])
            g, u = ref_of(wp1), ref_of(wp3)
            h_ref, h_tol = (mu.silu(g) * u)[o.ok], mu.glu_tol(g, u, tol_glu)[o.ok]
        else:
            ref = ref_of(wp1)[o.ok]
        for nt in (-1, 1):
            what = (f"K={K} M={M} N={N} {'glu' if glu else 'plain'} {'grouped' if grouped else 'ungrouped'} ksplit {ksplit} "
                    f"[nt {nt}]")
            with Knobs(-1, -1, nt):
                if glu:
                    hb, hi = _guarded(M, N, torch.bfloat16, dev)
                    lb, lo = _guarded(M, N, torch.bfloat16, dev)
                    if grouped:                                    # scattered planes: the views are the whole [R, N]
                        hi, lo = hb[:, :N], lb[:, :N]
                    ops.gemm_ps_mxfp4(o.xh, o.xl, wq, ws, w_up=wq3, s_up=ws3, out_split=True, out_planes=(hi, lo), **o.kw)
                    torch.cuda.synchronize()
                    close(what, (hb[:, :N].double() + lb[:, :N].double())[o.ok], h_ref, h_tol)
                    bad = lb[:, :N][o.ok].double().abs() > 2.0 ** -7 * hb[:, :N][o.ok].double().abs()
                    assert not bool(bad.any()), f"{what}: lo is not a residual of hi at {int(bad.sum())} elements"
                    for b in (hb, lb):
                        _guards(what, b, M, N, o.live)
                else:
                    b, out = _guarded(M, N, torch.float32, dev, lead=(ksplit,))
                    if grouped:
                        out = b[:, :, :N]
                    ops.gemm_ps_mxfp4(o.xh, o.xl, wq, ws, out=out if ksplit > 1 else out[0], ksplit=ksplit, **o.kw)
                    torch.cuda.synchronize()
                    close(what, b[:, :, :N].double().sum(0)[o.ok], ref, tol_plain)
                    _guards(what, b, M, N, o.live)


# fp32 arithmetic of the plain epilogue, relative to the magnitudes it acts on: four roundings of 2^-24 each (bias, act, scale, resid;
# there is no weight-scale multiply under MXFP4, where the int8 module counts five) plus the int8 module's 3 x 2^-24 for an erff /
# expf of a few ulp: that module's 2^-21 = 8 x 2^-24 less one rounding
EPI_REL = 7 * 2.0 ** -24


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("act", [None, "gelu", "relu", "silu"])
def test_plain_epilogue_terms(dev, act, grouped):
    """the non-GLU, ksplit = 1 epilogue the ABI accepts under MXFP4: act(a w'^T + bias) scale + resid through c_rowidx, written to
    fp32 C and to the planes in one call.  Bound: atol(K) on this case's rms(w'), as for every plain output, NOT widened by the
    activation's slope or the column scale; plus the fp32 arithmetic of the epilogue itself (EPI_REL of the magnitudes it acts on);
    the planes add their split's 2^-17 |value|.  The hi plane must equal C rounded to bf16."""
    from vita_amd import ops
    M, N, K = 200, 390, 192
    gen = torch.Generator(device=dev).manual_seed(4000 + 2 * list((None, "gelu", "relu", "silu")).index(act) + grouped)
    rows = mc.SMALL_ROWS[M] if grouped else (M,)
    G = len(rows)
    goff = [0]
    for r in rows:
        goff.append(goff[-1] + r)
    q, s, wp = _quant(randn(gen, (G, N, K), dev, 0.05).to(torch.bfloat16))
    x = randn(gen, (M, K), dev)
    xh, xl = ops.split_planes(x)
    bias, scale = randn(gen, (N,), dev, 0.5), 1 + randn(gen, (N,), dev, 0.25)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(5)).to(dev)
    resid_b, resid = _guarded(M, N, torch.float32, dev)
    resid.copy_(randn(gen, (M, N), dev))
    z = torch.empty((M, N), dtype=torch.float64, device=dev)
    for e in range(G):
        z[goff[e]:goff[e + 1]] = x[goff[e]:goff[e + 1]].double() @ wp[e].T
    z += bias.double()
    a = {None: z, "gelu": torch.nn.functional.gelu(z), "relu": torch.relu(z), "silu": mu.silu(z)}[act]
    ref = torch.empty_like(z)
    ref[perm] = a * scale.double() + resid.double()[perm]              # row m goes to output row perm[m], whose resid it adds
    tolr = torch.empty_like(z)
    tolr[perm] = atol(K, _rms(wp)) + EPI_REL * ((z.abs() + a.abs()) * scale.double().abs() + resid.double()[perm].abs())
    kw = dict(group_off=torch.tensor(goff, dtype=torch.int32, device=dev), ngroups=G, w_group_stride=N * K) if grouped else {}
    wq, ws = (q, s) if grouped else (q[0], s[0])
    cb, cv = _guarded(M, N, torch.float32, dev)
    hb, hi = _guarded(M, N, torch.bfloat16, dev)
    lb, lo = _guarded(M, N, torch.bfloat16, dev)
    ops.gemm_ps_mxfp4(xh, xl, wq, ws, bias=bias, act=act, scale=scale, resid=resid, c_rowidx=perm.to(torch.int32), out=cv,
                      out_split=True, out_planes=(hi, lo), **kw)
    torch.cuda.synchronize()
    what = f"epilogue act {act} {'grouped' if grouped else 'ungrouped'}"
    close(what + " C", cv, ref, tolr)
    close(what + " planes", hi.double() + lo.double(), ref, tolr + 2.0 ** -17 * ref.abs())
    assert torch.equal(hi, cv.to(torch.bfloat16)), f"{what}: the hi plane is not C rounded to bf16"
    for b in (cb, hb, lb, resid_b):
        _guards(what, b, M, N)


def test_conversion_probe_glu(dev):
    """the plain probe of tests/test_experts_mxfp4_gpu.py (one-hot activations: every output is ONE weight; code (n + k) % 16 at
    element k of row n, so every code sits at every nibble position of a stage; three stages) through the GLU form, whose LDS image
    interleaves gate and up rows: the codes on gate, a copy shifted by 5 codes and 3 ring places on up, N = 128 + 8: a full n-tile
    plus a tail, both load forms.  g = w1'[n, m] and u = w3'[n, m] are single weights; SiLU is not bit-reproducible, so h is held to
    the gate|up bound (atol(K) on the larger rms through d(SiLU(g) u), plus 2^-16 |h|).  The scale bytes are 125 .. 127 in
    neighbouring blocks, so |g|, |u| <= 6 where SiLU is well conditioned; a wrong nibble is off by >= 0.125 and a wrong block by a
    factor of 2 or 4, orders of magnitude outside the bound."""
    from vita_amd import ops
    N, K = 128 + 8, 192
    ring = (126, 127, 125, 127, 126, 125, 127, 125)                                    # neighbours always differ, wrap included
    c1, s1 = mu.mxfp4_probe(dev, N, K, 0, ring)
    c3, s3 = mu.mxfp4_probe(dev, N, K, 5, ring[3:] + ring[:3])
    x = torch.eye(K, device=dev, dtype=torch.float32)
    xh, xl = ops.split_planes(x)
    assert torch.equal(xh.float(), x) and not bool(xl.float().any())
    g, u = mu.dq_mxfp4(c1, s1).T, mu.dq_mxfp4(c3, s3).T
    assert float(g.abs().max()) == 6.0 and float(u.abs().max()) == 6.0
    tol = mu.glu_tol(g, u, atol(K, max(_rms(g), _rms(u))))
    for nt in (-1, 1):
        with Knobs(-1, -1, nt):
            b, out = _guarded(K, N, torch.float32, dev)
            ops.gemm_ps_mxfp4(xh, xl, c1, s1, w_up=c3, s_up=s3, out=out)
            torch.cuda.synchronize()
        close(f"conversion probe glu [nt {nt}]", out, mu.silu(g) * u, tol)
        _guards(f"conversion probe glu [nt {nt}]", b, K, N)


# ---- g. refusals (the return codes alone, without a GPU: tests/test_experts_mxfp4_cpu.py) ------------------------------------------
def test_refusals_write_nothing(dev):
    """the int8 module's list and MXFP4's own (ldw % 64, w_group_stride % 64, ldw < K): VH_E_SHAPE before anything is launched or
    written — C, the planes and nslab_out keep their sentinels.  M == 0 is accepted and writes nothing either."""
    from vita_amd import _lib, ops
    M, N, K = 32, 256, 256
    q = torch.full((9, N, K // 2), 0x22, dtype=torch.uint8, device=dev)
    s = torch.full((9, N, K // 32), 127, dtype=torch.uint8, device=dev)
    qw = torch.full((N, K // 2 + 16), 0x22, dtype=torch.uint8, device=dev)             # rows of K + 32 weights: ldw % 64 == 32
    sw = torch.full((N, K // 32 + 1), 127, dtype=torch.uint8, device=dev)
    x = torch.ones((M, K), dtype=torch.bfloat16, device=dev)
    goff9 = torch.tensor([0] * 9 + [M], dtype=torch.int32, device=dev)
    goff2 = torch.tensor([0, M // 2, M], dtype=torch.int32, device=dev)
    nslab = torch.full((1,), 77, dtype=torch.int32, device=dev)
    vec = torch.ones(N, device=dev)
    bufs = {"c": torch.full((8, M, N), SENT, device=dev), "hi": torch.full((M, N), SENT, dtype=torch.bfloat16, device=dev),
            "lo": torch.full((M, N), SENT, dtype=torch.bfloat16, device=dev)}
    planes = dict(out_split=True, out_planes=(bufs["hi"], bufs["lo"]))

    def untouched(what):
        torch.cuda.synchronize()
        for nm, b in bufs.items():
            guard(f"{what}: {nm}", b)
        assert int(nslab.item()) == 77, what

    for what, a, kw in [
            ("K % 64 != 0", (x[:, :96], x[:, :96], q[0, :, :48], s[0, :, :3]), dict(out=bufs["c"][0])),
            ("ksplit > K / 64", (x, x, q[0], s[0]), dict(out=bufs["c"][:5], ksplit=5)),
            ("K split with GLU", (x, x, q[0], s[0]), dict(w_up=q[1], s_up=s[1], out=bufs["c"][:2], ksplit=2)),
            ("device K split with GLU", (x, x, q[0], s[0]), dict(w_up=q[1], s_up=s[1], out=bufs["c"][:2], ksplit=-2, nslab_out=nslab)),
            ("K split with bias", (x, x, q[0], s[0]), dict(bias=vec, out=bufs["c"][:2], ksplit=2)),
            ("K split with act", (x, x, q[0], s[0]), dict(act="silu", out=bufs["c"][:2], ksplit=2)),
            ("K split with scale", (x, x, q[0], s[0]), dict(scale=vec, out=bufs["c"][:2], ksplit=2)),
            ("K split with resid", (x, x, q[0], s[0]), dict(resid=torch.ones((M, N), device=dev), out=bufs["c"][:2], ksplit=2)),
            ("K split with planes", (x, x, q[0], s[0]), dict(out=bufs["c"][:2], ksplit=2, **planes)),
            ("ngroups > 8", (x, x, q, s), dict(out=bufs["c"][0], group_off=goff9, ngroups=9, w_group_stride=N * K)),
            ("ldw % 64 != 0", (x, x, qw[:, :K // 2], sw[:, :K // 32]), dict(out=bufs["c"][0])),
            ("ldw % 64 != 0 into planes", (x, x, qw[:, :K // 2], sw[:, :K // 32]), planes),
            ("w_group_stride % 64 != 0", (x, x, q[:2], s[:2]), dict(out=bufs["c"][0], group_off=goff2, ngroups=2, w_group_stride=N * K + 32)),
            ("ldw < K", (x, x, q[0].as_strided((N, K // 2), (K // 2 - 32, 1)), s[0].as_strided((N, K // 32), (K // 32 - 2, 1))),
             dict(out=bufs["c"][:4], ksplit=-4, nslab_out=nslab))]:
        with pytest.raises(_lib.VitaHipError):
            ops.gemm_ps_mxfp4(*a, **kw)
        untouched(f"refused call ({what})")
    for what, kw in [("C", dict(out=bufs["c"][0])), ("planes", planes), ("device K split", dict(out=bufs["c"][:4], ksplit=-4, nslab_out=nslab)),
                     ("grouped", dict(out=bufs["c"][0], group_off=torch.zeros(3, dtype=torch.int32, device=dev), ngroups=2,
                                      w_group_stride=N * K))]:
        ops.gemm_ps_mxfp4(x, x, q[:2] if what == "grouped" else q[0], s[:2] if what == "grouped" else s[0], m=0, **kw)
        untouched(f"M == 0 ({what})")
