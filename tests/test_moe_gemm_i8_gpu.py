"""The int8 streaming MoE GEMM (vh_gemm_ps_i8 / k_gemm_sp_i8 in vh_gemm_sp.hip) at the released widths — H = 4096,
I = 14336, E = 8 and the TP shards of I — and across its schedule, against float64 references of the same operation on w' = q s.
Under int8 this one kernel serves the prefill MoE, every TP branch and the batched decode iterations, so what tests/test_moe_gemm_gpu.py
pins for the bf16 form is pinned here for the int8 stagers (8-byte pieces, shift-based int8 -> bf16 conversion, two stager waves by
stage parity) and the scaled epilogue, with that module's machinery (tests/moe_gemm_util.py) and case list (tests/moe_gemm_cases.py;
which schedule paths and stage parities the lists reach: tests/test_moe_gemm_sched_cpu.py).

Operands: the bf16 module's seeded W recipe, with one all-zero row and one outlier row planted in expert 0 of w1, w3 and w2, quantised
on the device one expert at a time (quant_rows_i8); activations N(0, 1) fp32 split into planes.  References: float64 matmuls on
w' = q s, one expert at a time, on the fp32 activations; every output element is compared.

Tolerance: the int8 kernel issues the bf16 kernel's MFMAs on weights that are exact in bf16 and adds one fp32 multiply by the scale
(2^-24 relative); w' has the rms of w.  So the bf16 module's bounds hold unchanged: atol(K) for down and plain, the GEMM bound through
d(SiLU(g) u) plus 2^-16 |h| for gate|up.  The small-K sections use atol(K) with their own rms(w'); the conversion probe is exact for
plain.  Worst |diff| / tol per section as measured: DESIGN 5.5, "kernel-level parity"."""
import pytest
import torch

from tests import moe_gemm_cases as mc
from tests import moe_gemm_util as mu
from tests.moe_gemm_util import SENT, Knobs, atol, close, guard, randn

pytestmark = pytest.mark.gpu

H, I, E = mc.H, mc.I, mc.E


# (zero row, outlier row) planted in expert 0.  w1 and w3 get DIFFERENT rows, so that a zero scale on one of s / s_up meets a live
# partner: column 3 has g = 0 under a live u, column 6 a live g under u = 0.
PLANT = {"w1": (3, 5), "w3": (6, 9), "w2": (3, 5)}


def _knobs():
    """both tile placements x non-temporal weight loads off / on.  ps_cfg is left alone: the int8 launcher ignores it (always the
    12-wave specialised kernel), so the bf16 module's 24 knob sets are 4 here."""
    return [Knobs(-1, x, n) for x in (0, 3) for n in (-1, 1)]


def _dq(q, s):
    return q.double() * s.double().unsqueeze(-1)


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


# ---- data ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def Q(dev):
    """q1, q3 [E, I, H], q2 [E, H, I] int8 with s1, s3 [E, I], s2 [E, H] fp32 (~1.4 GB), and the bf16 w2 they came from (the TP shards
    are quantised from it with the full rows' scales).  The bf16 w1 / w3 are freed once quantised."""
    from vita_amd.checkpoint import quant_rows_i8
    w = mu.make_weights(dev, plain=False)
    q = {}
    for k in ("w1", "w3", "w2"):
        zr, outl = PLANT[k]
        w[k][0, zr] = 0                                                # a zero row: scale 0, q 0
        w[k][0, outl, 11] = 0.75                                       # an outlier row: its scale is the outlier's
        rows, cols = w[k].shape[1:]
        q["q" + k[1]] = torch.empty((E, rows, cols), dtype=torch.int8, device=dev)
        q["s" + k[1]] = torch.empty((E, rows), dtype=torch.float32, device=dev)
        for e in range(E):
            quant_rows_i8(w[k][e], q=q["q" + k[1]][e], s=q["s" + k[1]][e])
        torch.cuda.synchronize()
        assert float(q["s" + k[1]][0, zr]) == 0 and not bool(q["q" + k[1]][0, zr].any())
        assert int(q["q" + k[1]][0, outl, 11]) == 127 and int(q["q" + k[1]][0, outl].abs().sum()) < 127 + 8 * cols
        if k != "w2":
            del w[k]
    q["w2"] = w["w2"]
    torch.cuda.empty_cache()
    yield q
    q.clear()
    w.clear()
    torch.cuda.empty_cache()


_CACHE = {}


def _case(dev, Q, key, rows, seed):
    if key not in _CACHE:
        _CACHE[key] = mu.build_case(dev, rows, seed, lambda e: (_dq(Q["q1"][e], Q["s1"][e]), _dq(Q["q3"][e], Q["s3"][e])))
    return _CACHE[key]


@pytest.fixture(scope="module")
def cases(dev, Q):
    """lazily built per-case operands and float64 references on w' (the bf16 module's seeds: the same activations)."""
    def get(name):
        return _case(dev, Q, name, mc.CASES[name].rows, 1000 + list(mc.CASES).index(name))
    yield get
    _CACHE.clear()
    torch.cuda.empty_cache()


# ---- runners ---------------------------------------------------------------------------------------------------------------------
def _run_gateup(c, what, q1, s1, q3, s3, n0=0, n1=I):
    """gate|up as the engine calls it: gathered through a_rowidx, written as guarded bf16 planes.  q1 / q3 [E, N, H] and s1 / s3
    [E, N] are the operands of columns [n0, n1) (dense: a rank's own tensors)."""
    from vita_amd import ops
    N = n1 - n0
    mu.run_gateup(c, what, lambda hi, lo: ops.gemm_ps_i8(c.x_hi, c.x_lo, q1, s1, w_up=q3, s_up=s3, s_group_stride=N, a_rowidx=c.tok,
                                                         group_off=c.goff, ngroups=E, w_group_stride=N * H, m=c.M, out_split=True,
                                                         out_planes=(hi, lo)), n0, n1)


def _run_down(c, Q, what, ksplit, q2=None, s2=None, k0=0, k1=I, n0=0, n1=H):
    """down as the engine calls it: scattered through c_rowidx into guarded slabs.  q2 [E, H, K] / s2 [E, H]: a rank's K range
    [k0, k1) of q under the full rows' scales; output columns [n0, n1) are passed as moe_down_gemm passes an overlap half:
    W + n0 ldw, s + n0, s_group_stride = H.  The reference is ALWAYS the full-row-scaled w' of the module's q2 / s2."""
    from vita_amd import ops
    K = k1 - k0
    q2, s2 = (Q["q2"], Q["s2"]) if q2 is None else (q2, s2)
    a_hi, a_lo = (c.h_hi, c.h_lo) if K == I else (c.h_hi[:, k0:k1], c.h_lo[:, k0:k1])
    ref = mu.down_ref(c, k0, k1, lambda e: _dq(Q["q2"][e, :, k0:k1], Q["s2"][e]))
    return mu.run_down(c, what, ksplit, K, ref,
                       lambda out, nslab: ops.gemm_ps_i8(a_hi, a_lo, q2[:, n0:n1], s2[:, n0:n1], s_group_stride=H, group_off=c.goff,
                                                         ngroups=E, w_group_stride=H * K, c_rowidx=c.slot, m=c.M, out=out, ksplit=ksplit,
                                                         nslab_out=nslab), n0, n1)


# ---- a. released widths, whole schedule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.CASES))
def test_gateup_released_width(dev, Q, cases, name):
    c = cases(name)
    for k in _knobs():
        with k:
            _run_gateup(c, f"{name} [{k}]", Q["q1"], Q["s1"], Q["q3"], Q["s3"])


@pytest.mark.parametrize("name", list(mc.CASES))
def test_down_released_width(dev, Q, cases, name):
    """the engine's device-chosen split (ksplit = -4, count through nslab_out) and fixed splits of 1, 2, 3 under every knob set."""
    c = cases(name)
    for k in _knobs():
        with k:
            for ksplit in (mc.MOE_KSPLIT, 1, 2, 3):
                _run_down(c, Q, f"{name} [{k}]", ksplit)


# ---- b. TP shards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tp", [2, 4, 8])
@pytest.mark.parametrize("name", mc.TP_CASES)
def test_tp_shards(dev, Q, cases, name, tp):
    """every rank's shard of I: gate|up on N = I / TP with the rank's slice of the scales; down on K = I / TP with q from
    quant_rows_i8(w2[e], col0, ncols), whose scales are the FULL rows' (a shard that rescaled its own slice computes another model
    and fails here against the full-row w'); and down's two overlap column halves (N = 2048) per rank; both placements."""
    from vita_amd.checkpoint import quant_rows_i8
    c = cases(name)
    it = I // tp
    for r in range(tp):
        k0, k1 = r * it, (r + 1) * it
        q1, q3 = Q["q1"][:, k0:k1].contiguous(), Q["q3"][:, k0:k1].contiguous()
        s1, s3 = Q["s1"][:, k0:k1].contiguous(), Q["s3"][:, k0:k1].contiguous()
        q2 = torch.empty((E, H, it), dtype=torch.int8, device=dev)
        s2 = torch.empty((E, H), dtype=torch.float32, device=dev)
        for e in range(E):
            quant_rows_i8(Q["w2"][e], col0=k0, ncols=it, q=q2[e], s=s2[e])
        for x in (0, 3):
            with Knobs(-1, x):
                _run_gateup(c, f"{name} tp{tp} rank {r} [xcd {x}]", q1, s1, q3, s3, k0, k1)
                _run_down(c, Q, f"{name} tp{tp} rank {r} [xcd {x}]", mc.MOE_KSPLIT, q2, s2, k0, k1)
                for hh in range(2):
                    _run_down(c, Q, f"{name} tp{tp} rank {r} half {hh} [xcd {x}]", mc.MOE_KSPLIT, q2, s2, k0, k1,
                              hh * (H // 2), (hh + 1) * (H // 2))
        del q1, q3, s1, s3, q2, s2
        c.y_ref.pop((k0, k1), None)


# ---- c. batched-decode shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cnt", mc.DECODE_CNTS, ids=lambda c: "-".join(map(str, c)))
def test_decode_iteration_shapes(dev, Q, cnt):
    """an iteration of a few concurrent sequences (n >= batch_moe_min runs this kernel under int8): a handful of rows per expert at
    the released widths, gate|up into planes and down with the device-chosen split; the checks of the released-width tests."""
    c = mu.build_case(dev, tuple(cnt), 2000 + mc.DECODE_CNTS.index(tuple(cnt)),
                      lambda e: (_dq(Q["q1"][e], Q["s1"][e]), _dq(Q["q3"][e], Q["s3"][e])))
    for k in _knobs():
        with k:
            _run_gateup(c, f"decode {cnt} [{k}]", Q["q1"], Q["s1"], Q["q3"], Q["s3"])
            _run_down(c, Q, f"decode {cnt} [{k}]", mc.MOE_KSPLIT)


# ---- d, e, f: small problems with their own weights --------------------------------------------------------------------------------
def _quant(w):
    """bf16 [G, N, K] -> q int8, s fp32 [G, N], w' float64"""
    from vita_amd.checkpoint import quant_rows_i8
    q = torch.empty(w.shape, dtype=torch.int8, device=w.device)
    s = torch.empty(w.shape[:2], dtype=torch.float32, device=w.device)
    for e in range(w.shape[0]):
        quant_rows_i8(w[e], q=q[e], s=s[e])
    torch.cuda.synchronize()
    return q, s, _dq(q, s)


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
    """1 .. 5 K stages: the stagers' prologue (stage 0, half each), the clamped re-load past the tile's end and the two stagers'
    stage parity, under both load forms (ps_nt); M of one row, one row tile + 1 and 13 row tiles; N with a tail that is no multiple
    of 4, below and above the tile width; grouped (gathered and scattered) and ungrouped (the launcher's rt_cap selection); GLU into
    planes, plain into fp32, and for plain the largest fixed split: one stage per slab.  One quantised [3, 390, K] gate and up
    tensor per K; a case takes its first G groups and N rows (row stride K, group strides of the whole tensor)."""
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
                            w_group_stride=NM * K, group_off=torch.tensor(o.goff, dtype=torch.int32, device=dev), s_group_stride=NM)
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
                    ops.gemm_ps_i8(o.xh, o.xl, wq, ws, w_up=wq3, s_up=ws3, out_split=True, out_planes=(hi, lo), **o.kw)
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
                    ops.gemm_ps_i8(o.xh, o.xl, wq, ws, out=out if ksplit > 1 else out[0], ksplit=ksplit, **o.kw)
                    torch.cuda.synchronize()
                    close(what, b[:, :, :N].double().sum(0)[o.ok], ref, tol_plain)
                    _guards(what, b, M, N, o.live)


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("act", [None, "gelu", "relu", "silu"])
def test_plain_epilogue_terms(dev, act, grouped):
    """the non-GLU, ksplit = 1 epilogue the ABI accepts under int8: act((a q^T) s + bias) scale + resid — the weight scale comes
    BEFORE the bias, as tile_epilogue orders it — written to fp32 C and to the planes in one call.  Bound: atol(K) on this case's
    rms(w'), as for every plain output, NOT widened by the activation's slope or the column scale; plus the fp32 arithmetic of the
    epilogue itself: five roundings (s, bias, act, scale, resid) and an erff / expf of a few ulp, 2^-21 of the magnitudes they act
    on; the planes add their split's 2^-17 |value|."""
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
    tolr[perm] = atol(K, _rms(wp)) + 2.0 ** -21 * ((z.abs() + a.abs()) * scale.double().abs() + resid.double()[perm].abs())
    kw = dict(group_off=torch.tensor(goff, dtype=torch.int32, device=dev), ngroups=G, w_group_stride=N * K, s_group_stride=N) if grouped else {}
    cb, cv = _guarded(M, N, torch.float32, dev)
    hb, hi = _guarded(M, N, torch.bfloat16, dev)
    lb, lo = _guarded(M, N, torch.bfloat16, dev)
    ops.gemm_ps_i8(xh, xl, q, s, bias=bias, act=act, scale=scale, resid=resid, c_rowidx=perm.to(torch.int32), out=cv, out_split=True,
                   out_planes=(hi, lo), **kw)
    torch.cuda.synchronize()
    what = f"epilogue act {act} {'grouped' if grouped else 'ungrouped'}"
    close(what + " C", cv, ref, tolr)
    close(what + " planes", hi.double() + lo.double(), ref, tolr + 2.0 ** -17 * ref.abs())
    assert torch.equal(hi, cv.to(torch.bfloat16)), f"{what}: the hi plane is not C rounded to bf16"
    for b in (cb, hb, lb, resid_b):
        _guards(what, b, M, N)


def _probe_q(N, K, shift, dev):
    """int8 [N, K] in which every column k holds every value -128 .. 127 once per 256 rows, and every row a run of consecutive
    values (so each byte of each 8-byte piece differs from its neighbours): q[n, k] = (n + 37 k + shift) mod 256 - 128."""
    n = torch.arange(N, device=dev).unsqueeze(1)
    k = torch.arange(K, device=dev).unsqueeze(0)
    return ((n + 37 * k + shift) % 256 - 128).to(torch.int8)


def test_conversion_probe_plain_bit_exact(dev):
    """one-hot activation rows (1.0: hi = 1, lo = 0), row m hot at k = m: C[m, n] is ONE weight, q[n, m] s[n], and must equal
    fp32(q) * s bit for bit — every int8 value at every byte position of the stagers' pieces, 3 K stages (the shared stage 0, one of
    either stager), a full 256-row n-tile plus a tail, both load forms.  -128 is never emitted by the quantiser but is accepted by
    the ABI: it is exactly -128 s.  A sign-extension, byte-order or swizzle fault shows as the (n, k) it hits."""
    from vita_amd import ops
    N, K = 256 + 8, 192
    q = _probe_q(N, K, 0, dev)
    assert all(int((q[:256, k] == v).sum()) == 1 for k in (0, 63, 191) for v in (-128, -1, 0, 127))
    s = (torch.arange(N, device=dev, dtype=torch.float32) * 3 + 1001) * 2.0 ** -20     # not powers of two: the multiply rounds
    x = torch.eye(K, device=dev, dtype=torch.float32)
    xh, xl = ops.split_planes(x)
    assert torch.equal(xh.float(), x) and not bool(xl.float().any())
    want = (q.float() * s.unsqueeze(1)).T.contiguous()                                 # [K, N]: fp32(q[n, m]) * s[n], one rounding
    for nt in (-1, 1):
        with Knobs(-1, -1, nt):
            b, out = _guarded(K, N, torch.float32, dev)
            ops.gemm_ps_i8(xh, xl, q, s, out=out)
            torch.cuda.synchronize()
        bad = out != want
        if bool(bad.any()):
            m, n = (int(v) for v in torch.nonzero(bad)[0])
            raise AssertionError(f"conversion probe [nt {nt}]: {int(bad.sum())} of {bad.numel()} differ; first at n {n}, k {m} (stage "
                                 f"{m // 64}, byte {m % 8} of its piece): q {int(q[n, m])}, got {float(out[m, n]):.9g}, want "
                                 f"{float(want[m, n]):.9g}")
        _guards(f"conversion probe [nt {nt}]", b, K, N)


def test_conversion_probe_glu(dev):
    """the same probe through the GLU form (gate and up rows interleaved in the LDS image): g = q1[n, m] s1[n], u = q3[n, m] s3[n]
    are single weights; SiLU is not bit-reproducible, so h is held to the gate|up bound (GEMM bound atol(K) on rms(w') through
    d(SiLU(g) u), plus 2^-16 |h|), which a wrong byte (off by >= one step of s) misses by orders of magnitude."""
    from vita_amd import ops
    N, K = 128 + 8, 192
    q1, q3 = _probe_q(N, K, 0, dev), _probe_q(N, K, 101, dev)
    s1 = (torch.arange(N, device=dev, dtype=torch.float32) * 3 + 1001) * 2.0 ** -17    # |g|, |u| <= ~1.4
    s3 = (torch.arange(N, device=dev, dtype=torch.float32) * 5 + 907) * 2.0 ** -17
    x = torch.eye(K, device=dev, dtype=torch.float32)
    xh, xl = ops.split_planes(x)
    g, u = _dq(q1, s1).T, _dq(q3, s3).T
    tol = mu.glu_tol(g, u, atol(K, max(_rms(g), _rms(u))))
    for nt in (-1, 1):
        with Knobs(-1, -1, nt):
            b, out = _guarded(K, N, torch.float32, dev)
            ops.gemm_ps_i8(xh, xl, q1, s1, w_up=q3, s_up=s3, out=out)
            torch.cuda.synchronize()
        close(f"conversion probe glu [nt {nt}]", out, mu.silu(g) * u, tol)
        _guards(f"conversion probe glu [nt {nt}]", b, K, N)


# ---- g. refusals (the return codes alone, without a GPU: tests/test_experts_int8_cpu.py) --------------------------------------------
def test_refusals_write_nothing(dev):
    from vita_amd import _lib, ops
    M, N, K = 32, 256, 256
    q = torch.ones((9, N, K), dtype=torch.int8, device=dev)
    s = torch.ones((9, N), dtype=torch.float32, device=dev)
    x = torch.ones((M, K), dtype=torch.bfloat16, device=dev)
    goff9 = torch.tensor([0] * 9 + [M], dtype=torch.int32, device=dev)
    nslab = torch.full((1,), 77, dtype=torch.int32, device=dev)
    vec = torch.ones(N, device=dev)
    bufs = {"c": torch.full((8, M, N), SENT, device=dev), "hi": torch.full((M, N), SENT, dtype=torch.bfloat16, device=dev),
            "lo": torch.full((M, N), SENT, dtype=torch.bfloat16, device=dev)}
    planes = dict(out_split=True, out_planes=(bufs["hi"], bufs["lo"]))
    for what, a, kw in [
            ("K % 64 != 0", (x[:, :96], x[:, :96], q[0, :, :96].contiguous(), s[0]), dict(out=bufs["c"][0])),
            ("ksplit > K / 64", (x, x, q[0], s[0]), dict(out=bufs["c"][:5], ksplit=5)),
            ("K split with GLU", (x, x, q[0], s[0]), dict(w_up=q[1], s_up=s[1], out=bufs["c"][:2], ksplit=2)),
            ("device K split with GLU", (x, x, q[0], s[0]), dict(w_up=q[1], s_up=s[1], out=bufs["c"][:2], ksplit=-2, nslab_out=nslab)),
            ("K split with bias", (x, x, q[0], s[0]), dict(bias=vec, out=bufs["c"][:2], ksplit=2)),
            ("K split with act", (x, x, q[0], s[0]), dict(act="silu", out=bufs["c"][:2], ksplit=2)),
            ("K split with scale", (x, x, q[0], s[0]), dict(scale=vec, out=bufs["c"][:2], ksplit=2)),
            ("K split with resid", (x, x, q[0], s[0]), dict(resid=torch.ones((M, N), device=dev), out=bufs["c"][:2], ksplit=2)),
            ("K split with planes", (x, x, q[0], s[0]), dict(out=bufs["c"][:2], ksplit=2, **planes)),
            ("ngroups > 8", (x, x, q, s), dict(out=bufs["c"][0], group_off=goff9, ngroups=9, w_group_stride=N * K, s_group_stride=N))]:
        with pytest.raises(_lib.VitaHipError):
            ops.gemm_ps_i8(*a, **kw)
        torch.cuda.synchronize()
        for nm, b in bufs.items():
            guard(f"refused call ({what}): {nm}", b)
        assert int(nslab.item()) == 77, what
