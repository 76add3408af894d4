"""The prefill's weight-streaming GEMMs (vh_gemm_ps / vh_gemm_sp.hip) at the released widths — H = 4096, I = 14336, E = 8 and the TP
shards of I — against float64 references of the same operation on the same bf16 weights, across the tile schedule (cases and why each
exists: tests/moe_gemm_cases.py; which schedule paths they reach: tests/test_moe_gemm_sched_cpu.py).

Operands: activations N(0, 1) fp32, split into bf16 hi / lo planes by ops.split_planes as the engine does; weights N(0, 0.02^2), generated
on the device from a seeded generator and rounded to bf16 (RNE).  References: torch float64 matmuls on the device, one expert at a time,
on the fp32 activations (so the plane split's own 2^-17 is inside the measured error).

Tolerance (the exact-mode model of tests/test_ops_gpu.py: every product carries the activation to ~2^-17, sums in fp32): the error of
one output grows like sqrt(K) x rms(a) x rms(w).  test_ops_gpu.py's gemm_ps tests use atol 3e-4 at K = 4096 with rms(w) = 0.05; scaled
to rms(w) = 0.02 that is 1.2e-4, and by sqrt(K / 4096) from there: 2.2e-4 at K = 14336 (down), 1.7e-4 / 1.2e-4 / 8.5e-5 / 6.0e-5 at
K = 7168 / 4096 / 3584 / 1792.  The outputs are O(1) (gate and up rms 1.3, down rms 2.4 at K = 14336); a missing lo plane costs
~1e-3, a lost row or tile the whole value.  Gate|up is SiLU(g) u emitted as bf16 planes: its bound is the GEMM bound carried through
d(SiLU(g) u) plus 2^-16 |h| for the fp32 epilogue and the output split."""
import math

import pytest
import torch

from tests import moe_gemm_cases as mc

pytestmark = pytest.mark.gpu

H, I, E = mc.H, mc.I, mc.E
W_STD = 0.02
SENT = 7.0                   # guard value: exact in fp32 and bf16, never a result
GUARD_ROWS, GUARD_COLS = 16, 64


def atol(K):
    return 3e-4 * (W_STD / 0.05) * math.sqrt(K / 4096)


class Knobs:
    """vh_tune settings for one run; every knob goes back to its default (-1) afterwards, as the ps_cfg fixture of test_ops_gpu.py."""

    def __init__(self, cfg=-1, xcd=-1, nt=-1):
        self.kv = {"ps_cfg": cfg, "ps_xcd": xcd, "ps_nt": nt}

    def __enter__(self):
        from vita_amd import _lib
        for k, v in self.kv.items():
            _lib.tune(k, v)
        return self

    def __exit__(self, *exc):
        from vita_amd import _lib
        for k in self.kv:
            _lib.tune(k, -1)

    def __repr__(self):
        return ",".join(f"{k}={v}" for k, v in self.kv.items())


def _knobs():
    """every case under the auto selection and under each forced ps_cfg x ps_xcd x ps_nt (forcing ps_cfg 2 is what takes the few-row
    cases, avg <= 64, to the specialised kernel's schedule; forcing 0 / 1 runs the 8-wave forms at the released widths)."""
    return [Knobs(c, x, n) for c in (-1, 0, 1, 2) for x in (0, 3) for n in (-1, 0, 1)]


def _randn(gen, shape, dev, std=1.0):
    return torch.randn(shape, generator=gen, device=dev, dtype=torch.float32).mul_(std)


def _close(what, got, ref, tol):
    """got (any float dtype) vs float64 ref, elementwise |got - ref| <= tol (scalar or tensor)."""
    d = (got.double() - ref).abs()
    bad = ~(d <= tol)                                     # NaN counts as bad
    if d.numel():
        print(f"{what}: max|diff| {float(d.max()):.3g}, worst |diff| / tol {float((d / tol).max()):.3g}")
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        t = tol if not torch.is_tensor(tol) else float(tol.reshape(-1)[i])
        raise AssertionError(f"{what}: {int(bad.sum())} of {d.numel()} outside tolerance; first flat {i} (row {i // ref.shape[-1]}): "
                             f"got {float(got.reshape(-1)[i]):.7g} ref {float(ref.reshape(-1)[i]):.7g} tol {t:.3g}; "
                             f"max|diff| {float(d.nan_to_num(float('inf')).max()):.3g}")


def _guard(what, t):
    if not bool((t == SENT).all()):
        n = int((t != SENT).sum())
        raise AssertionError(f"{what}: {n} of {t.numel()} guard values overwritten")


# ---- data ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def W(dev):
    """w1, w3 [E, I, H] and w2 [E, H, I] bf16 (~2.8 GB), qkv [6144, H] and o [H, H]."""
    gen = torch.Generator(device=dev).manual_seed(20261015)
    w = {k: torch.empty(shape, dtype=torch.bfloat16, device=dev) for k, shape in
         (("w1", (E, I, H)), ("w3", (E, I, H)), ("w2", (E, H, I)))}
    for k in ("w1", "w3", "w2"):
        for e in range(E):
            w[k][e] = _randn(gen, w[k].shape[1:], dev, W_STD)          # fp32 -> bf16 copy rounds to nearest even
    w["qkv"] = _randn(gen, (mc.NQKV, H), dev, W_STD).to(torch.bfloat16)
    w["o"] = _randn(gen, (H, H), dev, W_STD).to(torch.bfloat16)
    torch.cuda.synchronize()
    yield w
    w.clear()
    torch.cuda.empty_cache()


class CaseData:
    pass


_CACHE = {}


@pytest.fixture(scope="module")
def cases(dev, W):
    """lazily built per-case operands and float64 references, shared by the tests of this module."""
    def get(name):
        if name not in _CACHE:
            _CACHE[name] = _build_case(dev, W, name)
        return _CACHE[name]
    yield get
    _CACHE.clear()
    torch.cuda.empty_cache()


def _silu(x):
    return x * torch.sigmoid(x)


def _build_case(dev, W, name):
    from vita_amd import ops
    rows = mc.CASES[name].rows
    seed = 1000 + list(mc.CASES).index(name)
    gen = torch.Generator(device=dev).manual_seed(seed)
    cg = torch.Generator().manual_seed(seed)
    c = CaseData()
    c.rows, c.M = rows, sum(rows)
    goff = [0]
    for r in rows:
        goff.append(goff[-1] + r)
    c.goff_list = goff
    c.goff = torch.tensor(goff, dtype=torch.int32, device=dev)
    M = c.M
    # gate|up: tokens gathered in sorted order (each token twice, as top-2 routing; ascending inside an expert)
    S = (M + 1) // 2
    tok = torch.randperm(M, generator=cg) // 2
    for e in range(E):
        tok[goff[e]:goff[e + 1]] = tok[goff[e]:goff[e + 1]].sort().values
    c.tok = tok.to(torch.int32).to(dev)
    x = _randn(gen, (S, H), dev)
    c.x_hi, c.x_lo = ops.split_planes(x)
    g = torch.empty((M, I), dtype=torch.float64, device=dev)
    u = torch.empty((M, I), dtype=torch.float64, device=dev)
    for e in range(E):
        if rows[e]:
            xe = x[c.tok[goff[e]:goff[e + 1]].long()].double()
            g[goff[e]:goff[e + 1]] = xe @ W["w1"][e].double().T
            u[goff[e]:goff[e + 1]] = xe @ W["w3"][e].double().T
    c.h_ref = _silu(g) * u
    sg = torch.sigmoid(g)
    dsilu = sg * (1 + g * (1 - sg))
    c.h_tol = atol(H) * (dsilu.abs() * u.abs() + _silu(g).abs()) + 2.0 ** -16 * c.h_ref.abs()
    del g, u, sg, dsilu
    # down: its own N(0, 1) input rows, scattered to (token, slot) rows of an output with guard rows no index targets
    hin = _randn(gen, (M, I), dev)
    c.hin = hin
    c.h_hi, c.h_lo = ops.split_planes(hin)
    c.R = M + GUARD_ROWS
    slots = torch.randperm(c.R, generator=cg)
    c.guard_rows = slots[:GUARD_ROWS].sort().values.to(dev)
    c.slot = slots[GUARD_ROWS:].to(torch.int32).to(dev)
    c.live = torch.ones(c.R, dtype=torch.bool, device=dev)
    c.live[c.guard_rows] = False
    c.y_ref = {}                   # (k0, k1) K range -> float64 [R, H] (guard rows 0)
    torch.cuda.synchronize()
    return c


def _down_ref(c, W, k0, k1, w2s=None):
    if (k0, k1) not in c.y_ref:
        y = torch.zeros((c.R, H), dtype=torch.float64, device=c.hin.device)
        w2 = W["w2"] if w2s is None else w2s
        for e in range(E):
            b, n = c.goff_list[e], c.goff_list[e + 1]
            if n > b:
                we = w2[e].double() if w2s is not None else w2[e, :, k0:k1].double()
                y[c.slot[b:n].long()] = c.hin[b:n, k0:k1].double() @ we.T
        c.y_ref[(k0, k1)] = y
    return c.y_ref[(k0, k1)]


# ---- runners + checks ------------------------------------------------------------------------------------------------------------
def _run_gateup(c, W, what, n0=0, n1=I):
    """gate|up of columns [n0, n1) (one TP rank's shard) into guarded planes; checks values, lo as a residual, guards."""
    from vita_amd import ops
    N = n1 - n0
    hi_b = torch.full((c.M + GUARD_ROWS, N + GUARD_COLS), SENT, dtype=torch.bfloat16, device=c.x_hi.device)
    lo_b = torch.full_like(hi_b, SENT)
    hi, lo = hi_b[:c.M, :N], lo_b[:c.M, :N]
    ops.gemm_ps(c.x_hi, c.x_lo, W["w1"][:, n0:n1], w_up=W["w3"][:, n0:n1], a_rowidx=c.tok, group_off=c.goff, ngroups=E,
                w_group_stride=I * H, m=c.M, out_split=True, out_planes=(hi, lo))
    torch.cuda.synchronize()
    _close(f"{what} gate|up hi + lo", hi.double() + lo.double(), c.h_ref[:, n0:n1], c.h_tol[:, n0:n1])
    bad = lo.double().abs() > 2.0 ** -7 * hi.double().abs()
    assert not bool(bad.any()), f"{what}: lo is not a residual of hi at {int(bad.sum())} elements"
    for nm, b in (("hi", hi_b), ("lo", lo_b)):
        _guard(f"{what} {nm} guard rows", b[c.M:])
        _guard(f"{what} {nm} guard columns", b[:, N:])


def _run_down(c, W, what, ksplit, k0=0, k1=I, w2s=None, n0=0, n1=H):
    """down projection (K range [k0, k1) of w2, output columns [n0, n1)) scattered through c_rowidx into guarded slabs."""
    from vita_amd import ops
    dev = c.hin.device
    K, N = k1 - k0, n1 - n0
    nsl = abs(ksplit)
    buf = torch.full((nsl, c.R, N + GUARD_COLS), SENT, dtype=torch.float32, device=dev)
    out = buf[:, :, :N] if nsl > 1 or ksplit < 0 else buf[0, :, :N]
    nslab = torch.zeros(1, dtype=torch.int32, device=dev)
    if w2s is None:
        assert (k0, k1) == (0, I)
        w = W["w2"][:, n0:n1]
        a_hi, a_lo = c.h_hi, c.h_lo
    else:
        w = w2s[:, n0:n1]
        a_hi, a_lo = c.h_hi[:, k0:k1], c.h_lo[:, k0:k1]
    gs = H * K
    ops.gemm_ps(a_hi, a_lo, w, group_off=c.goff, ngroups=E, w_group_stride=gs, c_rowidx=c.slot, m=c.M, out=out, ksplit=ksplit,
                nslab_out=nslab if ksplit < 0 else None)
    torch.cuda.synchronize()
    ks = nsl
    if ksplit < 0:
        ks = int(nslab.item())
        assert 1 <= ks <= nsl, f"{what}: reported K split {ks} outside 1 .. {nsl}"
        _guard(f"{what} slabs {ks}.. above the reported count", buf[ks:])
    elif ksplit <= 1:
        ks = 1
    ref = _down_ref(c, W, k0, k1, w2s)[:, n0:n1]
    _close(f"{what} down (ksplit {ksplit} -> {ks} slabs)", buf[:ks, :, :N].double().sum(0)[c.live], ref[c.live], atol(K))
    _guard(f"{what} guard rows", buf[:ks, ~c.live])
    _guard(f"{what} guard columns", buf[:ks, :, N:])
    return ks


# ---- tests -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.CASES))
def test_gateup_released_width(dev, W, cases, name):
    c = cases(name)
    for k in _knobs():
        with k:
            _run_gateup(c, W, f"{name} [{k}]")


@pytest.mark.parametrize("name", list(mc.CASES))
def test_down_released_width(dev, W, cases, name):
    """the engine's device-chosen split (ksplit = -4, count through nslab_out) and fixed splits of 1, 2, 3 under every knob set."""
    c = cases(name)
    for k in _knobs():
        with k:
            for ksplit in (mc.MOE_KSPLIT, 1, 2, 3):
                _run_down(c, W, f"{name} [{k}]", ksplit)


@pytest.mark.parametrize("tp", [2, 4, 8])
@pytest.mark.parametrize("name", mc.TP_CASES)
def test_tp_shards(dev, W, cases, name, tp):
    """every rank's shard of I (gate|up N = I / TP, down K = I / TP: 28 K-steps at TP = 8), and the down projection's two overlap
    column halves (N = 2048) per rank, all in this process; both placements."""
    c = cases(name)
    it = I // tp
    for r in range(tp):
        k0, k1 = r * it, (r + 1) * it
        w2s = W["w2"][:, :, k0:k1].contiguous()
        for x in (0, 3):
            with Knobs(-1, x):
                _run_gateup(c, W, f"{name} tp{tp} rank {r} [xcd {x}]", k0, k1)
                _run_down(c, W, f"{name} tp{tp} rank {r} [xcd {x}]", mc.MOE_KSPLIT, k0, k1, w2s)
                for hh in range(2):
                    _run_down(c, W, f"{name} tp{tp} rank {r} half {hh} [xcd {x}]", mc.MOE_KSPLIT, k0, k1, w2s,
                              hh * (H // 2), (hh + 1) * (H // 2))
        del w2s
        c.y_ref.pop((k0, k1), None)


@pytest.mark.parametrize("proj", ["qkv", "o"])
def test_plain_projections(dev, W, proj):
    """the QKV (N = 6144, the engine's -qkv_slabs = -4) and O (N = 4096, ksplit = -8) projections on the same kernel: no groups, K split
    chosen on device, M from one token to a 4600-token prefill; both placements (which the plain GEMMs ignore: same bits)."""
    from vita_amd import ops
    w = W[proj]
    N = w.shape[0]
    ksplit = mc.QKV_KSPLIT if proj == "qkv" else mc.O_KSPLIT
    gen = torch.Generator(device=dev).manual_seed(77 if proj == "qkv" else 78)
    for M in mc.PLAIN_M:
        x = _randn(gen, (M, H), dev)
        xh, xl = ops.split_planes(x)
        ref = x.double() @ w.double().T
        prev = None
        for xcd in (0, 3):
            buf = torch.full((-ksplit, M + GUARD_ROWS, N + GUARD_COLS), SENT, dtype=torch.float32, device=dev)
            nslab = torch.zeros(1, dtype=torch.int32, device=dev)
            with Knobs(-1, xcd):
                ops.gemm_ps(xh, xl, w, out=buf[:, :M, :N], ksplit=ksplit, nslab_out=nslab)
            torch.cuda.synchronize()
            ks = int(nslab.item())
            what = f"{proj} M={M} [xcd {xcd}]"
            assert 1 <= ks <= -ksplit, f"{what}: reported K split {ks}"
            _close(f"{what} ({ks} slabs)", buf[:ks, :M, :N].double().sum(0), ref, atol(H))
            _guard(f"{what} slabs above the count", buf[ks:])
            _guard(f"{what} guard rows", buf[:ks, M:])
            _guard(f"{what} guard columns", buf[:ks, :, N:])
            if prev is not None:
                assert torch.equal(prev, buf), f"{what}: ps_xcd changed a plain GEMM's result"
            prev = buf
