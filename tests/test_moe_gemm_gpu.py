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
import pytest
import torch

from tests import moe_gemm_cases as mc
from tests import moe_gemm_util as mu
from tests.moe_gemm_util import GUARD_COLS, GUARD_ROWS, SENT, Knobs, atol
from tests.moe_gemm_util import close as _close
from tests.moe_gemm_util import guard as _guard
from tests.moe_gemm_util import randn as _randn

pytestmark = pytest.mark.gpu

H, I, E = mc.H, mc.I, mc.E


def _knobs():
    """every case under the auto selection and under each forced ps_cfg x ps_xcd x ps_nt (forcing ps_cfg 2 is what takes the few-row
    cases, avg <= 64, to the specialised kernel's schedule; forcing 0 / 1 runs the 8-wave forms at the released widths)."""
    return [Knobs(c, x, n) for c in (-1, 0, 1, 2) for x in (0, 3) for n in (-1, 0, 1)]


# ---- data (recipe, operands and references: tests/moe_gemm_util.py) ---------------------------------------------------------------
@pytest.fixture(scope="module")
def W(dev):
    """w1, w3 [E, I, H] and w2 [E, H, I] bf16 (~2.8 GB), qkv [6144, H] and o [H, H]."""
    w = mu.make_weights(dev)
    yield w
    w.clear()
    torch.cuda.empty_cache()


_CACHE = {}


@pytest.fixture(scope="module")
def cases(dev, W):
    """lazily built per-case operands and float64 references, shared by the tests of this module."""
    def get(name):
        if name not in _CACHE:
            _CACHE[name] = mu.build_case(dev, mc.CASES[name].rows, 1000 + list(mc.CASES).index(name),
                                         lambda e: (W["w1"][e].double(), W["w3"][e].double()))
        return _CACHE[name]
    yield get
    _CACHE.clear()
    torch.cuda.empty_cache()


# ---- runners (checks: tests/moe_gemm_util.py run_gateup / run_down) -----------------------------------------------------------------
def _run_gateup(c, W, what, n0=0, n1=I):
    """gate|up of columns [n0, n1) (one TP rank's shard) into guarded planes; checks values, lo as a residual, guards."""
    from vita_amd import ops
    mu.run_gateup(c, what, lambda hi, lo: ops.gemm_ps(c.x_hi, c.x_lo, W["w1"][:, n0:n1], w_up=W["w3"][:, n0:n1], a_rowidx=c.tok,
                                                      group_off=c.goff, ngroups=E, w_group_stride=I * H, m=c.M, out_split=True,
                                                      out_planes=(hi, lo)), n0, n1)


def _run_down(c, W, what, ksplit, k0=0, k1=I, w2s=None, n0=0, n1=H):
    """down projection (K range [k0, k1) of w2, output columns [n0, n1)) scattered through c_rowidx into guarded slabs."""
    from vita_amd import ops
    K = k1 - k0
    if w2s is None:
        assert (k0, k1) == (0, I)
        w = W["w2"][:, n0:n1]
        a_hi, a_lo = c.h_hi, c.h_lo
    else:
        w = w2s[:, n0:n1]
        a_hi, a_lo = c.h_hi[:, k0:k1], c.h_lo[:, k0:k1]
    ref = mu.down_ref(c, k0, k1, lambda e: (w2s[e] if w2s is not None else W["w2"][e, :, k0:k1]).double())
    return mu.run_down(c, what, ksplit, K, ref,
                       lambda out, nslab: ops.gemm_ps(a_hi, a_lo, w, group_off=c.goff, ngroups=E, w_group_stride=H * K, c_rowidx=c.slot,
                                                      m=c.M, out=out, ksplit=ksplit, nslab_out=nslab), n0, n1)


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
