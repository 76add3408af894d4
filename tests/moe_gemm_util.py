"""Machinery shared by the streaming MoE GEMM tests at the released widths (tests/test_moe_gemm_gpu.py: bf16 weights through
ops.gemm_ps; tests/test_moe_gemm_i8_gpu.py: int8 weights through ops.gemm_ps_i8; tests/test_moe_gemm_mxfp4_gpu.py: MXFP4 weights
through ops.gemm_ps_mxfp4): tolerances, the vh_tune knob context, the seeded weight recipe, per-case operands with float64
references, and the gate|up / down runners with their checks.  What differs between the forms — how the GEMM is called and which
weights the reference sees — is passed in as callables."""
import math

import torch

from tests import moe_gemm_cases as mc

H, I, E = mc.H, mc.I, mc.E
W_STD = 0.02
SENT = 7.0                   # guard value: exact in fp32 and bf16, never a result
GUARD_ROWS, GUARD_COLS = 16, 64


def atol(K, w_rms=W_STD):
    return 3e-4 * (w_rms / 0.05) * math.sqrt(K / 4096)


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


def randn(gen, shape, dev, std=1.0):
    return torch.randn(shape, generator=gen, device=dev, dtype=torch.float32).mul_(std)


def close(what, got, ref, tol):
    """got (any float dtype) vs float64 ref, elementwise |got - ref| <= tol (scalar or tensor)."""
    d = (got.double() - ref).abs()
    bad = ~(d <= tol)                                     # NaN counts as bad
    if d.numel():
        ratio = torch.where(d > 0, d / tol, torch.zeros_like(d))     # an exact element under a zero bound (a zero weight row) counts 0
        print(f"{what}: max|diff| {float(d.max()):.3g}, worst |diff| / tol {float(ratio.max()):.3g}")
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        t = tol if not torch.is_tensor(tol) else float(tol.reshape(-1)[i])
        raise AssertionError(f"{what}: {int(bad.sum())} of {d.numel()} outside tolerance; first flat {i} (row {i // ref.shape[-1]}): "
                             f"got {float(got.reshape(-1)[i]):.7g} ref {float(ref.reshape(-1)[i]):.7g} tol {t:.3g}; "
                             f"max|diff| {float(d.nan_to_num(float('inf')).max()):.3g}")


def guard(what, t):
    if not bool((t == SENT).all()):
        n = int((t != SENT).sum())
        raise AssertionError(f"{what}: {n} of {t.numel()} guard values overwritten")


def silu(x):
    return x * torch.sigmoid(x)


def glu_tol(g, u, gemm_tol):
    """bound of SiLU(g) u given the GEMM bound of g and u: carried through d(SiLU(g) u), plus 2^-16 |h| for the fp32 epilogue and
    the output split."""
    sg = torch.sigmoid(g)
    dsilu = sg * (1 + g * (1 - sg))
    return gemm_tol * (dsilu.abs() * u.abs() + silu(g).abs()) + 2.0 ** -16 * (silu(g) * u).abs()


E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def dq_mxfp4(codes, scales):
    """w' = e2m1(code) 2^(byte - 127) in float64 on the tensors' device: packed codes uint8 [.., K / 2] (element k in byte k >> 1, low
    nibble for even k), E8M0 scale bytes uint8 [.., K / 32] -> [.., K].  Code 8 (-0) is 0."""
    lut = torch.tensor(E2M1 + tuple(-v for v in E2M1), dtype=torch.float64, device=codes.device)
    c = torch.stack([codes & 15, codes >> 4], -1).reshape(*codes.shape[:-1], -1).long()
    X = torch.pow(torch.tensor(2.0, dtype=torch.float64, device=codes.device), scales.double() - 127)
    return (lut[c].reshape(*scales.shape, 32) * X.unsqueeze(-1)).reshape(c.shape)


def mxfp4_probe(dev, N, K, shift, ring):
    """the conversion probes' operand: codes [N, K / 2] with code (n + k + shift) % 16 at element k of row n, scale bytes [N, K / 32]
    with ring[(block + n) % len(ring)]"""
    k = torch.arange(K, device=dev)
    n = torch.arange(N, device=dev)
    code = ((n[:, None] + k[None, :] + shift) % 16).to(torch.uint8)
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    ring = torch.tensor(ring, dtype=torch.uint8, device=dev)
    scales = ring[(torch.arange(K // 32, device=dev)[None, :] + n[:, None]) % len(ring)].contiguous()
    return codes, scales


def make_weights(dev, plain=True):
    """w1, w3 [E, I, H] and w2 [E, H, I] bf16 (~2.8 GB) and, with plain, qkv [6144, H] and o [H, H] (drawn after the experts):
    N(0, 0.02^2) from one seeded generator."""
    gen = torch.Generator(device=dev).manual_seed(20261015)
    w = {k: torch.empty(shape, dtype=torch.bfloat16, device=dev) for k, shape in
         (("w1", (E, I, H)), ("w3", (E, I, H)), ("w2", (E, H, I)))}
    for k in ("w1", "w3", "w2"):
        for e in range(E):
            w[k][e] = randn(gen, w[k].shape[1:], dev, W_STD)          # fp32 -> bf16 copy rounds to nearest even
    if plain:
        w["qkv"] = randn(gen, (mc.NQKV, H), dev, W_STD).to(torch.bfloat16)
        w["o"] = randn(gen, (H, H), dev, W_STD).to(torch.bfloat16)
    torch.cuda.synchronize()
    return w


class CaseData:
    pass


def build_case(dev, rows, seed, gate_up_w, gemm_tol=None):
    """operands and float64 gate|up reference of one routing (rows per expert).  gate_up_w(e) -> (w1[e], w3[e]) as float64 [I, H].
    gemm_tol: the GEMM bound of g and u (atol(H) on the seeded recipe's rms unless the caller has its own weights' rms)."""
    from vita_amd import ops
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
    x = randn(gen, (S, H), dev)
    c.x_hi, c.x_lo = ops.split_planes(x)
    g = torch.empty((M, I), dtype=torch.float64, device=dev)
    u = torch.empty((M, I), dtype=torch.float64, device=dev)
    for e in range(E):
        if rows[e]:
            xe = x[c.tok[goff[e]:goff[e + 1]].long()].double()
            w1, w3 = gate_up_w(e)
            g[goff[e]:goff[e + 1]] = xe @ w1.T
            del w1
            u[goff[e]:goff[e + 1]] = xe @ w3.T
            del w3
    c.h_ref = silu(g) * u
    c.h_tol = glu_tol(g, u, atol(H) if gemm_tol is None else gemm_tol)
    del g, u
    # down: its own N(0, 1) input rows, scattered to (token, slot) rows of an output with guard rows no index targets
    hin = randn(gen, (M, I), dev)
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


def down_ref(c, k0, k1, down_w):
    """float64 [R, H] of the K range [k0, k1) (guard rows 0), cached on the case.  down_w(e) -> w2[e][:, k0:k1] as float64."""
    if (k0, k1) not in c.y_ref:
        y = torch.zeros((c.R, H), dtype=torch.float64, device=c.hin.device)
        for e in range(E):
            b, n = c.goff_list[e], c.goff_list[e + 1]
            if n > b:
                y[c.slot[b:n].long()] = c.hin[b:n, k0:k1].double() @ down_w(e).T
        c.y_ref[(k0, k1)] = y
    return c.y_ref[(k0, k1)]


def run_gateup(c, what, gemm, n0=0, n1=I):
    """gate|up of columns [n0, n1) (one TP rank's shard) into guarded planes; checks values, lo as a residual, guards.
    gemm(hi, lo) runs the GEMM into the two bf16 [M, N] views."""
    N = n1 - n0
    hi_b = torch.full((c.M + GUARD_ROWS, N + GUARD_COLS), SENT, dtype=torch.bfloat16, device=c.x_hi.device)
    lo_b = torch.full_like(hi_b, SENT)
    hi, lo = hi_b[:c.M, :N], lo_b[:c.M, :N]
    gemm(hi, lo)
    torch.cuda.synchronize()
    close(f"{what} gate|up hi + lo", hi.double() + lo.double(), c.h_ref[:, n0:n1], c.h_tol[:, n0:n1])
    bad = lo.double().abs() > 2.0 ** -7 * hi.double().abs()
    assert not bool(bad.any()), f"{what}: lo is not a residual of hi at {int(bad.sum())} elements"
    for nm, b in (("hi", hi_b), ("lo", lo_b)):
        guard(f"{what} {nm} guard rows", b[c.M:])
        guard(f"{what} {nm} guard columns", b[:, N:])


def run_down(c, what, ksplit, K, ref, gemm, n0=0, n1=H, tol=None):
    """down projection (a K range of w2 of K columns, output columns [n0, n1)) scattered through c_rowidx into guarded slabs.
    gemm(out, nslab) runs it (nslab: the device int of a device-chosen split, else None); ref: float64 [R, H] of that K range;
    tol: the bound (atol(K) on the seeded recipe's rms unless the caller has its own weights' rms)."""
    dev = c.hin.device
    N = n1 - n0
    nsl = abs(ksplit)
    buf = torch.full((nsl, c.R, N + GUARD_COLS), SENT, dtype=torch.float32, device=dev)
    out = buf[:, :, :N] if nsl > 1 or ksplit < 0 else buf[0, :, :N]
    nslab = torch.zeros(1, dtype=torch.int32, device=dev)
    gemm(out, nslab if ksplit < 0 else None)
    torch.cuda.synchronize()
    ks = nsl
    if ksplit < 0:
        ks = int(nslab.item())
        assert 1 <= ks <= nsl, f"{what}: reported K split {ks} outside 1 .. {nsl}"
        guard(f"{what} slabs {ks}.. above the reported count", buf[ks:])
    elif ksplit <= 1:
        ks = 1
    close(f"{what} down (ksplit {ksplit} -> {ks} slabs)", buf[:ks, :, :N].double().sum(0)[c.live], ref[:, n0:n1][c.live],
          atol(K) if tol is None else tol)
    guard(f"{what} guard rows", buf[:ks, ~c.live])
    guard(f"{what} guard columns", buf[:ks, :, N:])
    return ks
