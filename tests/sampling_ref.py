"""numpy restatement of the seeded sampling contract (include/vita_hip.h, vh_sampling; INTEGRATION.md "Sampling").

    z_i = (double)logit_i / T                     (NaN logits rank as -inf)
    top-k: keep z_i >= z_(k)                      (ties at the boundary kept)
    top-p: on the softmax of the top-k-kept set, keep i iff the mass of kept values strictly above z_i is < top_p
    token = argmax over kept i of z_i + G_i       (lowest index on ties; 0 when nothing finite is kept)
    G_i = -log(-log(u)), u = ((x >> 11) + 0.5) 2^-53, x = word i & 3 of Philox4x64-10, key (seed, 0), counter (i >> 2, draw, 0, 0)

T = 0 is greedy (the plain argmax).  T and top_p are the float32 values the C struct carries.
"""
import numpy as np

M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
_MASK32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhilo(a, m):
    """(hi, lo) of the 128-bit product of uint64 array a and the constant m."""
    a0, a1 = a & _MASK32, a >> _S32
    m0, m1 = np.uint64(m & 0xFFFFFFFF), np.uint64(m >> 32)
    p00, p01, p10, p11 = a0 * m0, a0 * m1, a1 * m0, a1 * m1
    mid = (p00 >> _S32) + (p01 & _MASK32) + (p10 & _MASK32)
    hi = p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)
    return hi, a * np.uint64(m)


def philox4x64(c0, c1, c2, c3, k0, k1):
    """Philox4x64-10 (Random123) of counters (c0, c1, c2, c3) under key (k0, k1): four uint64 arrays (the output words)."""
    with np.errstate(over="ignore"):
        x = [np.asarray(c, dtype=np.uint64).copy() for c in np.broadcast_arrays(c0, c1, c2, c3)]
        k0, k1 = np.uint64(k0), np.uint64(k1)
        for r in range(10):
            if r:
                k0, k1 = k0 + np.uint64(W0), k1 + np.uint64(W1)
            hi0, lo0 = _mulhilo(x[0], M0)
            hi1, lo1 = _mulhilo(x[2], M1)
            x = [hi1 ^ x[1] ^ k0, lo1, hi0 ^ x[3] ^ k1, lo0]
    return x


def gumbel(seed, draw, idx):
    """G_i of vocab indices idx (int array) at draw index `draw` under `seed`, in double."""
    idx = np.asarray(idx, dtype=np.int64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x64((idx >> 2).astype(np.uint64), np.uint64(int(draw) & 0xFFFFFFFFFFFFFFFF), np.uint64(0), np.uint64(0), seed, 0)
    x = np.choose((idx & 3).astype(np.int64), words)
    u = ((x >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    return -np.log(-np.log(u))


def scaled(logits, temperature):
    c = np.array(logits, dtype=np.float32)
    c[np.isnan(c)] = -np.inf
    return c.astype(np.float64) / np.float64(np.float32(temperature))


def keep_mask(logits, temperature, top_k=0, top_p=1.0):
    """the kept set of a row (bool [V]) under top-k then top-p."""
    z = scaled(logits, temperature)
    V = z.shape[0]
    keep = np.ones(V, dtype=bool)
    if 0 < top_k < V:
        keep = z >= np.sort(z)[::-1][top_k - 1]
    tp = float(np.float32(top_p))
    if tp < 1.0:
        zmax = z[keep].max()
        if zmax == -np.inf:
            return keep
        if zmax == np.inf:
            return keep & (z == np.inf)
        e = np.where(keep, np.exp(np.where(keep, z, zmax) - zmax), 0.0)
        target = tp * e.sum()
        vals, inv = np.unique(np.where(keep, z, -np.inf), return_inverse=True)   # ascending distinct values
        mass = np.bincount(inv.ravel(), weights=e, minlength=vals.shape[0])[::-1]    # per value, descending
        above = np.cumsum(mass) - mass                                               # mass strictly above each value
        kept_vals = vals[::-1][above < target]
        keep &= z >= kept_vals.min()
    return keep


def perturbed(logits, temperature, top_k, top_p, seed, draw):
    """z + G over the kept set, -inf elsewhere."""
    z = scaled(logits, temperature)
    keep = keep_mask(logits, temperature, top_k, top_p)
    with np.errstate(invalid="ignore"):
        return np.where(keep, z + gumbel(seed, draw, np.arange(z.shape[0])), -np.inf)


def sample(logits, temperature, top_k=0, top_p=1.0, seed=0, draw=0):
    """the token the contract draws from one row of logits."""
    if float(np.float32(temperature)) == 0.0:
        c = np.array(logits, dtype=np.float32)
        c[np.isnan(c)] = -np.inf
        return int(np.argmax(c)) if np.any(c > -np.inf) else 0
    s = perturbed(logits, temperature, top_k, top_p, seed, draw)
    return int(np.argmax(s)) if np.any(s > -np.inf) else 0


def top2_gap(logits, temperature, top_k, top_p, seed, draw):
    """gap between the two largest perturbed scores (what a disagreement with the device would be measured against)."""
    s = np.sort(perturbed(logits, temperature, top_k, top_p, seed, draw))[::-1]
    return float(s[0] - s[1]) if s.shape[0] > 1 else float("inf")


def filtered_softmax(logits, temperature, top_k=0, top_p=1.0):
    """the exact distribution a draw follows: softmax of z over the kept set."""
    z = scaled(logits, temperature)
    keep = keep_mask(logits, temperature, top_k, top_p)
    e = np.where(keep, np.exp(np.where(keep, z, 0.0) - z[keep].max()), 0.0)
    return e / e.sum()
