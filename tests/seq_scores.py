"""Score-level check of one generated token of a served sequence against the oracle's raw logits row of that step.

What a sequence with logprobs = K keeps per generated token (include/vita_hip.h vh_logit_rules; MixtralEngine.logprobs(s)) is the
chosen token's log-probability and the top-K ids and log-probabilities of its RAW row.  The top K pin individual logits; the
normaliser log sum exp depends on the whole row.

The bound is derived, not measured.  The project's bar for a decode step's scores is "every logit within LOGIT_TOL of the oracle's"
(tests/test_mixtral_gpu.py LOGIT_TOL, tests/test_long_context_gpu.py LOGIT_TOL: 1e-3, restated here).  log sum exp is 1-Lipschitz
in the sup norm, so if every logit is within LOGIT_TOL of the oracle's, every log-probability x_i - lse(x) is within 2 LOGIT_TOL;
and two logits can change order only if the oracle has them closer than 2 LOGIT_TOL.  A near tie in the oracle's row therefore
passes in either order; nothing else is excused."""
import numpy as np

from tests import logit_rules_ref as lr

LOGIT_TOL = 1e-3       # tests/test_mixtral_gpu.py, tests/test_long_context_gpu.py: "every step's logits within 1e-3"


def check_step(ref_row, token, dev_token_lp, dev_ids, dev_top, K, logit_tol=LOGIT_TOL, what="step"):
    """assert that (dev_token_lp, dev_ids[:K], dev_top[:K]) — the device's log-probability of `token` and its top-K list — are what
    a row within logit_tol of ref_row (the oracle's raw logits, [V]) gives.  -> the largest log-probability error met."""
    ref_row = np.asarray(ref_row)
    V = ref_row.shape[0]
    assert 0 < K <= V, (K, V)
    ids = np.asarray(dev_ids).astype(np.int64)[:K]
    top = np.asarray(dev_top, dtype=np.float32)[:K]
    tok_lp = np.float32(dev_token_lp)
    token = int(token)
    bound = 2.0 * logit_tol
    lp_ref = lr.log_softmax(ref_row).astype(np.float64)
    x = lr.canon(ref_row).astype(np.float64)

    # (b) a well-formed list: K valid, distinct ids, finite values in non-increasing order; the token's own value is the list's
    # entry when the token is listed (logit_rules_ref.logprobs: both are the same row's log-probability of that id) and no larger
    # than the list's smallest otherwise
    assert ids.shape == (K,) and top.shape == (K,), f"{what}: {ids.shape}, {top.shape} for K = {K}"
    assert ((ids >= 0) & (ids < V)).all(), f"{what}: ids outside the vocabulary: {ids.tolist()}"
    assert np.unique(ids).size == K, f"{what}: duplicated ids in the top {K}: {ids.tolist()}"
    assert np.isfinite(top).all() and np.isfinite(tok_lp), f"{what}: non-finite log-probabilities {top.tolist()}, token {tok_lp}"
    assert (np.diff(top) <= 0).all(), f"{what}: the top {K} log-probabilities are not in non-increasing order: {top.tolist()}"
    assert 0 <= token < V, f"{what}: token {token} outside the vocabulary"
    at = np.flatnonzero(ids == token)
    if at.size:
        assert tok_lp == top[at[0]], f"{what}: token {token} is listed with {top[at[0]]!r} but its own log-probability is {tok_lp!r}"
    else:
        assert tok_lp <= top[-1], f"{what}: token {token} is not listed but its log-probability {tok_lp!r} exceeds {top[-1]!r}"

    # (a) the values
    err = np.abs(top.astype(np.float64) - lp_ref[ids])
    worst = int(np.argmax(err))
    assert err[worst] <= bound, (f"{what}: log-probability of id {ids[worst]} (rank {worst}) is {top[worst]!r}, the oracle's "
                                 f"{lp_ref[ids[worst]]!r}: off by {err[worst]:.3e} > {bound:.1e}")
    terr = abs(float(tok_lp) - lp_ref[token])
    assert terr <= bound, f"{what}: log-probability of token {token} is {tok_lp!r}, the oracle's {lp_ref[token]!r}: off by {terr:.3e}"

    # (c) a valid top K of the oracle's row up to near ties
    rest = np.ones(V, bool)
    rest[ids] = False
    if rest.any():
        lo, out_hi = float(x[ids].min()), float(x[rest].max())
        assert lo >= out_hi - bound, (f"{what}: id {int(np.flatnonzero(rest)[np.argmax(x[rest])])} (oracle logit {out_hi!r}) is missing "
                                      f"from the top {K}, whose smallest oracle logit is {lo!r} (id {int(ids[np.argmin(x[ids])])})")
    return float(max(err[worst], terr))


def check_sequence(rows, tokens, lp, K, logit_tol=LOGIT_TOL, what="sequence"):
    """check_step for generated tokens 0 ... len(tokens) - 1 of one sequence: rows [n, V] the oracle's rows, lp = (token logprobs
    [>= n], top ids [>= n, >= K], top logprobs [>= n, >= K]) as numpy arrays (MixtralEngine.logprobs(s) copied to the host)."""
    tok_lp, top_id, top = lp
    return max(check_step(rows[i], tokens[i], tok_lp[i], top_id[i], top[i], K, logit_tol, what=f"{what}, generated token {i}")
               for i in range(len(tokens)))


# ---- the schedule of tests/test_batched_scores_gpu.py (pure Python, checked by tests/test_seq_scores_cpu.py) ------------------------
# prompt lengths; 63, 64 and 128 cross a page (= attention split) boundary within their first two decode steps
LENS = [5, 40, 63, 64, 97, 130, 20, 75, 128]
JOIN = [[5, 2], [3], [0], [8], [1, 4, 6], [7]]       # indices into LENS: widths 2, 3, 4, 5, 8, 9; the 75-token prompt joins last
LEAVE = [3, 0, 5, 8, 1, 7, 4, 6]                     # the 64-token prompt leaves first; the 63-token one is left and runs alone


def batched_schedule():
    """-> list of ("join", i) | ("decode", [i, ...]) | ("leave", i), i an index into LENS: two iterations at every width on the way
    up (2, 3, 4, 5, 8, 9) and at 7, 6 and 1 on the way down, one at the widths that were already run.  The decode list is the
    live list rotated by 4 * iteration + 2 places: groups of four are cut from it in order, so a sequence changes lane and group
    from one iteration to the next."""
    steps, live, it = [], [], 0

    def run(n_iter):
        nonlocal it
        for _ in range(n_iter):
            r = (4 * it + 2) % len(live)
            steps.append(("decode", live[r:] + live[:r]))
            it += 1

    for group in JOIN:
        for i in group:
            steps.append(("join", i))
            live.append(i)
        run(2)
    for i in LEAVE:
        steps.append(("leave", i))
        live.remove(i)
        run(2 if len(live) in (7, 6, 1) else 1)
    steps.append(("leave", live[0]))
    return steps


def tokens_per_request(steps):
    """generated tokens of every request under `steps`: the prefill's token and one per iteration it takes part in."""
    n = [1] * len(LENS)
    for kind, arg in steps:
        if kind == "decode":
            for i in arg:
                n[i] += 1
    return n
