"""tests/seq_scores.py check_step on rows whose exact log-probabilities are known: it accepts what a row within LOGIT_TOL gives
(a near tie listed in either order included) and rejects a wrong logit, a wrong normaliser, a wrong list, an unsorted list and a
duplicated id — each by the clause that is meant to catch it."""
import numpy as np
import pytest

from tests import logit_rules_ref as lr
from tests.seq_scores import LOGIT_TOL, check_sequence, check_step

K = 20
SIZES = [1000, 51760]


def _row(V, seed=0):
    """a random fp32 row whose 25 largest entries are 6.25e-3 apart (rank 5 - rank 21 = 0.1 exactly up to fp32 rounding, no near
    tie among them) -> (row, ids by rank)."""
    rng = np.random.default_rng(V + seed)
    row = rng.standard_normal(V).astype(np.float32)
    order = np.argsort(-row.astype(np.float64), kind="stable")
    row[order[:25]] = (row[order[25]] + 0.5 + 0.00625 * np.arange(24, -1, -1)).astype(np.float32)
    order = np.lexsort((np.arange(V), -row.astype(np.float64)))
    assert abs(float(row[order[5]]) - float(row[order[21]]) - 0.1) < 1e-6
    return row, order


def _exact(row, token):
    return lr.logprobs(row, token, K)


@pytest.mark.parametrize("V", SIZES)
def test_accepts_exact_logprobs(V):
    assert LOGIT_TOL == 1e-3
    row, order = _row(V)
    for token in (int(order[0]), int(order[7]), int(order[K]), int(order[V // 2])):      # the argmax, a listed one, two unlisted
        tok_lp, ids, top = _exact(row, token)
        assert check_step(row, token, tok_lp, ids, top, K, LOGIT_TOL) == 0.0
    # rows of other seeds, as a sequence; buffers wider than K (the engine's max_logprobs) are read up to K
    rows = np.stack([_row(V, seed)[0] for seed in (1, 2, 3)])
    toks = [int(np.argmax(r)) for r in rows]
    got = [lr.logprobs(r, t, K + 5) for r, t in zip(rows, toks)]
    lp = (np.array([g[0] for g in got]), np.stack([g[1] for g in got]), np.stack([g[2] for g in got]))
    assert check_sequence(rows, toks, lp, K) == 0.0


@pytest.mark.parametrize("V", SIZES)
def test_accepts_a_row_within_the_tolerance(V):
    """every logit moved by a random amount below LOGIT_TOL: inside the derived bound, whatever the signs."""
    row, order = _row(V)
    rng = np.random.default_rng(5)
    dev = (row.astype(np.float64) + rng.uniform(-0.99 * LOGIT_TOL, 0.99 * LOGIT_TOL, V)).astype(np.float32)
    token = int(order[0])
    worst = check_step(row, token, *_exact(dev, token), K, LOGIT_TOL)
    assert 0.0 < worst <= 2 * LOGIT_TOL


@pytest.mark.parametrize("V", SIZES)
def test_accepts_a_near_tie_in_either_order(V):
    row, order = _row(V)
    a, b = int(order[3]), int(order[4])
    row[b] = np.float32(float(row[a]) - 5e-4)
    dev = row.copy()
    dev[a], dev[b] = row[b], row[a]                        # each within 5e-4 of the oracle's: the device lists b before a
    for token in (a, b, int(order[0])):
        tok_lp, ids, top = _exact(dev, token)
        assert ids[3] == b and ids[4] == a
        check_step(row, token, tok_lp, ids, top, K, LOGIT_TOL)
    # the same near tie across the edge of the list: rank K - 1 and rank K
    row, order = _row(V)
    a, b = int(order[K - 1]), int(order[K])
    row[b] = np.float32(float(row[a]) - 5e-4)
    dev = row.copy()
    dev[a], dev[b] = row[b], row[a]
    tok_lp, ids, top = _exact(dev, int(order[0]))
    assert b in ids and a not in ids
    check_step(row, int(order[0]), tok_lp, ids, top, K, LOGIT_TOL)


@pytest.mark.parametrize("V", SIZES)
def test_rejects_one_listed_logit_moved(V):
    row, order = _row(V)
    token = int(order[0])
    for rank, by in ((10, 3e-3), (10, -3e-3), (0, 3e-3)):
        dev = row.copy()
        dev[order[rank]] = np.float32(float(row[order[rank]]) + by)
        with pytest.raises(AssertionError, match="off by"):
            check_step(row, token, *_exact(dev, token), K, LOGIT_TOL)


@pytest.mark.parametrize("V", SIZES)
def test_rejects_a_moved_normaliser(V):
    """the lower half of the vocabulary (by value) shifted by a constant: the 20 largest logits and their order stay, log sum exp
    moves by more than 2e-3 and every log-probability with it."""
    row, order = _row(V)
    token = int(order[0])
    dev = row.copy()
    dev[order[V // 2:]] += np.float32(0.05)
    tok_lp, ids, top = _exact(dev, token)
    assert ids.tolist() == order[:K].tolist() and np.array_equal(dev[ids], row[ids])
    moved = float(lr.log_softmax(row)[token]) - float(tok_lp)
    assert moved > 2 * LOGIT_TOL, moved
    with pytest.raises(AssertionError, match="off by"):
        check_step(row, token, tok_lp, ids, top, K, LOGIT_TOL)
    # the token's own value alone carries a wrong normaliser
    ok = _exact(row, int(order[K + 3]))
    with pytest.raises(AssertionError, match="log-probability of token"):
        check_step(row, int(order[K + 3]), np.float32(ok[0] - 3e-3), ok[1], ok[2], K, LOGIT_TOL)


@pytest.mark.parametrize("V", SIZES)
def test_rejects_a_list_that_is_not_the_top_k(V):
    """rank 21 listed instead of rank 5 (0.1 apart), every listed value exact and the list sorted: only clause (c) can see it."""
    row, order = _row(V)
    token = int(order[0])
    lp = lr.log_softmax(row)
    ids = np.concatenate([order[:5], order[6:K], order[21:22]]).astype(np.int32)
    top = lp[ids]
    assert (np.diff(top) < 0).all()
    with pytest.raises(AssertionError, match="is missing from the top"):
        check_step(row, token, lp[token], ids, top, K, LOGIT_TOL)


@pytest.mark.parametrize("V", SIZES)
def test_rejects_malformed_lists(V):
    row, order = _row(V)
    token = int(order[0])
    tok_lp, ids, top = _exact(row, token)
    i2, t2 = ids.copy(), top.copy()
    i2[[6, 7]], t2[[6, 7]] = ids[[7, 6]], top[[7, 6]]                  # right values, wrong order
    with pytest.raises(AssertionError, match="non-increasing"):
        check_step(row, token, tok_lp, i2, t2, K, LOGIT_TOL)
    i2, t2 = ids.copy(), top.copy()
    i2[7], t2[7] = ids[6], top[6]
    with pytest.raises(AssertionError, match="duplicated"):
        check_step(row, token, tok_lp, i2, t2, K, LOGIT_TOL)
    i2 = ids.copy()
    i2[K - 1] = -1                                                     # an unwritten entry
    with pytest.raises(AssertionError, match="outside the vocabulary"):
        check_step(row, token, tok_lp, i2, top, K, LOGIT_TOL)
    t2 = top.copy()
    t2[K - 1] = -np.inf
    with pytest.raises(AssertionError, match="non-finite"):
        check_step(row, token, tok_lp, ids, t2, K, LOGIT_TOL)
    with pytest.raises(AssertionError, match="non-finite"):
        check_step(row, token, np.float32("nan"), ids, top, K, LOGIT_TOL)
    # the token's value must be its entry of the list, or lie below the list
    with pytest.raises(AssertionError, match="is listed with"):
        check_step(row, token, np.nextafter(tok_lp, np.float32(-1e9)), ids, top, K, LOGIT_TOL)
    out = int(order[K + 2])
    with pytest.raises(AssertionError, match="is not listed"):
        check_step(row, out, top[3], ids, top, K, LOGIT_TOL)


def test_batched_schedule_shape():
    """the schedule of tests/test_batched_scores_gpu.py: the widths in order, everyone joins and leaves once, the first to leave is
    not the last to join, and the longest sequence sits in every lane of a group of four, in both groups of a 4 + 4 iteration and
    alone in the last group of the 4 + 1 and 4 + 4 + 1 iterations."""
    from tests.seq_scores import LENS, batched_schedule, tokens_per_request
    steps = batched_schedule()
    dec = [s[1] for s in steps if s[0] == "decode"]
    assert [len(d) for d in dec] == [2, 2, 3, 3, 4, 4, 5, 5, 8, 8, 9, 9, 8, 7, 7, 6, 6, 5, 4, 3, 2, 1, 1]
    joins, leaves = [s[1] for s in steps if s[0] == "join"], [s[1] for s in steps if s[0] == "leave"]
    assert sorted(joins) == sorted(leaves) == list(range(len(LENS))) and leaves[0] != joins[-1]
    live = set()
    for kind, arg in steps:
        if kind == "decode":
            assert set(arg) == live and len(set(arg)) == len(arg)
        else:
            live = live | {arg} if kind == "join" else live - {arg}
    longest = LENS.index(max(LENS))
    at = {(len(d), d.index(longest)) for d in dec if longest in d}
    assert {p % 4 for _, p in at} == {0, 1, 2, 3} and {(5, 4), (9, 8)} <= at, at
    assert any(w == 8 and p < 4 for w, p in at) and any(w == 8 and p >= 4 for w, p in at), at
    n = tokens_per_request(steps)
    assert sum(n) == len(LENS) + sum(len(d) for d in dec) and max(n) == 24 and min(n) >= 5, n
