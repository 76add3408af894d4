"""numpy restatement of the logit rules contract (include/vita_hip.h vh_logit_rules): the token table of a request, the penalty
arithmetic (every step one IEEE fp32 operation) and the log-probabilities of a raw row (double, rounded to fp32 once)."""
import numpy as np

PROMPT_BIT = np.uint32(0x80000000)


def seen_table(V, prompt_ids=(), output_ids=()):
    """uint32 [V]: bit 31 = the id occurs in the prompt (a set), low bits = how often it occurs in the output."""
    t = np.zeros(V, dtype=np.uint32)
    if len(prompt_ids):
        t[np.unique(np.asarray(prompt_ids, dtype=np.int64))] |= PROMPT_BIT
    if len(output_ids):
        t += np.bincount(np.asarray(output_ids, dtype=np.int64), minlength=V).astype(np.uint32)
    return t


def penalise(row, seen, r=1.0, f=0.0, p=0.0):
    """fp32 row as selection sees it: 1. seen at all: x > 0 ? x / r : x * r; 2. x - f * (float)count; 3. count > 0: x - p."""
    x = np.asarray(row, dtype=np.float32).copy()
    seen = np.asarray(seen).astype(np.uint32)
    cnt = seen & np.uint32(0x7FFFFFFF)
    r, f, p = np.float32(r), np.float32(f), np.float32(p)
    with np.errstate(all="ignore"):
        rep = np.where(x > 0, x / r, x * r).astype(np.float32)
        x = np.where(seen != 0, rep, x).astype(np.float32)
        x = (x - (f * cnt.astype(np.float32)).astype(np.float32)).astype(np.float32)
        x = np.where(cnt > 0, (x - p).astype(np.float32), x).astype(np.float32)
    return x


def canon(row):
    """NaN ranks as -inf, -0 is 0 (as the device's ordering keys)."""
    x = np.asarray(row, dtype=np.float32).copy()
    x[np.isnan(x)] = -np.inf
    x[x == 0] = 0.0
    return x


def log_softmax(row):
    """fp32 [V]: x - (M + log sum exp(x - M)) in double, rounded once; nothing finite: -inf everywhere."""
    x = canon(row).astype(np.float64)
    M = x.max()
    if not M > -np.inf:
        return np.full(x.shape, -np.inf, dtype=np.float32)
    with np.errstate(all="ignore"):
        lse = M + np.log(np.sum(np.exp(x - M)))
        return (x - lse).astype(np.float32)


def logprobs(row, token, K):
    """-> (logprob of `token`, top-K ids int32 [K], top-K logprobs fp32 [K]) of a raw row; the top K ordered by (logit descending,
    id ascending), entries past the vocabulary id -1 and -inf."""
    x = canon(row)
    lp = log_softmax(row)
    V = x.shape[0]
    order = np.lexsort((np.arange(V), -x.astype(np.float64)))[:K]
    ids = np.full(K, -1, dtype=np.int32)
    top = np.full(K, -np.inf, dtype=np.float32)
    ids[:len(order)] = order
    top[:len(order)] = lp[order]
    return np.float32(lp[int(token)]), ids, top
