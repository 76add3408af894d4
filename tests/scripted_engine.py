"""The scripted engine of the scheduler's CPU tests: the seq_* surface of MixtralEngine over reference-counted 64-token pages, without a
GPU.  It keeps what was WRITTEN in its pages and computes a sequence's next token from what its page table reads back (tokens =
f(history); prompt rows are one-hot ids), so a preempted and re-prefilled request must continue exactly where it was, and a wrong page
in a table, a page evicted while in use or a row written into a shared page shows as a wrong id (or trips the model's own assertion).
`calls` records every mutating call with its arguments, in order."""
import types

import numpy as np
import torch

V = 97
BATCH = ("seq_prefill_batch",)
SHARING = ("page_refs", "seq_hold_prefix", "pages_release", "seq_adopt")


class _Cfg:
    def __init__(self, max_seqs):
        self.max_seqs = max_seqs


def next_token(hist):
    h = 7
    for t in hist:
        h = (h * 31 + int(t) + 3) % 1000003
    return h % V


class ScriptedEngine:
    """batch=False: no seq_prefill_batch attribute (the batcher probes it with hasattr); sharing=False: none of the page-sharing
    entries; fail={"seq_adopt": 2}: the second seq_adopt call raises before it touches anything (recorded as ("fail", name, n))."""
    V = V
    K = 3                                 # top-K width of logprobs()
    _absent = ()

    def __init__(self, pool_tokens, max_seqs, max_new=64, max_prefill=512, batch=True, sharing=True, fail=None):
        self._absent = (() if batch else BATCH) + (() if sharing else SHARING)
        self.c = _Cfg(max_seqs)
        self.max_ctx, self.max_new, self.max_prefill = pool_tokens, max_new, max_prefill
        self.n_pages = pool_tokens // 64
        self._free = list(range(self.n_pages - 1, -1, -1))        # a stack
        self.refs = [0] * self.n_pages
        self.data = [[None] * 64 for _ in range(self.n_pages)]
        self.seqs = {}
        self.calls = []
        self.fail, self._seen = dict(fail or {}), {}

    def __getattribute__(self, name):
        if name in object.__getattribute__(self, "_absent"):
            raise AttributeError(name)
        return object.__getattribute__(self, name)

    def _script(self, name):
        n = self._seen[name] = self._seen.get(name, 0) + 1
        if self.fail.get(name) == n:
            self.calls.append(("fail", name, n))
            raise RuntimeError(f"scripted failure of {name} call {n}")

    def trace(self, *names):
        """the recorded calls of these names"""
        return [c for c in self.calls if c[0] in names]

    # ---- pool
    @property
    def free(self):
        return self.pages_free()

    def pages_free(self):
        assert len(self._free) == sum(1 for r in self.refs if r == 0)
        return len(self._free)

    def _unref(self, pg):
        assert self.refs[pg] >= 1
        self.refs[pg] -= 1
        if self.refs[pg] == 0:
            self._free.append(pg)

    def _hist(self, q):
        h = [self.data[q["pages"][p // 64]][p % 64] for p in range(q["pos"])]
        assert None not in h, "a sequence reads a row nobody wrote"
        return h

    def _short(self, q, n):
        """pages that n more rows of q take from the pool"""
        return -(-(q["pos"] + n) // 64) - len(q["pages"])

    def _write(self, q, ids):
        need = self._short(q, len(ids))
        if need > len(self._free):
            raise RuntimeError("KV pool exhausted")
        for _ in range(need):
            pg = self._free.pop()
            self.refs[pg] = 1
            self.data[pg] = [None] * 64
            q["pages"].append(pg)
        for t in ids:
            pg = q["pages"][q["pos"] // 64]
            assert self.refs[pg] == 1, "the engine writes a row of a page whose count is above 1"
            self.data[pg][q["pos"] % 64] = int(t)
            q["pos"] += 1

    def _feed(self, q, ids):
        self._write(q, ids)
        q["toks"] = [next_token(self._hist(q))]

    # ---- sequences
    def seq_alloc(self):
        self._script("seq_alloc")
        for s in range(self.c.max_seqs):
            if s not in self.seqs:
                self.seqs[s] = dict(pos=0, toks=[], pages=[])
                self.calls.append(("alloc", s))
                return s
        raise RuntimeError("no slot")

    def seq_free(self, s):
        for pg in reversed(self.seqs.pop(s)["pages"]):
            self._unref(pg)
        self.calls.append(("free", s))

    def seq_prefill(self, s, emb):
        self._script("seq_prefill")
        self._feed(self.seqs[s], emb.argmax(dim=1).tolist())
        self.calls.append(("prefill", s, int(emb.shape[0])))

    def seq_prefill_batch(self, seqs, embs):
        """checks the whole call before it touches anything, as the C entry point does"""
        self._script("seq_prefill_batch")
        lens = [int(e.shape[0]) for e in embs]
        if len(set(seqs)) != len(seqs) or sum(lens) > self.max_prefill:
            raise RuntimeError("batch rejected")
        if sum(self._short(self.seqs[s], n) for s, n in zip(seqs, lens)) > len(self._free):
            raise RuntimeError("KV pool exhausted")
        for s, e in zip(seqs, embs):
            self._feed(self.seqs[s], e.argmax(dim=1).tolist())
        self.calls.append(("prefill_batch", tuple(seqs), tuple(lens)))

    def seq_decode(self, seqs):
        for s in seqs:
            q = self.seqs[s]
            self._write(q, [q["toks"][-1]])
            q["toks"].append(next_token(self._hist(q)))
        self.calls.append(("decode", tuple(seqs)))

    def seq_set_sampling(self, s, draw0=0, **kw):
        self._script("seq_set_sampling")
        assert s in self.seqs
        self.calls.append(("set_sampling", s, int(draw0), kw))

    def seq_set_logit_rules(self, s, prompt_ids=None, output_ids=None, **kw):
        self._script("seq_set_logit_rules")
        assert s in self.seqs
        self.calls.append(("set_logit_rules", s, tuple(prompt_ids), tuple(output_ids), kw))

    def seq_pos(self, s):
        return self.seqs[s]["pos"]

    def seq_pages(self, s):
        return list(self.seqs[s]["pages"])

    def seq_tokens(self, s):
        return torch.tensor(self.seqs[s]["toks"] + [0] * (self.max_new - len(self.seqs[s]["toks"])))

    def seq_counters(self, s):
        return torch.tensor([self.seqs[s]["pos"], len(self.seqs[s]["toks"]), 0, 0])

    def check_device_flag(self, c):
        return c

    def logprobs(self, s):
        """(chosen id's logprob -(token + 1/4), top-K ids token + 1 .. token + K, their logprobs -(id + 1/2)) per token"""
        toks = self.seq_tokens(s)
        ids = torch.stack([toks + j + 1 for j in range(self.K)], dim=1).to(torch.int32)
        return -toks.float() - 0.25, ids, -(ids.float() + 0.5)

    # ---- shared pages
    def page_refs(self, pg):
        return self.refs[pg] if 0 <= pg < self.n_pages else -1

    def seq_hold_prefix(self, s, n):
        q = self.seqs[s]
        assert 1 <= n and 64 * n <= q["pos"], "hold past the position"
        for pg in q["pages"][:n]:
            self.refs[pg] += 1
        self.calls.append(("hold", s, n))
        return list(q["pages"][:n])

    def pages_release(self, pages):
        for pg in set(pages):
            assert self.refs[pg] >= pages.count(pg) >= 1, "release of a page that is not held"
        for pg in reversed(pages):
            self._unref(pg)
        self.calls.append(("release", tuple(pages)))

    def seq_adopt(self, s, pages):
        self._script("seq_adopt")
        q = self.seqs[s]
        assert q["pos"] == 0 and not q["pages"] and len(set(pages)) == len(pages) >= 1
        assert all(self.refs[pg] >= 1 for pg in pages), "adopting a free page"
        for pg in pages:
            self.refs[pg] += 1
        q["pages"], q["pos"] = list(pages), 64 * len(pages)
        self.calls.append(("adopt", s, tuple(pages)))


def _emb(ids):
    return torch.nn.functional.one_hot(torch.tensor(ids), V).float()


def embed_tokens(ids):
    """the batcher's embed_tokens hook for this engine"""
    return torch.nn.functional.one_hot(ids, V).float()


def _expected(ids, n):
    hist, out = list(ids), []
    for _ in range(n):
        out.append(next_token(hist))
        hist.append(out[-1])
    return out


def _ids(seed, n):
    return np.random.default_rng(seed).integers(1, V, size=n).tolist()


def _drain(bt, limit=10000):
    got, fin = {}, {}
    for _ in range(limit):
        if not bt.has_work():
            return got, fin
        for rid, new, finished, reason in bt.step():
            got.setdefault(rid, []).extend(new)
            if finished:
                fin[rid] = reason
    raise AssertionError("scheduler did not terminate")


class _Tok:
    def decode(self, ids, skip_special_tokens=False):
        return " ".join(str(i) for i in ids)


class FakeLLM:
    """the surface AsyncLLMEngine uses: model.engine / model.device / model.model.embed_tokens, _prepare, _embed, tokenizer."""

    def __init__(self, pool_tokens=64 * 16, max_seqs=3):
        eng = ScriptedEngine(pool_tokens, max_seqs, max_new=64, batch=False, sharing=False)
        table = torch.eye(V)
        self.model = types.SimpleNamespace(engine=eng, device=torch.device("cpu"),
                                           model=types.SimpleNamespace(embed_tokens=lambda ids: table[ids]))
        self.tokenizer = _Tok()

    def _prepare(self, inputs, sp):
        ids = list(inputs["prompt_token_ids"])
        if any(i < 0 for i in ids):
            raise ValueError("placeholder without data")
        return dict(ids=ids, max_tokens=min(sp.max_tokens, 64), eos=set(sp.stop_token_ids or []))

    def _embed(self, req):
        return _emb(req["ids"])


def no_cuda_sync(monkeypatch):
    """what each module's autouse fixture applies: the batcher's one synchronisation per step becomes a no-op"""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: type("S", (), {"synchronize": lambda self: None})())
