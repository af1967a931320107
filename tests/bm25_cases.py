"""Scaffolding shared by tests/test_bm25_ops.py and tests/test_bm25_device.py:
synthetic postings built straight from seeded tensors, the queries of the
GPU sweeps, a float64 reference and the contract check of a BM25 result. A
plain module, no fixtures; everything is deterministic and cached once per
process.

BM25 ties are the rule, not the exception (a one-term query over documents
of few distinct lengths), so id lists are never compared directly:
`check()` is the contract.
"""

import torch

from nornicdb_amd.ops import BM25Postings

NEG_INF = float("-inf")

K1, B = 1.2, 0.75

_cache = {}


def tolerance(t_count, ref_max):
    """4 (T + 8) 2^-24 max(ref), per query. A contribution takes at most 6
    fp32 roundings, summing T terms at most T - 1 more, rounding w, c0 and
    c1 to fp32 at most 3 more: T + 8 in all, each at most 2^-24 relative to
    a partial sum that never exceeds the largest score; the bound carries a
    factor 4 over that."""
    return 4.0 * (t_count + 8) * 2.0 ** -24 * ref_max


def make_postings(n, lengths, seed, special=None, uniform=False):
    """CPU BM25Postings over n documents: term t is held by lengths[t]
    random documents (ascending slots); `special` maps a term id to an
    explicit slot list. tf is 1..5 and doc_len 5..200, or with `uniform`
    every tf is 1 and every doc_len 40, so that a whole list ties."""
    g = torch.Generator().manual_seed(seed)
    docs = []
    for t, ln in enumerate(lengths):
        if special and t in special:
            d = torch.tensor(sorted(special[t]), dtype=torch.int64)
        else:
            d = torch.randperm(n, generator=g)[:ln].sort().values
        docs.append(d)
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor([len(d) for d in docs]), 0)
    post_doc = torch.cat(docs).to(torch.int32)
    m = post_doc.shape[0]
    if uniform:
        post_tf = torch.ones(m, dtype=torch.int32)
        doc_len = torch.full((n,), 40, dtype=torch.int32)
    else:
        post_tf = torch.randint(1, 6, (m,), generator=g).to(torch.int32)
        doc_len = torch.randint(5, 201, (n,), generator=g).to(torch.int32)
    return BM25Postings(off, post_doc, post_tf, doc_len, n)


def to_device(p, device):
    return BM25Postings(p.post_off.to(device), p.post_doc.to(device),
                        p.post_tf.to(device), p.doc_len.to(device), p.n_docs)


def constants(p):
    """(c0, c1) of the postings' own average length."""
    avg = float(p.doc_len.double().mean()) if p.n_docs else 1.0
    return K1 * (1 - B), K1 * B / avg


def dense_ref(p, q_terms, q_w, c0, c1):
    """float64 [Q, n] scores from the fp32 w, c0 and c1, summed in column
    order with plain slices of the CSR arrays; CPU tensors."""
    off = p.post_off.tolist()
    c0 = float(torch.tensor(c0, dtype=torch.float32))
    c1 = float(torch.tensor(c1, dtype=torch.float32))
    w = q_w.float().double()
    ref = torch.zeros(q_terms.shape[0], p.n_docs, dtype=torch.float64)
    for r, row in enumerate(q_terms.tolist()):
        for t, term in enumerate(row):
            if not 0 <= term < len(off) - 1:
                continue
            sl = slice(off[term], off[term + 1])
            d = p.post_doc[sl].long()
            tf = p.post_tf[sl].double()
            dl = p.doc_len[d].double()
            ref[r, d] += w[r, t] * tf / (tf + c0 + c1 * dl)
    return ref


def check(t_count, ref, allow, k, s, i):
    """The contract of a (scores [Q, k], slots [Q, k]) result. t_count: the
    queries' term columns, T; ref: float64 [Q, n] scores (dense_ref) on s's
    device; allow: bool [n] or None."""
    if s.is_cuda:
        torch.cuda.synchronize()
    q_count, n = ref.shape
    assert s.shape == (q_count, k) and i.shape == s.shape
    assert i.dtype == torch.int64 and s.dtype == torch.float32
    ok = ref > 0                       # touched
    if allow is not None:
        ok = ok & allow[None, :]
    kk = min(k, n)
    masked = ref.masked_fill(~ok, NEG_INF)
    rs = torch.full((q_count, k), NEG_INF, dtype=torch.float64,
                    device=ref.device)
    if kk:
        rs[:, :kk] = torch.topk(masked, kk, dim=-1).values
    m = ok.sum(-1).clamp_max(k)
    filled = torch.arange(k, device=s.device)[None, :] < m[:, None]
    assert ((i == -1) == ~filled).all(), i
    assert (s[~filled] == NEG_INF).all(), s
    loc = torch.where(filled, i, 0)
    assert ((loc >= 0) & (loc < max(n, 1))).all(), i
    if n:
        assert (torch.gather(ok, 1, loc) | ~filled).all(), \
            "a document that is untouched or not allowed was returned"
    srt = torch.where(filled, loc, -1 - torch.arange(k, device=s.device)) \
        .sort(dim=-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "duplicate hit"
    assert (s[:, :-1] >= s[:, 1:]).all(), "scores not descending"
    ref_max = ref.max(-1).values if n else \
        torch.zeros(q_count, dtype=torch.float64, device=ref.device)
    tol = tolerance(t_count, ref_max)[:, None].expand(-1, k)
    if filled.any():
        sd = s.double()
        err = ((sd - rs).abs() / tol)[filled].max().item()
        own = ((torch.gather(ref, 1, loc) - sd).abs() / tol)[filled] \
            .max().item()
        print(f"Q={q_count} k={k} T={t_count}: rank err {err:.3f} of the "
              f"tolerance, own err {own:.3f}")
        assert err <= 1.0, err
        assert own <= 1.0, own

