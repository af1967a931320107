"""ops.bm25: the torch oracle on the CPU, and the fused bm25_scan kernel
against it on the GPU under the contract of tests/bm25_cases.py."""

import pytest
import torch

from nornicdb_amd.ops import (bm25_build_postings, bm25_search,
                              bm25_search_exact, require_native)

from bm25_cases import (NEG_INF, check, constants, dense_ref, make_postings,
                        to_device)

_cache = {}


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def _py_scores(p, terms, weights, c0, c1):
    """{slot: score} of one query by a plain Python loop over the CSR
    arrays, in float64 from the fp32 w, c0 and c1."""
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    off, doc, tf, dl = (t.tolist() for t in
                        (p.post_off, p.post_doc, p.post_tf, p.doc_len))
    c0, c1 = f32(c0), f32(c1)
    scores = {}
    for term, w in zip(terms, weights):
        if not 0 <= term < len(off) - 1:
            continue
        for e in range(off[term], off[term + 1]):
            d = doc[e]
            scores[d] = scores.get(d, 0.0) + \
                f32(w) * tf[e] / (tf[e] + c0 + c1 * dl[d])
    return scores


def _small():
    if "small" not in _cache:
        p = make_postings(300, [0, 1, 7, 40, 150, 299, 300, 20], seed=3)
        _cache["small"] = (p, constants(p))
    return _cache["small"]


def test_build_postings_sorts_by_term_and_slot():
    term_docs = [{5: 2, 1: 1, 3: 4}, {}, {2: 7}, {4: 1, 0: 3}]
    p = bm25_build_postings(term_docs, [3, 1, 9, 4, 2, 6])
    assert p.n_docs == 6 and p.n_terms == 4
    assert p.post_off.tolist() == [0, 3, 3, 4, 6]
    assert p.post_doc.tolist() == [1, 3, 5, 2, 0, 4]
    assert p.post_tf.tolist() == [1, 4, 2, 7, 3, 1]
    assert p.doc_len.tolist() == [3, 1, 9, 4, 2, 6]
    assert p.post_off.dtype == torch.int64
    assert p.post_doc.dtype == p.post_tf.dtype == p.doc_len.dtype == \
        torch.int32


def test_cpu_exact_matches_python_loop():
    p, (c0, c1) = _small()
    g = torch.Generator().manual_seed(0)
    q_terms = torch.tensor([[3, 4, 5, -1], [2, 7, -1, -1], [6, 1, 3, 4]],
                           dtype=torch.int32)
    q_w = torch.rand(3, 4, generator=g) * 3 + 0.25
    allow = torch.rand(300, generator=g) < 0.6
    for mask in (None, allow):
        s, i = bm25_search_exact(p, q_terms, q_w, c0, c1, 12, allow=mask)
        assert s.shape == (3, 12) and s.dtype == torch.float32
        assert i.dtype == torch.int64
        for r in range(3):
            want = _py_scores(p, q_terms[r].tolist(), q_w[r].tolist(), c0, c1)
            if mask is not None:
                want = {d: v for d, v in want.items() if mask[d]}
            top = sorted(want.values(), reverse=True)[:12]
            assert len(top) == 12
            assert torch.allclose(s[r].double(), torch.tensor(top, dtype=torch.float64),
                                  rtol=1e-6, atol=0)
            for sc, d in zip(s[r].tolist(), i[r].tolist()):
                assert abs(want[d] - sc) <= 1e-6 * want[d]
        # bm25_search on CPU tensors is the oracle
        s2, i2 = bm25_search(p, q_terms, q_w, c0, c1, 12, allow=mask)
        assert torch.equal(s, s2) and torch.equal(i, i2)
        check(4, dense_ref(p, q_terms, q_w, c0, c1), mask, 12, s, i)


def test_cpu_only_touched_documents_are_hits():
    p, (c0, c1) = _small()
    q_terms = torch.tensor([[2, 1]], dtype=torch.int32)   # 7 + 1 postings
    q_w = torch.ones(1, 2)
    s, i = bm25_search_exact(p, q_terms, q_w, c0, c1, 20)
    touched = set(p.post_doc[p.post_off[1]:p.post_off[3]].tolist())
    m = len(touched)
    assert m <= 8
    assert set(i[0, :m].tolist()) == touched
    assert (i[0, m:] == -1).all() and (s[0, m:] == NEG_INF).all()
    assert (s[0, :m] > 0).all()
    # k beyond the corpus still pads
    s, i = bm25_search_exact(p, q_terms, q_w, c0, c1, 400)
    assert s.shape == (1, 400) and (i[0, m:] == -1).all()


def test_cpu_term_in_two_columns_counts_twice():
    p, (c0, c1) = _small()
    once = torch.tensor([[3]], dtype=torch.int32)
    twice = torch.tensor([[3, 3]], dtype=torch.int32)
    s1, i1 = bm25_search_exact(p, once, torch.full((1, 1), 1.5), c0, c1, 40)
    s2, i2 = bm25_search_exact(p, twice, torch.full((1, 2), 1.5), c0, c1, 40)
    a = dict(zip(i1[0].tolist(), s1[0].tolist()))
    b = dict(zip(i2[0].tolist(), s2[0].tolist()))
    assert a.keys() == b.keys() and len(a) == 40
    for d in a:
        assert b[d] == pytest.approx(2 * a[d], rel=1e-6)


def test_cpu_out_of_range_ids_are_skipped():
    p, (c0, c1) = _small()
    clean = torch.tensor([[4, -1, -1, 2]], dtype=torch.int32)
    noisy = torch.tensor([[4, p.n_terms, -7, 2]], dtype=torch.int32)
    w = torch.tensor([[1.0, 9.0, 9.0, 2.0]])
    sa, ia = bm25_search_exact(p, clean, w, c0, c1, 25)
    sb, ib = bm25_search_exact(p, noisy, w, c0, c1, 25)
    assert torch.equal(sa, sb) and torch.equal(ia, ib)
    none = torch.tensor([[-1, p.n_terms + 3, 0]], dtype=torch.int32)  # 0: empty
    s, i = bm25_search_exact(p, none, torch.ones(1, 3), c0, c1, 5)
    assert (i == -1).all() and (s == NEG_INF).all()


def test_host_function_rejects_cpu_tensors():
    nat = require_native()
    assert nat.BM25_RANGE == 8192
    p, (c0, c1) = _small()
    with pytest.raises(RuntimeError, match="bm25_scan"):
        nat.bm25_scan(p.post_off, p.post_doc, p.post_tf, p.doc_len,
                      torch.zeros(1, 2, dtype=torch.int32), torch.ones(1, 2),
                      c0, c1, 10, None)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

FIXED = [0, 1, 63, 64, 65, 4097]
T_MAX = 6


def _range():
    return int(require_native().BM25_RANGE)


def _big():
    """(postings on the CPU, on the GPU, (c0, c1)): n = 2 R + 37. Terms
    0..5 have the FIXED lengths, term 6 sits on the range borders, term 7
    is held by 60 % of the documents, the rest are random."""
    if "big" not in _cache:
        r = _range()
        n = 2 * r + 37
        g = torch.Generator().manual_seed(11)
        rand = torch.randint(2, 3000, (8,), generator=g).tolist()
        lengths = FIXED + [6, (n * 3) // 5] + rand
        border = [r - 1, r, 2 * r - 1, 2 * r, 0, n - 1]
        cpu = make_postings(n, lengths, seed=12, special={6: border})
        _cache["big"] = (cpu, to_device(cpu, "cuda"), constants(cpu))
    return _cache["big"]


def _queries(q_count):
    """(q_terms int32 [Q, T_MAX], q_w, ref float64 [Q, n], masks) for the
    big postings, the tensors on the GPU. Every query has its own T, padded
    with -1; query 0 names the border list and the short lists, query 1 (if
    any) only ids that are skipped, query 2 one term in two columns and an
    out-of-range id. allow: a random half of the documents, minus every
    query's best document."""
    key = ("queries", q_count)
    if key not in _cache:
        cpu, _, (c0, c1) = _big()
        g = torch.Generator().manual_seed(q_count)
        v = cpu.n_terms
        q_terms = torch.full((q_count, T_MAX), -1, dtype=torch.int32)
        q_terms[0] = torch.tensor([6, 1, 5, 2, 3, 4])
        for r in range(1, q_count):
            t = 1 + (r % T_MAX)
            q_terms[r, :t] = torch.randperm(v, generator=g)[:t] \
                .to(torch.int32)
        if q_count > 1:
            q_terms[1] = torch.tensor([-1, v, 0, v + 5, -3, -1])
        if q_count > 2:
            q_terms[2] = torch.tensor([7, 9, 7, v + 1, 6, -1])
        q_w = torch.rand(q_count, T_MAX, generator=g) * 3 + 0.25
        ref = dense_ref(cpu, q_terms, q_w, c0, c1)
        allow = torch.rand(cpu.n_docs, generator=g) < 0.5
        best = ref.argmax(-1)
        allow[best] = False
        _cache[key] = (q_terms.cuda(), q_w.cuda(), ref.cuda(), allow.cuda(),
                       best.cuda())
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("k", [1, 10, 16, 17, 40, 64, 65])
@pytest.mark.parametrize("q_count", [1, 3, 16])
def test_gpu_scan_sweep(q_count, k, masked):
    """k <= 64 is the kernel, 65 the dense torch route."""
    _, gpu, (c0, c1) = _big()
    q_terms, q_w, ref, allow, best = _queries(q_count)
    mask = allow if masked else None
    s, i = bm25_search(gpu, q_terms, q_w, c0, c1, k, allow=mask)
    check(T_MAX, ref, mask, k, s, i)
    if q_count > 1:   # every term of query 1 is skipped
        assert (i[1] == -1).all() and (s[1] == NEG_INF).all()
    if masked:   # every query's best document is disallowed
        assert not (i == best[:, None]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["one", "r-1", "r", "r+1"])
def test_gpu_scan_small_n(which):
    r = _range()
    n = {"one": 1, "r-1": r - 1, "r": r, "r+1": r + 1}[which]
    lengths = [min(n, ln) for ln in (1, 64, n, 500, 0)]
    special = {0: [n - 1]}
    cpu = make_postings(n, lengths, seed=n, special=special)
    gpu = to_device(cpu, "cuda")
    c0, c1 = constants(cpu)
    q_terms = torch.tensor([[0, 3, 2, 1]], dtype=torch.int32)
    q_w = torch.tensor([[2.0, 0.5, 1.25, 3.0]])
    ref = dense_ref(cpu, q_terms, q_w, c0, c1).cuda()
    allow = torch.ones(n, dtype=torch.bool)
    allow[::3] = False
    for mask in (None, allow.cuda()):
        for k in (10, 64):
            s, i = bm25_search(gpu, q_terms.cuda(), q_w.cuda(), c0, c1, k,
                               allow=mask)
            check(4, ref, mask, k, s, i)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_gpu_scan_forced_multi_range_walk(monkeypatch, masked):
    """NORNICDB_BM25_BLOCKS=2: the 3 ranges go to 2 blocks, so block 0
    walks two ranges and carries its best K across them; at Q = 3 every
    query has a single block for all three."""
    monkeypatch.setenv("NORNICDB_BM25_BLOCKS", "2")
    _, gpu, (c0, c1) = _big()
    for q_count in (1, 3):
        q_terms, q_w, ref, allow, _ = _queries(q_count)
        mask = allow if masked else None
        for k in (10, 64):
            s, i = bm25_search(gpu, q_terms, q_w, c0, c1, k, allow=mask)
            check(T_MAX, ref, mask, k, s, i)


@pytest.mark.gpu
def test_gpu_scan_is_deterministic():
    _, gpu, (c0, c1) = _big()
    q_terms, q_w, _, allow, _ = _queries(16)
    for mask in (None, allow):
        for k in (10, 40):
            s1, i1 = bm25_search(gpu, q_terms, q_w, c0, c1, k, allow=mask)
            s2, i2 = bm25_search(gpu, q_terms, q_w, c0, c1, k, allow=mask)
            assert torch.equal(s1, s2) and torch.equal(i1, i2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 64])
def test_gpu_scan_whole_list_ties(k):
    """doc_len all equal and tf all 1: every document of a list has the
    same score, so the oracle's hits are unordered and only the contract
    can be checked."""
    r = _range()
    n = 2 * r + 37
    cpu = make_postings(n, [5000, 300, 9, 0], seed=5, uniform=True)
    gpu = to_device(cpu, "cuda")
    c0, c1 = constants(cpu)
    q_terms = torch.tensor([[0, -1], [1, 0], [2, 1]], dtype=torch.int32)
    q_w = torch.tensor([[1.5, 0.0], [0.75, 1.5], [2.0, 0.75]])
    ref = dense_ref(cpu, q_terms, q_w, c0, c1)
    assert ref[0].unique().numel() == 2        # 0 and the one tied score
    allow = torch.rand(n, generator=torch.Generator().manual_seed(1)) < 0.5
    for mask in (None, allow.cuda()):
        s, i = bm25_search(gpu, q_terms.cuda(), q_w.cuda(), c0, c1, k,
                           allow=mask)
        check(2, ref.cuda(), mask, k, s, i)


@pytest.mark.gpu
def test_gpu_host_function_rejects_bad_arguments():
    nat = require_native()
    _, gpu, (c0, c1) = _big()
    q_terms, q_w, _, _, _ = _queries(3)
    good = dict(post_off=gpu.post_off, post_doc=gpu.post_doc,
                post_tf=gpu.post_tf, doc_len=gpu.doc_len, q_terms=q_terms,
                q_w=q_w, c0=c0, c1=c1, k_out=10, allow=None)
    nat.bm25_scan(**good)

    def bad(**kw):
        with pytest.raises(RuntimeError, match="bm25_scan"):
            nat.bm25_scan(**{**good, **kw})

    bad(k_out=0)
    bad(k_out=65)
    bad(post_off=gpu.post_off.to(torch.int32))
    bad(post_doc=gpu.post_doc.long())
    bad(post_tf=gpu.post_tf[:-1])
    bad(doc_len=gpu.doc_len.cpu())
    bad(q_terms=q_terms.long())
    bad(q_terms=q_terms.t())
    bad(q_w=q_w[:, :-1].contiguous())
    bad(q_w=q_w.double())
    bad(allow=torch.zeros(3, dtype=torch.int32, device="cuda"))
    # nothing to scan: the all-unfilled result, without a launch
    for kw in (dict(q_terms=q_terms[:, :0].contiguous(),
                    q_w=q_w[:, :0].contiguous()),
               dict(post_doc=gpu.post_doc[:0], post_tf=gpu.post_tf[:0]),
               dict(doc_len=gpu.doc_len[:0])):
        s, i = nat.bm25_scan(**{**good, **kw})
        assert s.shape == (3, 10) and (s == -1e30).all() and (i == -1).all()
