"""Filtered kNN: packed allow-mask format, CPU contract and, on GPU, every
kernel route (gemv, MFMA bf16, fp8, int8) with the mask fused in.

The contract under test (ops/knn.py): with m allowed rows the output is
[Q, min(k, N)]; the first min(k, m) slots are the allowed top scores in
descending order and every remaining slot is (score -inf, index -1).
"""

import pytest
import torch

from nornicdb_amd.ops import knn_search
from nornicdb_amd.ops.knn import (knn_search_int8, pack_allow_mask,
                                  quantize_fp8, quantize_int8,
                                  unpack_allow_mask)

NEG_INF = float("-inf")


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 96, 12345])
def test_pack_unpack_roundtrip(n):
    g = torch.Generator().manual_seed(n)
    allow = torch.rand(n, generator=g) < 0.5
    words = pack_allow_mask(allow)
    assert words.dtype == torch.int32 and words.shape == ((n + 31) // 32,)
    assert torch.equal(unpack_allow_mask(words, n), allow)
    ones = torch.ones(n, dtype=torch.bool)
    assert torch.equal(unpack_allow_mask(pack_allow_mask(ones), n), ones)


def test_pack_bit_order():
    allow = torch.zeros(64, dtype=torch.bool)
    allow[[0, 31, 32, 63]] = True
    assert pack_allow_mask(allow).tolist() == [-2147483647, -2147483647]


def _masked_ref(scores, allow, k):
    return torch.topk(scores.masked_fill(~allow, NEG_INF), k, dim=-1)


def test_cpu_filtered_equals_masked_topk():
    torch.manual_seed(0)
    db = torch.randn(500, 64)
    q = torch.randn(7, 64)
    allow = torch.rand(500) < 0.3
    rs, ri = _masked_ref(q @ db.T, allow, 5)
    for mask in (allow, pack_allow_mask(allow)):
        s, i = knn_search(db, q, 5, allow=mask)
        assert torch.equal(i, ri)
        assert torch.allclose(s, rs)


def test_cpu_fewer_allowed_than_k_pads():
    torch.manual_seed(1)
    db = torch.randn(100, 32)
    q = torch.randn(4, 32)
    allow = torch.zeros(100, dtype=torch.bool)
    allow[[3, 50, 99]] = True
    s, i = knn_search(db, q, 8, allow=allow)
    assert s.shape == (4, 8) and i.shape == (4, 8)
    for r in range(4):
        assert sorted(i[r, :3].tolist()) == [3, 50, 99]
    assert (i[:, 3:] == -1).all()
    assert (s[:, 3:] == NEG_INF).all()
    assert (s[:, :2] >= s[:, 1:3]).all()
    # nothing allowed at all
    s, i = knn_search(db, q, 8, allow=torch.zeros(100, dtype=torch.bool))
    assert (i == -1).all() and (s == NEG_INF).all()


def test_cpu_row_base_shifts_hits_not_padding():
    torch.manual_seed(2)
    db = torch.randn(64, 16)
    q = torch.randn(3, 16)
    allow = torch.zeros(64, dtype=torch.bool)
    allow[[5, 6]] = True
    s, i = knn_search(db, q, 4, row_base=1000, allow=allow)
    for r in range(3):
        assert sorted(i[r, :2].tolist()) == [1005, 1006]
    assert (i[:, 2:] == -1).all()
    assert (s[:, 2:] == NEG_INF).all()


def test_cpu_int8_filtered():
    torch.manual_seed(3)
    db = torch.nn.functional.normalize(torch.randn(300, 64), dim=-1)
    q = db[:5].clone()
    db8, sa = quantize_int8(db)
    allow = torch.rand(300) < 0.5
    allow[:5] = False
    qi, sq = quantize_int8(q)
    ref = (qi.float() * sq[:, None]) @ (db8.float() * sa[:, None]).T
    rs, ri = _masked_ref(ref, allow, 6)
    s, i = knn_search_int8(db8, sa, q, 6, row_base=10, allow=allow)
    assert torch.equal(i, ri + 10)
    assert torch.allclose(s, rs)


# ---------------------------------------------------------------------------
# GPU: five routes through the dispatch in ops/knn.py
# ---------------------------------------------------------------------------
D = 128
ROW_BASE = 1000


class _Route:
    """One kernel route. tol is the atol of that kernel's unfiltered test in
    tests/test_ops_vector.py (gemv 1e-2, MFMA bf16 2e-2, fp8 1e-3 and int8
    1e-4 against an fp32 product of the same stored values)."""

    def __init__(self, name, kind, q_count, k, tol):
        self.name, self.kind, self.q_count, self.k, self.tol = \
            name, kind, q_count, k, tol

    def __repr__(self):
        return self.name

    def store(self, db):
        if self.kind == "bf16":
            return db.to(torch.bfloat16)
        if self.kind == "fp8":
            return quantize_fp8(db)
        return quantize_int8(db)

    def search(self, st, q, k, row_base, allow):
        if self.kind == "bf16":
            return knn_search(st, q.to(torch.bfloat16), k, row_base,
                              allow=allow)
        if self.kind == "fp8":
            return knn_search(st, q, k, row_base, allow=allow)
        return knn_search_int8(st[0], st[1], q, k, row_base, allow=allow)

    def exact_scores(self, st, q):
        """fp32 scores of the stored (quantized) values, [Q, N]."""
        if self.kind == "bf16":
            return q.to(torch.bfloat16).float() @ st.float().T
        if self.kind == "fp8":
            return q.to(torch.float8_e4m3fn).float() @ st.float().T
        qi, sq = quantize_int8(q)
        return (qi.float() * sq[:, None]) @ (st[0].float() * st[1][:, None]).T


ROUTES = [
    _Route("gemv-q3-k10", "bf16", 3, 10, 1e-2),
    _Route("gemv-q16-k16", "bf16", 16, 16, 1e-2),
    _Route("mfma-bf16-q40-k10", "bf16", 40, 10, 2e-2),
    _Route("fp8-q40-k10", "fp8", 40, 10, 1e-3),
    _Route("int8-q40-k10", "int8", 40, 10, 1e-4),
]

_corpus_cache = {}


def _corpus(n):
    """Unit-norm fp32 rows on the GPU, generated once per size."""
    if n not in _corpus_cache:
        g = torch.Generator(device="cuda").manual_seed(n)
        db = torch.randn(n, D, device="cuda", generator=g)
        _corpus_cache[n] = torch.nn.functional.normalize(db, dim=-1)
    return _corpus_cache[n]


_store_cache = {}


def _stored(route, n):
    key = (route.kind, n)
    if key not in _store_cache:
        _store_cache[key] = route.store(_corpus(n))
    return _store_cache[key]


def _decoy_case(n, q_count, density, seed, zero_rows=None):
    """Queries that copy disallowed rows: (q [Q, D], allow bool [N]). Row 0
    and the last row (tail of the MFMA routes) are always among them."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n - 2, generator=g)[:q_count - 2] + 1
    rows = torch.cat([torch.tensor([0, n - 1]), perm])[:q_count]
    allow = torch.rand(n, generator=g) < density
    allow[rows] = False
    if zero_rows is not None:
        allow[zero_rows[0]:zero_rows[1]] = False
    return _corpus(n)[rows.cuda()].clone(), allow.cuda()


def _check_filtered(route, st, q, allow, k, s, i):
    """The decoy assertions: nothing disallowed, rank-by-rank scores, each
    id's own score, padding."""
    torch.cuda.synchronize()
    n = allow.shape[0]
    m = int(allow.sum())
    kk = min(k, m)
    assert s.shape == (q.shape[0], min(k, n)) and i.shape == s.shape
    assert i.dtype == torch.int64 and s.dtype == torch.float32
    assert (i[:, kk:] == -1).all(), i
    assert (s[:, kk:] == NEG_INF).all(), s
    if kk == 0:
        return
    loc = i[:, :kk] - ROW_BASE
    assert ((loc >= 0) & (loc < n)).all(), i
    assert allow[loc].all(), "a disallowed row was returned"
    srt = loc.sort(dim=-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "duplicate hit"
    ref = route.exact_scores(st, q)
    rs, _ = torch.topk(ref.masked_fill(~allow, NEG_INF), kk, dim=-1)
    got = s[:, :kk]
    err = (got - rs).abs().max().item()
    own = (torch.gather(ref, 1, loc) - got).abs().max().item()
    print(f"{route.name}: n={n} m={m} rank err {err:.3e} own err {own:.3e}")
    assert err <= route.tol, err
    assert own <= route.tol, own
    assert (got[:, :-1] >= got[:, 1:]).all()


BIT_ROWS = [0, 31, 32, 95, 96, 191, 192, 228]


@pytest.mark.gpu
@pytest.mark.parametrize("stray", [False, True], ids=["clean", "stray-bits"])
@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_gpu_bit_positions(route, stray):
    """N=229 = two 96-row panels + a 37-row tail; the allowed rows sit on
    every word and panel edge. Exact and independent of numerics. Each
    route runs at its own k (a bf16 Q=16 call with k=10 would leave the
    gemv route), so the 8 hits are followed by k-8 padding slots."""
    n = 229
    st = _stored(route, n)
    allow = torch.zeros(n, dtype=torch.bool)
    allow[BIT_ROWS] = True
    words = pack_allow_mask(allow)
    if stray:
        # bits 229..255 of the last word: rows that do not exist
        words[-1] |= torch.tensor(-1 << (n & 31), dtype=torch.int32)
    q = _corpus(n)[:route.q_count]
    s, i = route.search(st, q, route.k, ROW_BASE, words.cuda())
    torch.cuda.synchronize()
    assert i.shape == (route.q_count, route.k)
    want = [r + ROW_BASE for r in BIT_ROWS]
    for r in range(route.q_count):
        assert sorted(i[r, :8].tolist()) == want, (r, i[r])
    assert (i[:, 8:] == -1).all()
    assert (s[:, 8:] == NEG_INF).all()
    assert torch.isfinite(s[:, :8]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("density", [0.5, 0.01], ids=["half", "sparse"])
@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_gpu_decoys(route, density):
    """Every query is a copy of a disallowed row, so an unfiltered search
    would put that row first with score ~1."""
    n = 12345
    st = _stored(route, n)
    q, allow = _decoy_case(n, route.q_count, density, seed=7)
    # bool form (packed on entry) and packed form must agree
    s, i = route.search(st, q, route.k, ROW_BASE, allow)
    _check_filtered(route, st, q, allow, route.k, s, i)
    s2, i2 = route.search(st, q, route.k, ROW_BASE, pack_allow_mask(allow))
    assert torch.equal(i, i2) and torch.equal(s, s2)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_gpu_empty_mask(route):
    n = 12345
    st = _stored(route, n)
    q = _corpus(n)[:route.q_count]
    allow = torch.zeros(n, dtype=torch.bool, device="cuda")
    s, i = route.search(st, q, route.k, ROW_BASE, allow)
    _check_filtered(route, st, q, allow, route.k, s, i)
    assert (i == -1).all() and (s == NEG_INF).all()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_gpu_stride_loops(route, monkeypatch):
    """Two MFMA workgroups over 7 panels + 5 tail rows and one gemv block,
    so every block walks its stride loop; panel 3 is masked out entirely so
    the panel-skip branch runs between two scored panels."""
    monkeypatch.setenv("NORNICDB_KNN_GRID", "2")
    monkeypatch.setenv("NORNICDB_GEMV_BLOCKS", "1")
    n = 96 * 7 + 5
    st = _stored(route, n)
    q, allow = _decoy_case(n, route.q_count, 0.5, seed=11,
                           zero_rows=(96 * 3, 96 * 4))
    assert not allow[96 * 3:96 * 4].any() and allow[96 * 4:].any()
    s, i = route.search(st, q, route.k, ROW_BASE, allow)
    _check_filtered(route, st, q, allow, route.k, s, i)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES, ids=repr)
def test_gpu_allow_none_unchanged(route):
    """allow=None is the call that existed before the mask argument."""
    n = 12345
    st = _stored(route, n)
    q = _corpus(n)[5:5 + route.q_count]
    s, i = route.search(st, q, route.k, ROW_BASE, None)
    if route.kind == "int8":
        s0, i0 = knn_search_int8(st[0], st[1], q, route.k, ROW_BASE)
    elif route.kind == "fp8":
        s0, i0 = knn_search(st, q, route.k, ROW_BASE)
    else:
        s0, i0 = knn_search(st, q.to(torch.bfloat16), route.k, ROW_BASE)
    torch.cuda.synchronize()
    assert torch.equal(s, s0) and torch.equal(i, i0)
    assert (i >= ROW_BASE).all() and torch.isfinite(s).all()
    # an all-ones mask returns the same hits as no mask
    ones = torch.ones(n, dtype=torch.bool, device="cuda")
    s1, i1 = route.search(st, q, route.k, ROW_BASE, ones)
    assert torch.equal(s1, s0) and torch.equal(i1, i0)


@pytest.mark.gpu
def test_gpu_wrapper_rejects_bad_mask():
    from nornicdb_amd.ops import require_native
    nat = require_native()
    db = _corpus(229).to(torch.bfloat16)
    q = db[:2].contiguous()
    with pytest.raises(RuntimeError):      # too few words for 229 rows
        nat.knn_gemv(db, q, 0, 5, torch.zeros(7, dtype=torch.int32,
                                              device="cuda"))
    with pytest.raises(RuntimeError):      # wrong dtype
        nat.knn_gemv(db, q, 0, 5, torch.zeros(8, dtype=torch.int64,
                                              device="cuda"))
    with pytest.raises(RuntimeError):      # host tensor
        nat.knn_gemv(db, q, 0, 5, torch.zeros(8, dtype=torch.int32))
