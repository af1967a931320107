"""The shared top-k core (csrc/topk.h, csrc/topk_merge.hip) through every
route that uses it: gemv, bf16 MFMA, fp8 / int8 MFMA and the three IVF scans.

Two things are pinned that no other test isolates:

* the merge's one semantic line, `id < 0 ? -1 : row_base + id`: with fewer
  allowed rows than k and a non-zero row_base every unfilled slot must come
  back as (-inf, -1), never as row_base - 1;
* blocks that walk several panels with one running list per thread, merged
  from exactly two blocks (NORNICDB_KNN_GRID=2), at the smallest shapes: one
  and two K tiles of the quantised kernel, k = 1 and the full list.
"""

import pytest
import torch

from nornicdb_amd.ops import IVFLists, ivf_search
from nornicdb_amd.ops import ivf as ivf_ops
from nornicdb_amd.ops.knn import (_knn_bm, _knn_q8_bm, knn_search,
                                  knn_search_exact, knn_search_int8,
                                  quantize_fp8, quantize_int8)

NEG_INF = float("-inf")
ROW_BASE = 1000
# score tolerances of the same routes in tests/test_ops_vector.py
TOL = {"gemv": 1e-2, "mfma": 2e-2, "fp8": 1e-3, "int8": 1e-4}
# IVF scans against the fp32 product of the same stored values, bound of
# tests/test_ivf_quant.py: the elementwise products are exact in fp32 (int8,
# e4m3 and bf16 alike), so kernel and oracle differ in summation order only,
# D * 2^-24 * |q||x| <= 256 * 6e-8 = 1.5e-5 here
TOL_IVF = 4e-4

_cache = {}


def _rows(route):
    """Five quantised panels + 7 tail rows, or three bf16 panels + 7."""
    return (_knn_q8_bm() * 5 if route in ("fp8", "int8")
            else _knn_bm() * 3) + 7


def _unit(n, d, seed):
    key = (n, d, seed)
    if key not in _cache:
        g = torch.Generator(device="cuda").manual_seed(seed)
        _cache[key] = torch.nn.functional.normalize(
            torch.randn(n, d, device="cuda", generator=g), dim=-1)
    return _cache[key]


def _search(route, x, q, k, allow):
    """(scores, ids, fp32 values of the stored rows, of the scored query)."""
    if route == "int8":
        db, sa = quantize_int8(x)
        qi, sq = quantize_int8(q)
        s, i = knn_search_int8(db, sa, q, k, row_base=ROW_BASE, allow=allow)
        return s, i, db.float() * sa[:, None], qi.float() * sq[:, None]
    if route == "fp8":
        db = quantize_fp8(x)
        s, i = knn_search(db, q, k, row_base=ROW_BASE, allow=allow)
        return s, i, db.float(), q.to(torch.float8_e4m3fn).float()
    db = x.to(torch.bfloat16)
    qb = q.to(torch.bfloat16)
    s, i = knn_search(db, qb, k, row_base=ROW_BASE, allow=allow)
    return s, i, db.float(), qb.float()


def _check(s, i, vals, qv, k, allow, tol):
    """Against knn_search_exact on the values the route scored: scores by
    rank, each returned row's own score, and the unfilled slots."""
    torch.cuda.synchronize()
    es, ei = knn_search_exact(vals, qv, k, row_base=ROW_BASE, allow=allow)
    assert s.shape == es.shape and i.shape == ei.shape
    assert i.dtype == torch.int64 and s.dtype == torch.float32
    filled = ei >= 0
    assert torch.equal(i >= 0, filled), i
    assert (i[~filled] == -1).all() and (s[~filled] == NEG_INF).all(), (s, i)
    assert (i != ROW_BASE - 1).all()
    loc = torch.where(filled, i - ROW_BASE, 0)
    assert ((loc >= 0) & (loc < vals.shape[0])).all(), i
    if allow is not None:
        assert (allow[loc] | ~filled).all(), "a disallowed row was returned"
    if filled.any():
        err = (s - es)[filled].abs().max().item()
        own = (torch.gather(qv @ vals.T, 1, loc) - s)[filled].abs().max().item()
        print(f"rank err {err:.3e} own err {own:.3e}")
        assert err <= tol, err
        assert own <= tol, own
    assert (s[:, :-1] >= s[:, 1:]).all()


ROUTES = [("gemv", 2), ("mfma", 17), ("fp8", 17), ("int8", 17)]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 3), (1, 0)])
@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("route,q_count", ROUTES)
def test_unfilled_slots_knn(route, q_count, d, k, m):
    """m < k allowed rows: one early, the last row a kernel panel holds and a
    tail row; the other k - m slots are (-inf, -1)."""
    n = _rows(route)
    x = _unit(n, d, 1)
    q = _unit(q_count, d, 2)
    allow = torch.zeros(n, dtype=torch.bool, device="cuda")
    for r in [5, n - 8, n - 1][:m]:
        allow[r] = True
    s, i, vals, qv = _search(route, x, q, k, allow)
    _check(s, i, vals, qv, k, allow, TOL[route])
    assert (i >= 0).sum(-1).eq(m).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 17])
@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("fmt", ["bf16", "int8", "fp8"])
def test_unfilled_slots_ivf(monkeypatch, fmt, d, k):
    """Q = 1, two of four lists probed, three reachable allowed rows (two in
    a probed list, one in the tail) and one allowed row out of reach. k = 16
    takes the K=16 scan and merge, k = 17 the K=64 ones."""
    def boom(*a, **kw):
        raise AssertionError("the torch gather route was taken")
    monkeypatch.setattr(ivf_ops, "_ivf_gather", boom)
    n = 487
    tail_start = n - 7
    x = _unit(n, d, 3)
    q = _unit(1, d, 4)
    off = torch.tensor([0, 120, 240, 360, 480], dtype=torch.int32)
    rows = torch.randperm(tail_start,
                          generator=torch.Generator().manual_seed(5))
    lists = IVFLists(torch.zeros(4, 8, device="cuda"), off.cuda(),
                     rows.to(torch.int32).cuda(), tail_start, 120)
    probes = torch.tensor([[2, 0]], dtype=torch.int32, device="cuda")
    reach = [int(rows[3]), int(rows[300]), n - 2]     # lists 0, 2 and tail
    allow = torch.zeros(n, dtype=torch.bool, device="cuda")
    allow[reach + [int(rows[130])]] = True             # list 1: not probed
    scales = None
    if fmt == "int8":
        db, scales = quantize_int8(x)
        vals = db.float() * scales[:, None]
        qi, sq = quantize_int8(q)
        qv = qi.float() * sq[:, None]
    elif fmt == "fp8":
        db = quantize_fp8(x)
        vals, qv = db.float(), q.to(torch.float8_e4m3fn).float()
    else:
        db = x.to(torch.bfloat16)
        vals, qv = db.float(), q.to(torch.bfloat16).float()
    s, i = ivf_search(db, q, k, lists, probes, tail_start, row_base=ROW_BASE,
                      allow=allow, scales=scales)
    ok = torch.zeros(n, dtype=torch.bool, device="cuda")
    ok[reach] = True
    _check(s, i, vals, qv, k, ok, TOL_IVF)
    assert sorted(i[0, :3].tolist()) == sorted(r + ROW_BASE for r in reach)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("route", ["mfma", "fp8", "int8"])
def test_multi_panel_walk(monkeypatch, route, d, k, masked):
    """Two blocks share the panels (quantised: five, so three and two; bf16:
    three, so two and one) and the merge sees exactly their lists; the 7
    rows behind the last panel are the torch-scored tail."""
    monkeypatch.setenv("NORNICDB_KNN_GRID", "2")
    n = _rows(route)
    x = _unit(n, d, 6)
    q = _unit(17, d, 7)
    allow = None
    if masked:
        g = torch.Generator(device="cuda").manual_seed(8)
        allow = torch.rand(n, device="cuda", generator=g) < 0.5
    s, i, vals, qv = _search(route, x, q, k, allow)
    _check(s, i, vals, qv, k, allow, TOL[route])
    assert (i >= 0).all()
