"""IVF search over quantized corpora: the route table (`ivf_route_kind`)
and, on the GPU, the fused `ivf_scan_i8` / `ivf_scan_fp8` kernels.

Contract under test (ops/ivf.py), as for the bf16 kernel: the output is
[Q, min(k, N)]; the first slots hold the top scores, descending, over
{rows of the probed lists} U tail, intersected with the allow mask; every
remaining slot is (score -inf, index -1). Scores are those of
`ivf_search_exact` on the same stored values: int8 rows times their
per-row scale against the int8-quantised query times its scale, e4m3 rows
against the e4m3 query.
"""

import numpy as np
import pytest
import torch

from nornicdb_amd.ops import (ivf_build_lists, ivf_route, ivf_search,
                              ivf_search_exact, pack_allow_mask)
from nornicdb_amd.ops import ivf as ivf_ops
from nornicdb_amd.ops.knn import quantize_fp8, quantize_int8
from nornicdb_amd.search.kmeans import kmeans

from ivf_cases import (N, NEG_INF, ROW_BASE, TAILS, check, clustered,
                       gpu_case, gpu_lists, case_probes, recall_at)


# ---------------------------------------------------------------------------
# CPU: the route table
# ---------------------------------------------------------------------------
_KIND = {torch.bfloat16: "scan", torch.int8: "scan_i8",
         torch.float8_e4m3fn: "scan_fp8"}


@pytest.mark.parametrize("k", [1, 64, 65])
@pytest.mark.parametrize("d", [96, 128, 384, 1024])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.int8,
                                   torch.float8_e4m3fn, torch.float32],
                         ids=["bf16", "int8", "fp8", "fp32"])
def test_route_kind_table(dtype, d, k):
    from nornicdb_amd.ops import ivf_route_kind
    want = "gather"
    if dtype in _KIND and d % 128 == 0 and k <= 64:
        want = _KIND[dtype]
    assert ivf_route_kind(dtype, d, k) == want
    assert ivf_ops.ivf_route_kind(dtype, d, k) == want


# ---------------------------------------------------------------------------
# GPU fixture: the one of tests/test_ivf.py, except that every row is a unit
# vector times a factor from {0.5, 1, 2}, so int8 row scales spread about
# 7x and query scales differ from query to query.
# ---------------------------------------------------------------------------
# Kernel and oracle are fp32 products of the same stored values; they differ
# in summation order only (the int32 dot is exact and converts to fp32
# exactly for D * 127^2 < 2^24): D * 2^-24 * |q||x| with |q||x| <= 4 and
# D <= 1024 is 2.4e-4 < 4e-4.
TOL = 4e-4

_cache = {}


def _base(d):
    """fp32 [N, D] on the GPU: unit rows times 0.5, 1 or 2."""
    key = ("base", d)
    if key not in _cache:
        g = torch.Generator(device="cuda").manual_seed(d)
        x = torch.nn.functional.normalize(
            torch.randn(N, d, device="cuda", generator=g), dim=-1)
        f = torch.tensor([0.5, 1.0, 2.0], device="cuda")[
            torch.randint(0, 3, (N,), device="cuda", generator=g)]
        _cache[key] = x * f[:, None]
    return _cache[key]


def _stored(fmt, d):
    """(db, scales or None, fp32 values of the stored rows [N, D])."""
    key = ("stored", fmt, d)
    if key not in _cache:
        if fmt == "int8":
            db, sa = quantize_int8(_base(d))
            _cache[key] = (db, sa, db.float() * sa[:, None])
        else:
            db = quantize_fp8(_base(d))
            _cache[key] = (db, None, db.float())
    return _cache[key]


def _query_values(fmt, q):
    if fmt == "int8":
        qi, sq = quantize_int8(q)
        return qi.float() * sq[:, None]
    return q.to(torch.float8_e4m3fn).float()


def _case(d, q_count, tail_start, masked):
    """(q fp32 [Q, D], allow bool [N] or None, ok bool [Q, N]): every query
    is a copy of its decoy row (ivf_cases.decoy_case)."""
    return gpu_case(("base", d), _base(d), q_count, tail_start, masked)


def _forbid_gather(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("the torch gather route was taken")
    monkeypatch.setattr(ivf_ops, "_ivf_gather", boom)


# ---------------------------------------------------------------------------
# GPU: the kernels through ivf_search
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("k", [1, 16, 17, 64])
@pytest.mark.parametrize("q_count", [1, 5, 17])
@pytest.mark.parametrize("d", [128, 384, 1024])
@pytest.mark.parametrize("fmt", ["int8", "fp8"])
def test_gpu_quant_scan_sweep(monkeypatch, fmt, d, q_count, k, masked):
    _forbid_gather(monkeypatch)
    db, scales, vals = _stored(fmt, d)
    probes = case_probes(q_count).cuda()
    for tail_start in TAILS:
        lists, _ = gpu_lists(tail_start)
        q, allow, ok = _case(d, q_count, tail_start, masked)
        ref = _query_values(fmt, q) @ vals.T
        for row_base in (0, ROW_BASE):
            s, i = ivf_search(db, q, k, lists, probes, tail_start,
                              row_base=row_base, allow=allow, scales=scales)
            check(ref, TOL, ok, k, row_base, s, i)
        # against the oracle itself, slot by slot
        es, ei = ivf_search_exact(db, q, k, lists, probes, tail_start,
                                  row_base=ROW_BASE, allow=allow,
                                  scales=scales)
        check(ref, 0.0, ok, k, ROW_BASE, es, ei)
        assert torch.equal(i == -1, ei == -1)
        fin = ei >= 0
        gap = (s - es)[fin].abs().max().item() if fin.any() else 0.0
        print(f"tail {tail_start}: max |kernel - oracle| by rank {gap:.3e}")
        assert gap <= TOL, gap
    if masked:   # packed form of the mask
        s2, i2 = ivf_search(db, q, k, lists, probes, tail_start,
                            row_base=ROW_BASE, allow=pack_allow_mask(allow),
                            scales=scales)
        assert torch.equal(s, s2) and torch.equal(i, i2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("fmt", ["int8", "fp8"])
def test_gpu_quant_takes_the_kernel_route(monkeypatch, fmt, k):
    _forbid_gather(monkeypatch)
    tail_start = N - 37
    db, scales, vals = _stored(fmt, 128)
    lists, _ = gpu_lists(tail_start)
    q, allow, ok = _case(128, 5, tail_start, True)
    s, i = ivf_search(db, q, k, lists, case_probes(5).cuda(), tail_start,
                      row_base=ROW_BASE, allow=allow, scales=scales)
    check(_query_values(fmt, q) @ vals.T, TOL, ok, k, ROW_BASE, s, i)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 64])
@pytest.mark.parametrize("fmt", ["int8", "fp8"])
def test_gpu_quant_all_skipped(monkeypatch, fmt, k):
    _forbid_gather(monkeypatch)
    db, scales, _ = _stored(fmt, 128)
    lists, _ = gpu_lists(N)
    q = _base(128)[:5].contiguous()
    probes = torch.full((5, 4), -1, dtype=torch.int32, device="cuda")
    s, i = ivf_search(db, q, k, lists, probes, N, row_base=ROW_BASE,
                      scales=scales)
    torch.cuda.synchronize()
    assert s.shape == (5, k)
    assert (i == -1).all() and (s == NEG_INF).all()
    # no probe columns at all, with and without a tail
    none = torch.empty(5, 0, dtype=torch.int32, device="cuda")
    s, i = ivf_search(db, q, k, lists, none, N, scales=scales)
    assert (i == -1).all() and (s == NEG_INF).all()
    lists37, _ = gpu_lists(N - 37)
    s, i = ivf_search(db, q, k, lists37, none, N - 37, scales=scales)
    torch.cuda.synchronize()
    kk = min(k, 37)
    for r in range(5):
        assert set(i[r, :kk].tolist()) <= set(range(N - 37, N))
        assert len(set(i[r, :kk].tolist())) == kk
    assert (i[:, 37:] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["int8", "fp8"])
def test_gpu_quant_repeated_probe_scanned_once(monkeypatch, fmt):
    _forbid_gather(monkeypatch)
    db, scales, _ = _stored(fmt, 128)
    lists, _ = gpu_lists(N)
    q = _base(128)[:3].contiguous()
    once = torch.tensor([[5, 2, -1, -1]] * 3, dtype=torch.int32).cuda()
    twice = torch.tensor([[5, 2, 5, 2]] * 3, dtype=torch.int32).cuda()
    s1, i1 = ivf_search(db, q, 40, lists, once, N, scales=scales)
    s2, i2 = ivf_search(db, q, 40, lists, twice, N, scales=scales)
    torch.cuda.synchronize()
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    assert (i1 >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 40])
def test_gpu_int8_is_deterministic(monkeypatch, k):
    """The 16-lane reduction is an integer sum: no order dependence."""
    _forbid_gather(monkeypatch)
    tail_start = N - 37
    db, scales, _ = _stored("int8", 1024)
    lists, _ = gpu_lists(tail_start)
    q, allow, _ = _case(1024, 17, tail_start, True)
    probes = case_probes(17).cuda()
    a = ivf_search(db, q, k, lists, probes, tail_start, allow=allow,
                   scales=scales)
    b = ivf_search(db, q, k, lists, probes, tail_start, allow=allow,
                   scales=scales)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["int8", "fp8"])
def test_gpu_quant_wrapper_rejects_bad_arguments(fmt):
    from nornicdb_amd.ops import require_native
    nat = require_native()
    st, scales, _ = _stored(fmt, 128)
    lists, cpu = gpu_lists(N)
    pr = case_probes(2).cuda()
    qf = _base(128)[:2].contiguous()
    tail = {"probes": pr, "list_off": lists.list_off,
            "list_rows": lists.list_rows, "tail_start": N,
            "max_len": lists.max_len, "row_base": 0, "k_out": 10,
            "allow": None}
    if fmt == "int8":
        qi, sq = quantize_int8(qf)
        good = {"db": st, "sa": scales, "q": qi, "sq": sq, **tail}
        fn = nat.ivf_scan_i8
    else:
        good = {"db": st.view(torch.uint8),
                "q": qf.to(torch.float8_e4m3fn).view(torch.uint8), **tail}
        fn = nat.ivf_scan_fp8
    s, i = fn(*good.values())
    assert s.shape == (2, 10)

    def bad(**kw):
        args = dict(good)
        args.update(kw)
        with pytest.raises(RuntimeError):
            fn(*args.values())

    bad(k_out=0)
    bad(k_out=65)
    bad(tail_start=-1)
    bad(tail_start=N + 1)
    bad(probes=pr[:1])                          # Q rows
    bad(probes=pr[0])                           # not 2-D
    bad(probes=pr.long())                       # dtype
    bad(probes=pr.cpu())                        # device
    bad(list_rows=cpu.list_rows)                # host tensor
    bad(list_off=lists.list_off.long())
    bad(q=qf)                                   # float query
    bad(q=good["q"][:, :96])                    # not contiguous
    bad(db=_base(128).to(torch.bfloat16))       # bf16 corpus
    bad(db=good["db"][:, :96])                  # not contiguous
    bad(allow=torch.zeros(3, dtype=torch.int32, device="cuda"))
    if fmt == "int8":
        bad(sa=scales[:-1].contiguous())        # wrong length
        bad(sq=sq[:1].contiguous())
        bad(sa=scales.double())
        bad(sq=sq.cpu())
        bad(db=st.view(torch.uint8))
    else:
        bad(db=st.view(torch.int8))


# ---------------------------------------------------------------------------
# GPU: index level
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("quant", ["int8", "fp8"])
def test_gpu_quant_index_level(monkeypatch, quant):
    from nornicdb_amd.search import EmbeddingIndex, IVFIndex
    _forbid_gather(monkeypatch)
    x, _ = clustered(1, 128, n=2000)
    mat = x.numpy()
    ids = [f"v{j}" for j in range(2000)]
    emb = EmbeddingIndex(128, device="cuda", quant=quant)
    emb.add_batch(ids, mat)
    ivf = IVFIndex(emb, nprobe=4)
    ivf.build(n_lists=16)
    assert ivf.built and ivf.n_lists == 16

    for j in (0, 7, 1999):                      # a stored row finds itself
        hits = ivf.search(mat[j], 10)
        assert hits[0][0] == f"v{j}" and len(hits) == 10
        assert len({h for h, _ in hits}) == 10
    batch = ivf.search_batch(mat[:5], 10)
    assert [b[0][0] for b in batch] == ids[:5]
    assert batch[0] == ivf.search(mat[0], 10)

    allowed = [f"v{j}" for j in range(0, 2000, 3)]
    got = ivf.search(mat[21], 10, allow_ids=allowed)
    assert len(got) == 10 and all(h in set(allowed) for h, _ in got)
    assert got[0][0] == "v21"
    for b in ivf.search_batch(mat[:4], 10, allow_ids=allowed):
        assert b and all(h in set(allowed) for h, _ in b)

    emb.remove("v7")                            # a removed id stays away
    hits = ivf.search(mat[7], 40)
    assert hits and all(h != "v7" for h, _ in hits)
    assert all(h != "v7" for b in ivf.search_batch(mat[5:9], 40)
               for h, _ in b)
    new = np.asarray(mat[7])                    # and the tail is scanned
    emb.add("fresh", new)
    assert ivf.tail == 1
    assert ivf.search(new, 3)[0][0] == "fresh"


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["int8", "fp8"])
def test_gpu_quant_recall_floor(monkeypatch, fmt):
    """IVF against the exact top-10 over the same quantised values."""
    _forbid_gather(monkeypatch)
    x, q = clustered(0, 128, device="cuda")
    c, assign = kmeans(x, 32, seed=0)
    lists = ivf_build_lists(assign, c.shape[0], x.shape[0], c)
    n = x.shape[0]
    if fmt == "int8":
        db, scales = quantize_int8(x)
    else:
        db, scales = quantize_fp8(x), None
    every = torch.arange(32, dtype=torch.int32, device="cuda").repeat(
        q.shape[0], 1)
    _, ref = ivf_search_exact(db, q, 10, lists, every, n, scales=scales)
    _, got = ivf_search(db, q, 10, lists, ivf_route(lists, q, 4), n,
                        scales=scales)
    r = recall_at(got, ref)
    print(f"{fmt} recall@10 at nprobe=4: {r:.4f}")
    assert r >= 0.95
