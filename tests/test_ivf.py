"""IVF search ops: inverted-list build, routing, the CPU/oracle path and, on
the GPU, the fused `ivf_scan` kernel and the torch gather fallback.

Contract under test (ops/ivf.py): the output is [Q, min(k, N)]; the first
slots hold the top scores, descending, over {rows of the probed lists} U
tail, intersected with the allow mask; every remaining slot is
(score -inf, index -1).
"""

import pytest
import torch

from nornicdb_amd.ops import (IVFLists, ivf_build_lists, ivf_route,
                              ivf_search, ivf_search_exact, knn_search_exact,
                              pack_allow_mask)
from nornicdb_amd.ops.ivf import _reachable
from nornicdb_amd.ops.knn import quantize_fp8, quantize_int8
from nornicdb_amd.search.kmeans import kmeans

from ivf_cases import (N, NEG_INF, ROW_BASE, TAILS, case_probes, check,
                       clustered, cpu_lists, gpu_case, gpu_lists, py_reach,
                       recall_at)


# ---------------------------------------------------------------------------
# CPU: ivf_build_lists
# ---------------------------------------------------------------------------
def test_build_lists_counting_sort():
    g = torch.Generator().manual_seed(0)
    n, c = 1000, 12
    assign = torch.randint(0, c, (n,), generator=g)
    assign[assign == 5] = 6                     # cluster 5 is empty
    lists = ivf_build_lists(assign, c, n, torch.zeros(c, 8))
    assert isinstance(lists, IVFLists) and lists.n_lists == c
    assert lists.list_off.dtype == torch.int32
    assert lists.list_rows.dtype == torch.int32
    assert lists.centroids.dtype == torch.float32
    off = lists.list_off.tolist()
    assert off[0] == 0 and off[-1] == n and len(off) == c + 1
    assert all(a <= b for a, b in zip(off, off[1:]))
    assert off[5] == off[6]                     # the empty cluster
    assert sorted(lists.list_rows.tolist()) == list(range(n))
    for cl in range(c):
        seg = lists.list_rows[off[cl]:off[cl + 1]]
        assert (assign[seg.long()] == cl).all()
        assert (seg[1:] > seg[:-1]).all()       # stable: slot order kept
    assert lists.max_len == max(b - a for a, b in zip(off, off[1:]))
    assert lists.n_built == n


def test_build_lists_unlisted_rows_and_bad_input():
    assign = torch.tensor([2, -1, 0, 2, -1, 1])
    lists = ivf_build_lists(assign, 3, 6, torch.zeros(3, 4))
    assert lists.list_off.tolist() == [0, 1, 2, 4]
    assert lists.list_rows.tolist() == [2, 5, 0, 3]
    assert lists.max_len == 2
    with pytest.raises(AssertionError):
        ivf_build_lists(torch.tensor([0, 3]), 3, 2, torch.zeros(3, 4))
    with pytest.raises(AssertionError):
        ivf_build_lists(torch.tensor([0, 1]), 3, 5, torch.zeros(3, 4))
    empty = ivf_build_lists(torch.full((4,), -1), 2, 4, torch.zeros(2, 4))
    assert empty.list_off.tolist() == [0, 0, 0] and empty.max_len == 0


def test_route_matches_squared_l2():
    torch.manual_seed(1)
    cent = torch.randn(20, 16)
    q = torch.randn(7, 16)
    lists = ivf_build_lists(torch.zeros(1, dtype=torch.long), 20, 1, cent)
    pr = ivf_route(lists, q, 5)
    assert pr.dtype == torch.int32 and pr.shape == (7, 5)
    d2 = ((q[:, None, :] - cent[None]) ** 2).sum(-1)
    assert torch.equal(pr.long(), torch.topk(-d2, 5).indices)
    assert ivf_route(lists, q, 99).shape == (7, 20)


# ---------------------------------------------------------------------------
# CPU: ivf_search
# ---------------------------------------------------------------------------
def _cpu_case(n=600, d=32, c=10, n_built=550, seed=0):
    g = torch.Generator().manual_seed(seed)
    db = torch.randn(n, d, generator=g)
    q = torch.randn(6, d, generator=g)
    assign = torch.randint(0, c, (n_built,), generator=g)
    lists = ivf_build_lists(assign, c, n_built, torch.zeros(c, d))
    return db, q, lists


def test_cpu_equals_exact_topk_over_masked_union():
    db, q, lists = _cpu_case()
    n, n_built = db.shape[0], lists.n_built
    g = torch.Generator().manual_seed(5)
    probes = torch.stack([torch.randperm(10, generator=g)[:3]
                          for _ in range(6)]).to(torch.int32)
    allow = torch.rand(n, generator=g) < 0.5
    reach = py_reach(lists, probes, n, n_built)
    for mask in (None, allow, pack_allow_mask(allow)):
        ok = reach if mask is None else reach & allow
        ref = (q @ db.T).masked_fill(~ok, NEG_INF)
        rs, ri = torch.topk(ref, 7, dim=-1)
        s, i = ivf_search(db, q, 7, lists, probes, n_built, allow=mask)
        assert torch.equal(i, ri) and torch.allclose(s, rs)
        s2, i2 = ivf_search_exact(db, q, 7, lists, probes, n_built,
                                  allow=mask)
        assert torch.equal(i, i2) and torch.equal(s, s2)
    # unprobed, non-tail rows are really excluded by this case
    assert not reach.all() and reach[:, n_built:].all()


def test_cpu_all_lists_equals_knn_search_exact():
    db, q, lists = _cpu_case(n_built=600)
    probes = torch.arange(10, dtype=torch.int32).repeat(6, 1)
    s, i = ivf_search(db, q, 9, lists, probes, 600, row_base=40)
    rs, ri = knn_search_exact(db, q, 9, row_base=40)
    assert torch.equal(i, ri) and torch.equal(s, rs)


def test_cpu_pads_and_row_base_and_skips():
    db, q, lists = _cpu_case()
    n, n_built = db.shape[0], lists.n_built
    off = lists.list_off.tolist()
    small = min(range(10), key=lambda c: off[c + 1] - off[c])
    m = off[small + 1] - off[small]
    members = set(lists.list_rows[off[small]:off[small + 1]].tolist())
    # one probed list, no tail, k larger than the list
    probes = torch.tensor([[small, -1, -1]] * 6, dtype=torch.int32)
    db_nt = db[:n_built]
    s, i = ivf_search(db_nt, q, m + 5, lists, probes, n_built, row_base=1000)
    assert s.shape == (6, m + 5) and i.dtype == torch.int64
    assert (i[:, m:] == -1).all() and (s[:, m:] == NEG_INF).all()
    for r in range(6):
        assert {x - 1000 for x in i[r, :m].tolist()} == members
    assert (s[:, :m - 1] >= s[:, 1:m]).all()
    # -1, out-of-range and repeated probes add nothing
    noisy = torch.tensor([[-1, small, 10, small, -7, 99]] * 6,
                         dtype=torch.int32)
    s2, i2 = ivf_search(db_nt, q, m + 5, lists, noisy, n_built, row_base=1000)
    assert torch.equal(i, i2) and torch.equal(s, s2)
    # only skips, no tail: all padding
    none = torch.full((6, 4), -1, dtype=torch.int32)
    s3, i3 = ivf_search(db_nt, q, 5, lists, none, n_built)
    assert (i3 == -1).all() and (s3 == NEG_INF).all()
    # only skips, with a tail: exactly the tail rows
    s4, i4 = ivf_search(db, q, n, lists, none, n_built, row_base=7)
    t = n - n_built
    for r in range(6):
        assert sorted(i4[r, :t].tolist()) == list(range(n_built + 7, n + 7))
    assert (i4[:, t:] == -1).all()


def test_cpu_int8_uses_row_scales():
    torch.manual_seed(3)
    db = torch.nn.functional.normalize(torch.randn(300, 64), dim=-1)
    q = db[:4].clone()
    db8, sa = quantize_int8(db)
    lists = ivf_build_lists(torch.arange(300) % 5, 5, 300, torch.zeros(5, 64))
    probes = torch.tensor([[0, 1]] * 4, dtype=torch.int32)
    qi, sq = quantize_int8(q)
    ref = (qi.float() * sq[:, None]) @ (db8.float() * sa[:, None]).T
    ok = py_reach(lists, probes, 300, 300)
    rs, ri = torch.topk(ref.masked_fill(~ok, NEG_INF), 6, dim=-1)
    s, i = ivf_search(db8, q, 6, lists, probes, 300, scales=sa)
    assert torch.equal(i, ri) and torch.allclose(s, rs)


# ---------------------------------------------------------------------------
# Recall floor on clustered data (a condition, not a measurement)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_cpu_recall_floor(seed):
    x, q = clustered(seed, 64)
    c, assign = kmeans(x, 32, seed=seed)
    lists = ivf_build_lists(assign, c.shape[0], x.shape[0], c)
    _, ref = knn_search_exact(x, q, 10)
    for nprobe in (4, 8):
        _, got = ivf_search(x, q, 10, lists, ivf_route(lists, q, nprobe),
                            x.shape[0])
        r = recall_at(got, ref)
        print(f"seed {seed} nprobe {nprobe}: recall@10 {r:.4f}")
        assert r >= 0.95


# ---------------------------------------------------------------------------
# GPU: ivf_scan kernel and the gather fallback
# ---------------------------------------------------------------------------
_cache = {}


def _corpus(d):
    """Unit-norm bf16 rows on the GPU, generated once per D."""
    key = ("db", d)
    if key not in _cache:
        g = torch.Generator(device="cuda").manual_seed(d)
        db = torch.randn(N, d, device="cuda", generator=g)
        _cache[key] = torch.nn.functional.normalize(db, dim=-1) \
            .to(torch.bfloat16)
    return _cache[key]


def _case(d, q_count, tail_start, masked):
    """(q bf16 [Q, D], allow bool [N] or None, ok bool [Q, N]): every query
    is a copy of its decoy row (ivf_cases.decoy_case)."""
    return gpu_case(("bf16", d), _corpus(d), q_count, tail_start, masked)


# atol of the gemv route's dot product on unit-norm rows
# (tests/test_ops_vector.py): same fdot2 code here
SCAN_TOL = 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("k", [1, 10, 16, 17, 40, 64])
@pytest.mark.parametrize("q_count", [1, 5, 17])
@pytest.mark.parametrize("d", [128, 384, 1024])
def test_gpu_scan_sweep(d, q_count, k, masked):
    db = _corpus(d)
    probes = case_probes(q_count).cuda()
    for tail_start in TAILS:
        lists, _ = gpu_lists(tail_start)
        q, allow, ok = _case(d, q_count, tail_start, masked)
        for row_base in (0, ROW_BASE):
            s, i = ivf_search(db, q, k, lists, probes, tail_start,
                              row_base=row_base, allow=allow)
            check(q.float() @ db.float().T, SCAN_TOL, ok, k, row_base, s, i)
    # the oracle meets the same contract bit for bit on the same inputs
    es, ei = ivf_search_exact(db, q, k, lists, probes, tail_start,
                              row_base=ROW_BASE, allow=allow)
    check(q.float() @ db.float().T, 0.0, ok, k, ROW_BASE, es, ei)
    if masked:   # packed form of the mask
        s2, i2 = ivf_search(db, q, k, lists, probes, tail_start,
                            row_base=ROW_BASE, allow=pack_allow_mask(allow))
        assert torch.equal(s, s2) and torch.equal(i, i2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 64])
def test_gpu_scan_all_skipped(k):
    db = _corpus(128)
    lists, _ = gpu_lists(N)
    q = db[:5].contiguous()
    probes = torch.full((5, 4), -1, dtype=torch.int32, device="cuda")
    s, i = ivf_search(db, q, k, lists, probes, N, row_base=ROW_BASE)
    torch.cuda.synchronize()
    assert s.shape == (5, k)
    assert (i == -1).all() and (s == NEG_INF).all()
    # no probe columns at all, with and without a tail
    none = torch.empty(5, 0, dtype=torch.int32, device="cuda")
    s, i = ivf_search(db, q, k, lists, none, N)
    assert (i == -1).all() and (s == NEG_INF).all()
    lists37, _ = gpu_lists(N - 37)
    s, i = ivf_search(db, q, k, lists37, none, N - 37)
    torch.cuda.synchronize()
    kk = min(k, 37)
    for r in range(5):
        assert set(i[r, :kk].tolist()) <= set(range(N - 37, N))
        assert len(set(i[r, :kk].tolist())) == kk
    assert (i[:, 37:] == -1).all()


@pytest.mark.gpu
def test_gpu_scan_repeated_probe_scanned_once():
    db = _corpus(128)
    lists, _ = gpu_lists(N)
    q = db[:3].contiguous()
    once = torch.tensor([[5, 2, -1, -1]] * 3, dtype=torch.int32).cuda()
    twice = torch.tensor([[5, 2, 5, 2]] * 3, dtype=torch.int32).cuda()
    s1, i1 = ivf_search(db, q, 40, lists, once, N)
    s2, i2 = ivf_search(db, q, 40, lists, twice, N)
    torch.cuda.synchronize()
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    assert (i1 >= 0).all()


# ---------------------------------------------------------------------------
# The bf16 and the fp8 scan against an exact reference, bit for bit. One
# kernel text serves both element sizes; this is the guard on its address
# arithmetic.
#
# Corpus and queries are k / 8 with k in -2..2: exact in bf16 and in e4m3.
# Every product is a multiple of 1/64 of magnitude <= 4/64, so any partial
# sum of up to 384 of them is an integer below 2^11 in units of 1/64: exact
# in fp32 in whatever order it is taken. The fp32 matmul on the CPU is
# therefore THE score, and both kernels must return it. int8 is left out:
# 0.125 / (0.25 / 127) = 63.5 does not survive the rounding.
# ---------------------------------------------------------------------------
EXACT_DIMS = [128, 384]
EXACT_Q, EXACT_K, EXACT_TAIL = 5, 10, N - 37


def _exact_case(d, masked):
    """CPU: (db fp32 [N, d], q fp32 [5, d], allow bool [N] or None, ref fp32
    [5, N]): the exact scores, -inf outside the rows that
    ivf_search_exact's reachability and the mask let a query return."""
    key = ("exact", d, masked)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 + d)
        db = torch.randint(-2, 3, (N, d), generator=g).float() / 8
        q = torch.randint(-2, 3, (EXACT_Q, d), generator=g).float() / 8
        allow = (torch.rand(N, generator=g) < 0.5) if masked else None
        ok = _reachable(cpu_lists(EXACT_TAIL), case_probes(EXACT_Q), N,
                        EXACT_TAIL)
        if masked:
            ok = ok & allow[None, :]
        _cache[key] = (db, q, allow, (q @ db.T).masked_fill(~ok, NEG_INF))
    return _cache[key]


@pytest.mark.parametrize("d", EXACT_DIMS)
def test_exact_reference(d):
    """Conditions on the reference alone."""
    db, q, _, ref = _exact_case(d, False)
    for t in (db, q):       # the values survive both storage formats
        assert torch.equal(t.to(torch.bfloat16).float(), t)
        assert torch.equal(t.to(torch.float8_e4m3fn).float(), t)
    fin = ref > NEG_INF
    assert torch.equal(ref[fin].double(), (q.double() @ db.double().T)[fin])
    # reachability agrees with the plain-Python one of the other tests
    assert torch.equal(fin, py_reach(cpu_lists(EXACT_TAIL),
                                     case_probes(EXACT_Q), N, EXACT_TAIL))
    # unmasked, every query fills all k slots
    assert (torch.topk(ref, EXACT_K, dim=-1).values > NEG_INF).all()
    _, _, allow, mref = _exact_case(d, True)
    assert ((mref > NEG_INF) == (fin & allow[None, :])).all()


def _check_exact(s, i, ref, row_base):
    """(s, i) against the exact scores ref [Q, n] (-inf where a row is
    unreachable or disallowed). Scores tie often: nothing is asserted about
    which of several tied rows comes back."""
    k = s.shape[1]
    s_ref = torch.topk(ref, k, dim=-1).values
    assert s.shape == s_ref.shape and i.shape == s_ref.shape
    assert s.dtype == torch.float32 and i.dtype == torch.int64
    assert torch.equal(s, s_ref), (s != s_ref).nonzero()[:8]
    filled = s_ref > NEG_INF
    assert ((i >= 0) == filled).all()
    assert (i[~filled] == -1).all()
    loc = (i - row_base).clamp_min(0)
    assert ((i - row_base >= 0) | ~filled).all() and (loc < ref.shape[1]).all()
    # reachable, allowed, and scored exactly what was returned
    assert (torch.gather(ref, 1, loc) == s)[filled].all()
    assert (torch.gather(ref, 1, loc) > NEG_INF)[filled].all()
    srt = torch.sort(torch.where(filled, i, -1 - torch.arange(
        k, device=i.device).expand_as(i)), dim=-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "duplicate hit"


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("d", EXACT_DIMS)
def test_gpu_scan_exact_across_formats(monkeypatch, d, masked):
    from nornicdb_amd.ops import ivf as ivf_ops

    def boom(*a, **kw):
        raise AssertionError("the torch gather route was taken")
    monkeypatch.setattr(ivf_ops, "_ivf_gather", boom)
    db, q, allow, ref = (None if t is None else t.cuda()
                         for t in _exact_case(d, masked))
    lists, _ = gpu_lists(EXACT_TAIL)
    probes = case_probes(EXACT_Q).cuda()
    got = {}
    for fmt, stored in (("bf16", db.to(torch.bfloat16)),
                        ("fp8", quantize_fp8(db))):
        s, i = ivf_search(stored, q, EXACT_K, lists, probes, EXACT_TAIL,
                          row_base=ROW_BASE, allow=allow)
        torch.cuda.synchronize()
        _check_exact(s, i, ref, ROW_BASE)
        got[fmt] = s
    assert torch.equal(got["bf16"], got["fp8"])


# Both sides are fp32 products of the same stored values; they differ only
# in summation order: D * 2^-24 * |q||x| <= 1024 * 6e-8 < 1e-4.
FALLBACK_TOL = 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16-k100", "fp8", "int8", "bf16-d96"])
def test_gpu_fallback_contract(kind):
    """k > 64, quantized corpora and D % 128 != 0 take the gather path."""
    tail_start = N - 37
    d = 96 if kind == "bf16-d96" else 128
    k = 100 if kind == "bf16-k100" else 10
    lists, _ = gpu_lists(tail_start)
    probes = case_probes(5).cuda()
    if d == 128:
        q, allow, ok = _case(128, 5, tail_start, True)
        base = _corpus(128)
    else:
        g = torch.Generator(device="cuda").manual_seed(96)
        base = torch.nn.functional.normalize(
            torch.randn(N, 96, device="cuda", generator=g), dim=-1) \
            .to(torch.bfloat16)
        q = base[:5].contiguous()
        _, allow, ok = _case(128, 5, tail_start, True)
    scales = None
    if kind == "fp8":
        st = quantize_fp8(base.float())
        qv = q.to(torch.float8_e4m3fn).float()
        vals = st.float()
    elif kind == "int8":
        st, scales = quantize_int8(base.float())
        qi, sq = quantize_int8(q)
        qv = qi.float() * sq[:, None]
        vals = st.float() * scales[:, None]
    else:
        st, qv, vals = base, q.float(), base.float()
    s, i = ivf_search(st, q, k, lists, probes, tail_start, row_base=ROW_BASE,
                      allow=allow, scales=scales)
    check(qv @ vals.T, FALLBACK_TOL, ok, k, ROW_BASE, s, i)


@pytest.mark.gpu
def test_gpu_wrapper_rejects_bad_arguments():
    from nornicdb_amd.ops import require_native
    nat = require_native()
    db = _corpus(128)
    lists, cpu = gpu_lists(N)
    q = db[:2].contiguous()
    pr = case_probes(2).cuda()
    good = (db, q, pr, lists.list_off, lists.list_rows, N, lists.max_len, 0,
            10, None)
    s, i = nat.ivf_scan(*good)
    assert s.shape == (2, 10)

    def bad(**kw):
        names = ["db", "q", "probes", "list_off", "list_rows", "tail_start",
                 "max_len", "row_base", "k_out", "allow"]
        args = dict(zip(names, good))
        args.update(kw)
        with pytest.raises(RuntimeError):
            nat.ivf_scan(*[args[n] for n in names])

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
    bad(q=q.float())
    bad(db=db[:, :96])                          # not contiguous
    bad(allow=torch.zeros(3, dtype=torch.int32, device="cuda"))


@pytest.mark.gpu
def test_gpu_recall_floor_kernel_path():
    """Same clustered generator at D=128, scored by the kernel."""
    x, q = clustered(0, 128, device="cuda")
    c, assign = kmeans(x, 32, seed=0)
    lists = ivf_build_lists(assign, c.shape[0], x.shape[0], c)
    xb, qb = x.to(torch.bfloat16), q.to(torch.bfloat16)
    _, ref = knn_search_exact(xb, qb, 10)
    _, got = ivf_search(xb, qb, 10, lists, ivf_route(lists, q, 4),
                        x.shape[0])
    r = recall_at(got, ref)
    print(f"recall@10 at nprobe=4: {r:.4f}")
    assert r >= 0.95
