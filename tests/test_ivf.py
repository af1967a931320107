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
from nornicdb_amd.ops.knn import quantize_fp8, quantize_int8
from nornicdb_amd.search.kmeans import kmeans

NEG_INF = float("-inf")


def _py_reach(lists, probes, n, tail_start):
    """bool [Q, n] from plain Python slices of the CSR arrays."""
    off = lists.list_off.tolist()
    rows = lists.list_rows.tolist()
    reach = torch.zeros(probes.shape[0], n, dtype=torch.bool)
    for qi, pr in enumerate(probes.tolist()):
        for c in pr:
            if 0 <= c < len(off) - 1:
                reach[qi, rows[off[c]:off[c + 1]]] = True
        reach[qi, tail_start:] = True
    return reach


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
    reach = _py_reach(lists, probes, n, n_built)
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
    ok = _py_reach(lists, probes, 300, 300)
    rs, ri = torch.topk(ref.masked_fill(~ok, NEG_INF), 6, dim=-1)
    s, i = ivf_search(db8, q, 6, lists, probes, 300, scales=sa)
    assert torch.equal(i, ri) and torch.allclose(s, rs)


# ---------------------------------------------------------------------------
# Recall floor on clustered data (a condition, not a measurement)
# ---------------------------------------------------------------------------
def clustered(seed, d, device="cpu", n=4096, n_centres=32, n_queries=64):
    """Unit-norm fp32 rows around 32 random unit centres, and queries that
    are perturbed rows."""
    g = torch.Generator().manual_seed(seed)
    nz = torch.nn.functional.normalize
    centres = nz(torch.randn(n_centres, d, generator=g), dim=-1)
    which = torch.randint(0, n_centres, (n,), generator=g)
    x = nz(centres[which] + 0.15 * torch.randn(n, d, generator=g), dim=-1)
    pick = torch.randperm(n, generator=g)[:n_queries]
    q = nz(x[pick] + 0.05 * torch.randn(n_queries, d, generator=g), dim=-1)
    return x.to(device), q.to(device)


def recall_at(got_idx, ref_idx):
    hits = sum(len(set(a) & set(b))
               for a, b in zip(got_idx.tolist(), ref_idx.tolist()))
    return hits / ref_idx.numel()


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
N = 3000
C = 24
ROW_BASE = 1000
TAILS = [N, N - 1, N - 37]
# list 0 empty, 1..4 around the 16-lane group count, 5 long enough that a
# block strides through it several times at every Q below; the rest random
FIXED = [0, 1, 15, 16, 17, 1200]
AWKWARD = [0, 1, 2, 3, 4, 5]

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


def _lists(tail_start):
    """CSR over a random permutation of rows [0, tail_start): rows are in
    random order inside every list. Returns (lists on GPU, lists on CPU)."""
    key = ("lists", tail_start)
    if key not in _cache:
        g = torch.Generator().manual_seed(tail_start)
        rest = tail_start - sum(FIXED)
        cuts = torch.sort(torch.randint(0, rest + 1, (C - len(FIXED) - 1,),
                                        generator=g)).values.tolist()
        sizes = FIXED + [b - a for a, b in zip([0] + cuts, cuts + [rest])]
        assert len(sizes) == C and sum(sizes) == tail_start
        off = torch.zeros(C + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(torch.tensor(sizes), 0)
        rows = torch.randperm(tail_start, generator=g).to(torch.int32)
        cpu = IVFLists(torch.zeros(C, 8), off, rows, tail_start, max(sizes))
        gpu = IVFLists(cpu.centroids.cuda(), off.cuda(), rows.cuda(),
                       tail_start, max(sizes))
        _cache[key] = (gpu, cpu)
    return _cache[key]


def _probes(q_count):
    """int32 [Q, 8]: six distinct lists per query with two -1 entries mixed
    in; query 0 probes the awkward lists, query 1 (if any) also carries an
    out-of-range id."""
    key = ("probes", q_count)
    if key not in _cache:
        g = torch.Generator().manual_seed(q_count)
        out = torch.full((q_count, 8), -1, dtype=torch.int32)
        for r in range(q_count):
            cols = torch.randperm(8, generator=g)[:6]
            pick = torch.tensor(AWKWARD) if r == 0 else \
                torch.randperm(C, generator=g)[:6]
            out[r, cols] = pick.to(torch.int32)
        if q_count > 1:
            out[1, (out[1] == -1).nonzero()[0, 0]] = C + 5
        _cache[key] = out
    return _cache[key]


def _case(d, q_count, tail_start, masked):
    """(q bf16 [Q, D], allow bool [N] or None, ok bool [Q, N]). Every query
    copies a row it must not return: a row of a list it does not probe, or
    (masked, odd queries) a disallowed row of a list it does probe."""
    key = ("case", d, q_count, tail_start, masked)
    if key in _cache:
        return _cache[key]
    db = _corpus(d)
    _, cpu = _lists(tail_start)
    probes = _probes(q_count)
    reach = _py_reach(cpu, probes, N, tail_start)
    g = torch.Generator().manual_seed(q_count * 7 + tail_start)
    allow = None
    if masked:
        allow = torch.rand(N, generator=g) < 0.5
    decoys = []
    for r in range(q_count):
        pool = (~reach[r]).nonzero().flatten()
        if masked and r % 2 == 1:
            pool = reach[r].nonzero().flatten()
        row = int(pool[int(torch.randint(0, len(pool), (1,), generator=g))])
        if masked:
            allow[row] = False
        decoys.append(row)
    ok = reach if allow is None else reach & allow[None, :]
    assert not ok[torch.arange(q_count), torch.tensor(decoys)].any()
    q = db[torch.tensor(decoys).cuda()].clone()
    out = (q, None if allow is None else allow.cuda(), ok.cuda())
    _cache[key] = out
    return out


def _check(scores_fn, tol, q, ok, k, row_base, s, i):
    """ok: bool [Q, N], the rows each query may return. scores_fn() is the
    fp32 [Q, N] product of the stored values."""
    torch.cuda.synchronize()
    q_count, n = ok.shape
    kk = min(k, n)
    assert s.shape == (q_count, kk) and i.shape == s.shape
    assert i.dtype == torch.int64 and s.dtype == torch.float32
    ref = scores_fn().masked_fill(~ok, NEG_INF)
    rs, _ = torch.topk(ref, kk, dim=-1)
    m = ok.sum(-1).clamp_max(kk)
    filled = torch.arange(kk, device=s.device)[None, :] < m[:, None]
    assert ((i == -1) == ~filled).all(), i
    assert (s[~filled] == NEG_INF).all(), s
    loc = torch.where(filled, i - row_base, 0)
    assert ((loc >= 0) & (loc < n)).all(), i
    assert (torch.gather(ok, 1, loc) | ~filled).all(), \
        "a row outside the probed, allowed set was returned"
    srt = torch.where(filled, loc, -1 - torch.arange(kk, device=s.device)) \
        .sort(dim=-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "duplicate hit"
    err = (s - rs)[filled].abs().max().item() if filled.any() else 0.0
    own = (torch.gather(ref, 1, loc) - s)[filled].abs().max().item() \
        if filled.any() else 0.0
    print(f"Q={q_count} k={k}: rank err {err:.3e} own err {own:.3e}")
    assert err <= tol, err
    assert own <= tol, own
    assert (s[:, :-1] >= s[:, 1:]).all()


# atol of the gemv route's dot product on unit-norm rows
# (tests/test_ops_vector.py): same fdot2 code here
SCAN_TOL = 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("k", [1, 10, 16, 17, 40, 64])
@pytest.mark.parametrize("q_count", [1, 5, 17])
@pytest.mark.parametrize("d", [128, 1024])
def test_gpu_scan_sweep(d, q_count, k, masked):
    db = _corpus(d)
    probes = _probes(q_count).cuda()
    for tail_start in TAILS:
        lists, _ = _lists(tail_start)
        q, allow, ok = _case(d, q_count, tail_start, masked)
        for row_base in (0, ROW_BASE):
            s, i = ivf_search(db, q, k, lists, probes, tail_start,
                              row_base=row_base, allow=allow)
            _check(lambda: q.float() @ db.float().T, SCAN_TOL, q, ok, k,
                   row_base, s, i)
    # the oracle meets the same contract bit for bit on the same inputs
    es, ei = ivf_search_exact(db, q, k, lists, probes, tail_start,
                              row_base=ROW_BASE, allow=allow)
    _check(lambda: q.float() @ db.float().T, 0.0, q, ok, k, ROW_BASE, es, ei)
    if masked:   # packed form of the mask
        s2, i2 = ivf_search(db, q, k, lists, probes, tail_start,
                            row_base=ROW_BASE, allow=pack_allow_mask(allow))
        assert torch.equal(s, s2) and torch.equal(i, i2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [16, 64])
def test_gpu_scan_all_skipped(k):
    db = _corpus(128)
    lists, _ = _lists(N)
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
    lists37, _ = _lists(N - 37)
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
    lists, _ = _lists(N)
    q = db[:3].contiguous()
    once = torch.tensor([[5, 2, -1, -1]] * 3, dtype=torch.int32).cuda()
    twice = torch.tensor([[5, 2, 5, 2]] * 3, dtype=torch.int32).cuda()
    s1, i1 = ivf_search(db, q, 40, lists, once, N)
    s2, i2 = ivf_search(db, q, 40, lists, twice, N)
    torch.cuda.synchronize()
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    assert (i1 >= 0).all()


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
    lists, _ = _lists(tail_start)
    probes = _probes(5).cuda()
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
    _check(lambda: qv @ vals.T, FALLBACK_TOL, q, ok, k, ROW_BASE, s, i)


@pytest.mark.gpu
def test_gpu_wrapper_rejects_bad_arguments():
    from nornicdb_amd.ops import require_native
    nat = require_native()
    db = _corpus(128)
    lists, cpu = _lists(N)
    q = db[:2].contiguous()
    pr = _probes(2).cuda()
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
