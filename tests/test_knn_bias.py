"""Per-row score bias of the bf16 kNN routes: score = q.x + row_bias[row].

CPU: the exact route against topk(q @ db.T + b), alone and combined with an
allow-mask, a row_base and fewer allowed rows than k.

GPU: the gemv and the MFMA route (main panels, tail, several panels per
block) with inputs whose scores are exact in fp32, so scores and indices
must equal the fp32 reference bit for bit; a zero corpus whose ranking is
the bias alone (row mapping); a bias that overturns the ranking; the bias
under a mask; and float inputs within the routes' usual tolerances.
"""

import pytest
import torch

from nornicdb_amd.ops import knn_search, knn_search_exact
from nornicdb_amd.ops.knn import (_knn_bm, knn_search_int8, pack_allow_mask,
                                  quantize_fp8, quantize_int8)

NEG_INF = float("-inf")


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def _cpu_case(seed, n=500, d=64, q=7):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g), torch.randn(q, d, generator=g),
            torch.randn(n, generator=g) * 3.0)


def test_cpu_bias_equals_topk():
    db, q, b = _cpu_case(0)
    rs, ri = torch.topk(q @ db.T + b, 5, dim=-1)
    s, i = knn_search(db, q, 5, row_bias=b)
    assert torch.equal(i, ri)
    assert torch.allclose(s, rs)
    # the bias matters: the unbiased ranking is another one
    _, ui = knn_search(db, q, 5)
    assert not torch.equal(ui, ri)
    # and the exact reference takes the same argument
    es, ei = knn_search_exact(db, q, 5, row_bias=b)
    assert torch.equal(ei, ri) and torch.allclose(es, rs)


def test_cpu_bias_with_allow_and_row_base():
    db, q, b = _cpu_case(1)
    allow = torch.rand(500, generator=torch.Generator().manual_seed(11)) < 0.3
    rs, ri = torch.topk((q @ db.T + b).masked_fill(~allow, NEG_INF), 5, dim=-1)
    for mask in (allow, pack_allow_mask(allow)):
        s, i = knn_search(db, q, 5, row_base=1000, allow=mask, row_bias=b)
        assert torch.equal(i, ri + 1000)
        assert torch.allclose(s, rs)


def test_cpu_bias_fewer_allowed_than_k_pads():
    db, q, b = _cpu_case(2)
    allow = torch.zeros(500, dtype=torch.bool)
    allow[[3, 50, 499]] = True
    s, i = knn_search(db, q, 8, row_base=10, allow=allow, row_bias=b)
    assert s.shape == (7, 8) and i.shape == (7, 8)
    ref = q @ db.T + b
    for r in range(7):
        order = sorted([3, 50, 499], key=lambda x: -ref[r, x].item())
        assert i[r, :3].tolist() == [x + 10 for x in order]
        assert torch.allclose(s[r, :3], ref[r, order])
    assert (i[:, 3:] == -1).all()
    assert (s[:, 3:] == NEG_INF).all()


def test_bias_rejected_on_quantised_corpora():
    db, q, b = _cpu_case(3, n=200)
    with pytest.raises(ValueError):
        knn_search(quantize_fp8(db), q, 5, row_bias=b)
    d8, sa = quantize_int8(db)
    with pytest.raises(ValueError):
        knn_search_int8(d8, sa, q, 5, row_bias=b)
    with pytest.raises(ValueError):
        knn_search(db, q, 5, row_bias=b[:-1])


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
ROW_BASE = 1000


def _exact_inputs(n, d, q_count, seed):
    """Integer entries in [-2, 2] (exact in bf16) and a bias b_r + r/4096
    with integer b_r in [-256, 0]. Every score is a multiple of 2^-12 below
    2^10 in magnitude (|dot| <= 4 * d = 512), 22 bits: exact in fp32 in any
    summation order. The fractions r/4096, r < 4096, are distinct, so no
    two rows tie for any query. All on the CPU; callers move what they use."""
    assert n <= 4096
    g = torch.Generator().manual_seed(seed)
    db = torch.randint(-2, 3, (n, d), generator=g).float()
    q = torch.randint(-2, 3, (q_count, d), generator=g).float()
    b = torch.randint(-256, 1, (n,), generator=g).float() + \
        torch.arange(n).float() / 4096.0
    return db, q, b


def _run_exact(n, d, q_count, k, seed, row_base=0, allow=None):
    """Biased search on the GPU against knn_search_exact in fp32 on the CPU:
    equal scores and indices, bit for bit."""
    db, q, b = _exact_inputs(n, d, q_count, seed)
    rs, ri = knn_search_exact(db, q, k, row_base, allow=allow, row_bias=b)
    s, i = knn_search(db.to("cuda", torch.bfloat16),
                      q.to("cuda", torch.bfloat16), k, row_base,
                      allow=None if allow is None else allow.cuda(),
                      row_bias=b.cuda())
    torch.cuda.synchronize()
    assert i.dtype == torch.int64 and s.dtype == torch.float32
    assert torch.equal(i.cpu(), ri), (i.cpu() - ri).nonzero()[:8]
    assert torch.equal(s.cpu(), rs)
    # the bias took part: without it the ranking is another one
    _, ui = knn_search_exact(db, q, k, row_base, allow=allow)
    assert not torch.equal(ui, ri)


@pytest.mark.gpu
@pytest.mark.parametrize("q_count", [1, 8])
def test_gpu_exact_gemv(q_count):
    _run_exact(1000, 128, q_count, 16, seed=q_count)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("q_count", [9, 256])
def test_gpu_exact_mfma(q_count, d):
    """Two panels and a 37-row tail."""
    _run_exact(2 * _knn_bm() + 37, d, q_count, 10, seed=q_count + d,
               row_base=ROW_BASE)


@pytest.mark.gpu
def test_gpu_exact_mfma_one_block_three_panels(monkeypatch):
    """One block walks three panels: its bias fetches cross panel
    boundaries with the stage stream."""
    monkeypatch.setenv("NORNICDB_KNN_GRID", "1")
    _run_exact(3 * _knn_bm(), 128, 40, 10, seed=5, row_base=ROW_BASE)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["gemv", "mfma"])
def test_gpu_row_mapping(route):
    """Zero corpus, bias a permutation of 0..N-1: the top-k of every query
    is the k largest biases in order, whatever the query. Any bias attached
    to the wrong row shows, in every 16-row chunk, both row groups and the
    tail; no dot product can cover for it."""
    q_count, k, n = (3, 16, 1000) if route == "gemv" \
        else (40, 10, 2 * _knn_bm() + 37)
    g = torch.Generator().manual_seed(n)
    perm = torch.randperm(n, generator=g)
    b = perm.float()
    db = torch.zeros(n, 128, device="cuda", dtype=torch.bfloat16)
    q = torch.randn(q_count, 128, generator=g).to("cuda", torch.bfloat16)
    s, i = knn_search(db, q, k, ROW_BASE, row_bias=b.cuda())
    torch.cuda.synchronize()
    want_i = torch.argsort(perm, descending=True)[:k] + ROW_BASE
    want_s = torch.arange(n - 1, n - 1 - k, -1).float()
    assert torch.equal(i.cpu(), want_i.expand(q_count, k))
    assert torch.equal(s.cpu(), want_s.expand(q_count, k))
    # every 7th row, through every chunk: a bias of 2n on row r puts r first
    bd = b.cuda()
    for r in range(0, n, 7):
        b2 = bd.clone()
        b2[r] = 2.0 * n
        _, i2 = knn_search(db, q[:min(q_count, 9)], 1, 0, row_bias=b2)
        assert (i2 == r).all(), r


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["gemv", "mfma"])
def test_gpu_bias_decides(route):
    """Unit-norm rows; a bias of +4 lifts the 10 lowest-scoring rows above
    every inner product (all within [-1, 1]): the biased top-10 is exactly
    those rows and shares nothing with the unbiased top-10."""
    n, d = 2 * _knn_bm() + 37, 128
    q_count = 1 if route == "gemv" else 16
    g = torch.Generator().manual_seed(3)
    db = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)
    q0 = torch.nn.functional.normalize(torch.randn(1, d, generator=g), dim=-1)
    # queries close to one another, so "lowest-scoring" means the same rows
    q = torch.nn.functional.normalize(
        q0 + 0.02 * torch.randn(q_count, d, generator=g), dim=-1)
    dbh, qh = db.to(torch.bfloat16), q.to(torch.bfloat16)
    ref = qh.float() @ dbh.float().T
    low = torch.topk(ref.mean(0), 10, largest=False).indices
    # a property of the inputs: the lifted rows are far from any top-10
    assert not set(low.tolist()) & set(torch.topk(ref, 30).indices.flatten().tolist())
    b = torch.zeros(n)
    b[low] = 4.0
    us, ui = knn_search(dbh.cuda(), qh.cuda(), 10)
    s, i = knn_search(dbh.cuda(), qh.cuda(), 10, row_bias=b.cuda())
    torch.cuda.synchronize()
    for r in range(q_count):
        assert set(i[r].tolist()) == set(low.tolist())
        assert not set(i[r].tolist()) & set(ui[r].tolist())
    assert (s >= 3.0).all() and (us <= 1.01).all()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["gemv", "mfma"])
def test_gpu_filtered_biased_exact(route):
    """Random 30 % mask over the exact-arithmetic inputs: mask and bias
    combine, bit for bit."""
    q_count, k, n = (8, 16, 1000) if route == "gemv" \
        else (40, 10, 2 * _knn_bm() + 37)
    allow = torch.rand(n, generator=torch.Generator().manual_seed(9)) < 0.3
    _run_exact(n, 128, q_count, k, seed=21, row_base=ROW_BASE, allow=allow)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["gemv", "mfma"])
def test_gpu_filtered_biased_padding(route):
    """3 allowed rows, k = 8: three hits in biased order, then (-inf, -1)."""
    q_count, n = (2, 1000) if route == "gemv" else (40, 2 * _knn_bm() + 37)
    db, q, b = _exact_inputs(n, 128, q_count, seed=31)
    allow = torch.zeros(n, dtype=torch.bool)
    rows = [5, _knn_bm() + 170, n - 1]   # both row groups' panels and the tail
    allow[rows] = True
    s, i = knn_search(db.to("cuda", torch.bfloat16),
                      q.to("cuda", torch.bfloat16), 8, ROW_BASE,
                      allow=allow.cuda(), row_bias=b.cuda())
    torch.cuda.synchronize()
    s, i = s.cpu(), i.cpu()
    assert s.shape == (q_count, 8)
    ref = q @ db.T + b
    for r in range(q_count):
        order = sorted(rows, key=lambda x: -ref[r, x].item())
        assert i[r, :3].tolist() == [x + ROW_BASE for x in order]
        assert torch.equal(s[r, :3], ref[r, order])
    assert (i[:, 3:] == -1).all()
    assert (s[:, 3:] == NEG_INF).all()


# gemv 1e-2, MFMA bf16 2e-2: the atol of the routes' unbiased tests in
# tests/test_ops_vector.py, as quoted in tests/test_knn_filtered.py
@pytest.mark.gpu
@pytest.mark.parametrize("route,q_count,k,tol", [("gemv", 4, 16, 1e-2),
                                                 ("mfma", 40, 10, 2e-2)])
def test_gpu_float_euclidean_bias(route, q_count, k, tol):
    """Rows of norm 0.5..4 with the Euclidean bias -|x|^2/2 of the stored
    values, against fp32 scores of the same stored values: rank-by-rank
    scores and each returned row's own score, as test_knn_filtered compares
    a route with its reference. |q.x| <= 4 and |bias| <= 8: the one extra
    fp32 rounding is of a sum below 16, about 1e-6."""
    n, d = 2 * _knn_bm() + 37, 128
    g = torch.Generator().manual_seed(17)
    db = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)
    db = (db * (0.5 + 3.5 * torch.rand(n, 1, generator=g))).to(torch.bfloat16)
    # half the queries near a stored row, half unrelated; norm <= 1
    q = torch.nn.functional.normalize(torch.randn(q_count, d, generator=g),
                                      dim=-1)
    near = torch.randperm(n, generator=g)[:q_count // 2]
    q[:q_count // 2] = torch.nn.functional.normalize(db[near].float(), dim=-1)
    q = q.to(torch.bfloat16)
    b = -0.5 * db.float().square().sum(-1)
    ref = q.float() @ db.float().T + b
    rs, _ = torch.topk(ref, k, dim=-1)
    s, i = knn_search(db.cuda(), q.cuda(), k, ROW_BASE, row_bias=b.cuda())
    torch.cuda.synchronize()
    s, loc = s.cpu(), i.cpu() - ROW_BASE
    assert ((loc >= 0) & (loc < n)).all()
    srt = loc.sort(dim=-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "duplicate hit"
    err = (s - rs).abs().max().item()
    own = (torch.gather(ref, 1, loc) - s).abs().max().item()
    print(f"{route}: rank err {err:.3e} own err {own:.3e}")
    assert err <= tol, err
    assert own <= tol, own
    assert (s[:, :-1] >= s[:, 1:]).all()
