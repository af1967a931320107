"""Pipelined fused kNN kernel (csrc/knn_mfma.hip): stage stream, buffer
rotation across panels, filtered panel skip.

Every case goes through knn_search and is compared with fp32 exact scoring
of the stored bf16 values at the MFMA route's atol of 2e-2. A returned
index is accepted when its exact score is within that atol of the exact
k-th score (ties and near-ties may legitimately swap).

Shapes are the smallest that reach every path of the stage stream: D=64 is
shorter than the prefetch distance (every corpus prefetch crosses a panel
boundary), D=192 walks the 3-deep corpus ring and the 2-deep query ring out
of phase with the panel length, NORNICDB_KNN_GRID in {1, 2, 3} makes one
workgroup walk many panels. Row counts come in two sets: multiples of 96
and multiples of the panel height the kernel was compiled with (PANEL), so
that panel edges are hit whatever that height is.
"""

import functools

import pytest
import torch

from nornicdb_amd.ops import knn_search
from nornicdb_amd.ops.knn import _knn_bm

pytestmark = pytest.mark.gpu

ATOL = 2e-2
PANEL = _knn_bm()  # rows per panel of the compiled kernel
DIMS = [64, 128, 192, 1024]
ROWS = sorted({m * h + t for h in (96, PANEL)
               for m, t in ((1, 0), (2, 0), (5, 17), (37, 0))})
GRIDS = ["1", "2", "3", None]


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("NORNICDB_KNN_GRID", raising=False)
    else:
        monkeypatch.setenv("NORNICDB_KNN_GRID", grid)


@functools.lru_cache(maxsize=None)
def _unit(n, d, seed):
    """[n, d] bf16 unit rows on the GPU; cached, never modified in place."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, d, device="cuda", generator=g)
    return torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)


def _exact(db, q, allow=None):
    sc = q.float() @ db.float().T
    if allow is not None:
        sc = sc.masked_fill(~allow, float("-inf"))
    return sc


def _check(s, i, db, q, k, row_base=0, allow=None):
    """(s, i) against fp32 exact scoring of db/q; returns the exact scores."""
    sc = _exact(db, q, allow)
    kk = min(k, db.shape[0])
    s_ref = torch.topk(sc, kk, dim=-1).values
    assert s.shape == s_ref.shape and i.shape == s_ref.shape
    assert torch.allclose(s, s_ref, atol=ATOL), (s - s_ref).abs().max()
    filled = i >= 0
    # unfilled slots exist only under a mask and are exactly (-inf, -1)
    assert (filled == (s_ref > float("-inf"))).all()
    assert (s[~filled] == float("-inf")).all() and (i[~filled] == -1).all()
    loc = (i - row_base).clamp_min(0)
    assert (loc < db.shape[0]).all()
    got = torch.gather(sc, 1, loc)
    assert ((got - s).abs() <= ATOL)[filled].all()
    kth = s_ref[:, -1:].clamp_min(-1e30)
    assert (got >= kth - ATOL)[filled].all()
    # no index twice in a row of results
    srt = torch.sort(torch.where(filled, i, -1 - torch.arange(
        kk, device=i.device).expand_as(i)), dim=-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all()
    return sc


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("d", DIMS)
def test_shape_sweep(d, grid, monkeypatch):
    _set_grid(monkeypatch, grid)
    db_all = _unit(ROWS[-1], d, 100 + d)
    for q_count in (9, 256):
        q = _unit(256, d, 200 + d)[:q_count]
        for n in ROWS:
            db = db_all[:n]
            s, i = knn_search(db, q, 10, row_base=7)
            _check(s, i, db, q, 10, row_base=7)


@pytest.mark.parametrize("grid", ["1", None], ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("d", [192, 1024])
def test_planted_winners(d, grid, monkeypatch):
    """Copies of queries in the first and last row of the first, a middle
    and the last panel come back exactly, at rank 1, with row_base added."""
    _set_grid(monkeypatch, grid)
    n_panels = 37
    db = _unit(n_panels * PANEL, d, 300 + d).clone()
    q = _unit(256, d, 400 + d)
    rows = [p * PANEL + r for p in (0, n_panels // 2, n_panels - 1)
            for r in (0, PANEL - 1)]
    for j, r in enumerate(rows):
        db[r] = q[j]
    row_base = 1_000_003
    s, i = knn_search(db, q, 10, row_base=row_base)
    _check(s, i, db, q, 10, row_base=row_base)
    want = torch.tensor(rows, device="cuda") + row_base
    assert (i[:len(rows), 0] == want).all(), (i[:len(rows), 0], want)
    assert (s[:len(rows), 0] > 0.9).all()


@pytest.mark.parametrize("grid", ["1", None], ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("d", DIMS)
def test_k_slice_canary(d, shift, grid, monkeypatch):
    """Row r is non-zero in exactly one 32-wide K slice, r mod (D/32), with
    a value that depends on r; the queries are all ones. A stage that is
    read early, stale or twice moves a score by a whole slice (to zero or
    to double), not by a rounding error. All values and sums are exact in
    bf16/fp32."""
    _set_grid(monkeypatch, grid)
    n = 37 * PANEL
    r = torch.arange(n, device="cuda")
    val = (1.0 + ((r * 37 + shift * 61) % 128).float() / 128.0) \
        * torch.exp2(-((r // 128 + shift) % 4).float())
    sl = r % (d // 32)
    col = torch.arange(d, device="cuda")
    db = torch.where((col[None, :] // 32) == sl[:, None], val[:, None],
                     torch.zeros((), device="cuda")).to(torch.bfloat16)
    assert (db.float().sum(-1) == 32 * val).all()  # exactly representable
    q = torch.ones(256, d, device="cuda", dtype=torch.bfloat16)
    s, i = knn_search(db, q, 10)
    sc = _check(s, i, db, q, 10)
    # exact arithmetic: the scores must match bit for bit
    assert (s == torch.topk(sc, 10, dim=-1).values).all()


def _panel_mask(n, live_panels, single=None):
    allow = torch.zeros(n, dtype=torch.bool, device="cuda")
    for p in live_panels:
        allow[p * PANEL:(p + 1) * PANEL] = True
    if single is not None:
        p, r = single
        allow[p * PANEL:(p + 1) * PANEL] = False
        allow[p * PANEL + r] = True
    return allow


@pytest.mark.parametrize("d", [64, 192, 1024])
def test_filtered_panel_skip_one_block(d, monkeypatch):
    """One workgroup walks all panels: all-zero panels at the start, between
    two live panels and at the end, and a panel with a single allowed row."""
    monkeypatch.setenv("NORNICDB_KNN_GRID", "1")
    n = 9 * PANEL + 17
    db = _unit(n, d, 500 + d)
    q = _unit(256, d, 600 + d)
    # panels 0,1 dead; 2 live; 3 dead; 4 live; 5 one row; 6 live; 7,8 dead
    allow = _panel_mask(n, [2, 4, 6], single=(5, 41))
    for tail in (False, True):
        allow[9 * PANEL:] = tail
        s, i = knn_search(db, q, 10, row_base=11, allow=allow)
        _check(s, i, db, q, 10, row_base=11, allow=allow)
        assert allow[(i[i >= 0] - 11)].all()

    # fewer allowed rows than k: one row of one panel, the rest padding
    allow = _panel_mask(n, [], single=(5, PANEL - 1))
    s, i = knn_search(db, q, 10, row_base=11, allow=allow)
    _check(s, i, db, q, 10, row_base=11, allow=allow)
    assert (i[:, 0] == 11 + 5 * PANEL + PANEL - 1).all()
    assert (i[:, 1:] == -1).all() and (s[:, 1:] == float("-inf")).all()


@pytest.mark.parametrize("grid", ["1", None], ids=lambda g: f"grid{g}")
def test_back_to_back_calls(grid, monkeypatch):
    """Two calls on different corpora of equal size on one stream: neither
    may see the other's staged tiles or candidate buffers."""
    _set_grid(monkeypatch, grid)
    d, n = 192, 37 * PANEL
    db1, db2 = _unit(n, d, 701), _unit(n, d, 702)
    q = _unit(256, d, 703)
    s1, i1 = knn_search(db1, q, 10)
    s2, i2 = knn_search(db2, q, 10)
    _check(s2, i2, db2, q, 10)
    _check(s1, i1, db1, q, 10)
