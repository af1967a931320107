"""Row groups of the fused kNN kernel (csrc/knn_mfma.hip, KNN_RG): a panel
of P rows is KNN_RG row groups of H = P / KNN_RG rows, each with its own
top-k list per query column, its own candidate list and its own slice of the
allow mask; the query stage is staged once for all of them.

Every case goes through knn_search and is compared with fp32 exact scoring
of the stored bf16 values at the MFMA route's atol of 2e-2; a returned index
is accepted when its exact score is within that atol of the exact k-th score
(the rule of test_knn_pipeline._check). Planted rows are exact copies of
queries, so their rank and index are checked exactly.

Shapes: D=64 (every corpus prefetch crosses a panel boundary) and D=192
(rings out of phase with the panel), at most 37 panels, Q=256 and Q=9,
NORNICDB_KNN_GRID=1 (one workgroup walks all panels, two candidate lists)
and the default grid (one panel per workgroup).
"""

import functools

import pytest
import torch

from nornicdb_amd.ops import knn_search, native_or_none
from nornicdb_amd.ops.knn import _knn_bm

pytestmark = pytest.mark.gpu

ATOL = 2e-2
P = _knn_bm()                                        # rows per panel
RG = int(getattr(native_or_none(), "KNN_RG", 1))     # row groups per panel
H = P // RG                                          # rows per row group
N_PANELS = 37
DIMS = [64, 192]
GRIDS = ["1", None]
QS = [256, 9]

seam = pytest.mark.skipif(RG < 2, reason="built with one row group per panel")


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


def _check(s, i, db, q, k, row_base=0, allow=None):
    """(s, i) against fp32 exact scoring of db/q; returns the exact scores."""
    sc = q.float() @ db.float().T
    if allow is not None:
        sc = sc.masked_fill(~allow, float("-inf"))
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


@seam
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("q_count", QS)
@pytest.mark.parametrize("d", DIMS)
def test_planted_winners_on_the_seam(d, q_count, grid, monkeypatch):
    """Copies of queries in the last row of row group 0 and the first row of
    row group 1, and in the first and last row of the panel, of the first, a
    middle and the last panel: each at rank 1, with row_base added."""
    _set_grid(monkeypatch, grid)
    db = _unit(N_PANELS * P, d, 1100 + d).clone()
    q = _unit(256, d, 1200 + d)[:q_count]
    panels = (0, N_PANELS // 2, N_PANELS - 1)
    # seam rows first, so that Q=9 still covers the seam of every panel
    rows = [p * P + r for r in (H - 1, H) for p in panels] + \
           [p * P + r for r in (0, P - 1) for p in panels]
    rows = rows[:q_count]
    for j, r in enumerate(rows):
        db[r] = q[j]
    row_base = 1_000_003
    s, i = knn_search(db, q, 10, row_base=row_base)
    _check(s, i, db, q, 10, row_base=row_base)
    want = torch.tensor(rows, device="cuda") + row_base
    assert (i[:len(rows), 0] == want).all(), (i[:len(rows), 0], want)
    assert (s[:len(rows), 0] > 0.9).all()


@seam
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("q_count", QS)
@pytest.mark.parametrize("d", DIMS)
def test_both_lists_of_one_column(d, q_count, grid, monkeypatch):
    """One query has 20 scaled copies: 5 in row group 0 and 5 in row group 1
    of one panel, 10 in row group 1 of a later panel. The answer is the 10
    largest scales across all three lists, in order.

    The query is +-1/8 everywhere and the scales are c/16 with 20 <= c < 40
    (six significant bits), so rows, products and partial sums are exact in
    bf16/fp32: the 20 scores are distinct and compared bit for bit. Every
    other row is a unit vector and scores at most |query| < the smallest
    planted score. With the default grid the panels sit in the second half,
    where a merge over only gridDim.x lists would not look."""
    _set_grid(monkeypatch, grid)
    db = _unit(N_PANELS * P, d, 1300 + d).clone()
    q = _unit(256, d, 1400 + d)[:q_count].clone()
    jq = 5
    sign = torch.where(_unit(1, d, 1500 + d)[0] >= 0, 1.0, -1.0)
    q[jq] = (sign / 8).to(torch.bfloat16)
    scale = (20 + torch.arange(20, device="cuda")).float() / 16   # ascending
    pa, pb = N_PANELS // 2 + 1, N_PANELS - 3
    place = {}  # scale rank -> corpus row
    for ranks, lo, step in (
            ((19, 16, 13, 10, 7), pa * P, H // 5 - 1),          # pa, group 0
            ((18, 15, 12, 9, 6), pa * P + H, H // 5 - 1),       # pa, group 1
            ((17, 14, 11, 8, 5, 4, 3, 2, 1, 0), pb * P + H, H // 10 - 1)):
        for n_, c in enumerate(ranks):
            place[c] = lo + 1 + step * n_
            assert lo <= place[c] < lo + H
    assert sorted(place) == list(range(20))
    for c, r in place.items():
        db[r] = (q[jq].float() * scale[c]).to(torch.bfloat16)
        assert (db[r].float() == q[jq].float() * scale[c]).all()
    row_base = 77
    s, i = knn_search(db, q, 10, row_base=row_base)
    sc = _check(s, i, db, q, 10, row_base=row_base)
    want_i = torch.tensor([place[c] for c in range(19, 9, -1)],
                          device="cuda") + row_base
    assert (i[jq] == want_i).all(), (i[jq], want_i)
    assert (s[jq] == torch.topk(sc[jq], 10).values).all()
    assert (s[jq] == scale.flip(0)[:10] * (d / 64.0)).all()


@pytest.mark.parametrize("q_count", QS)
@pytest.mark.parametrize("d", DIMS)
def test_one_panel_and_neighbours(d, q_count, monkeypatch):
    """n = P with one block (one panel, nothing else), n = P + 17 (panel
    plus torch-scored tail) and n = P - 1 (below the kernel route)."""
    monkeypatch.setenv("NORNICDB_KNN_GRID", "1")
    db_all = _unit(P + 17, d, 1600 + d).clone()
    q = _unit(256, d, 1700 + d)[:q_count]
    db_all[H - 1], db_all[H % P], db_all[P - 2] = q[0], q[1], q[2]
    for n in (P, P + 17, P - 1):
        db = db_all[:n]
        s, i = knn_search(db, q, 10, row_base=5)
        _check(s, i, db, q, 10, row_base=5)
        want = torch.tensor([H - 1, H % P, P - 2], device="cuda") + 5
        assert (i[:3, 0] == want).all(), (n, i[:3, 0])


def _mask(n, spans):
    allow = torch.zeros(n, dtype=torch.bool, device="cuda")
    for lo, hi in spans:
        allow[lo:hi] = True
    return allow


@seam
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("q_count", QS)
@pytest.mark.parametrize("d", DIMS)
def test_filtered_row_groups(d, q_count, grid, monkeypatch):
    """Masks that split a panel along the row-group seam; with grid 1 one
    workgroup walks dead panels before, between and after the live ones.

    panel 0 dead | 1 only row group 1 | 2 dead | 3 only row group 0 | 4 dead
    | 5 only row H-1 | 6 only row H | 7 all | 8 dead | 17-row tail."""
    _set_grid(monkeypatch, grid)
    n = 9 * P + 17
    db = _unit(n, d, 1800 + d).clone()
    q = _unit(256, d, 1900 + d)[:q_count]
    # allowed copies: must win. Copies under the mask: must not come back.
    win = [1 * P + H, 1 * P + P - 1, 3 * P, 3 * P + H - 1, 5 * P + H - 1,
           6 * P + H]
    hidden = [1 * P + H - 1, 3 * P + H, 0 * P + H]
    for j, r in enumerate(win):
        db[r] = q[j]
    for j, r in enumerate(hidden):
        db[r] = q[len(win) + j]
    spans = [(1 * P + H, 2 * P), (3 * P, 3 * P + H),
             (5 * P + H - 1, 5 * P + H), (6 * P + H, 6 * P + H + 1),
             (7 * P, 8 * P)]
    for tail in (False, True):
        allow = _mask(n, spans + ([(9 * P, n)] if tail else []))
        s, i = knn_search(db, q, 10, row_base=11, allow=allow)
        _check(s, i, db, q, 10, row_base=11, allow=allow)
        assert allow[(i[i >= 0] - 11)].all()
        want = torch.tensor(win, device="cuda") + 11
        assert (i[:len(win), 0] == want).all(), (i[:len(win), 0], want)
        assert (s[len(win):len(win) + len(hidden), 0] < 0.9).all()

    # fewer allowed rows than k: the two rows on either side of one seam
    # and of another panel's, the rest is padding
    allow = _mask(n, [(5 * P + H - 1, 5 * P + H), (6 * P + H, 6 * P + H + 1)])
    s, i = knn_search(db, q, 10, row_base=11, allow=allow)
    _check(s, i, db, q, 10, row_base=11, allow=allow)
    both = torch.tensor([5 * P + H - 1, 6 * P + H], device="cuda") + 11
    assert (torch.sort(i[:, :2], dim=-1).values == both).all()
    assert (i[:, 2:] == -1).all() and (s[:, 2:] == float("-inf")).all()
    assert i[4, 0] == both[0] and i[5, 0] == both[1]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
def test_back_to_back_calls(grid, monkeypatch):
    """Two calls on different corpora of equal size on one stream: neither
    may see the other's candidate lists (gridDim.x * KNN_RG of them each).
    Each corpus has its own winners in the last row group of a late panel."""
    _set_grid(monkeypatch, grid)
    d, n = 192, N_PANELS * P
    db1, db2 = _unit(n, d, 2001).clone(), _unit(n, d, 2002).clone()
    q = _unit(256, d, 2003)
    r1, r2 = (N_PANELS - 1) * P + P - 1, (N_PANELS - 2) * P + P - H
    db1[r1], db2[r2] = q[0], q[0]
    s1, i1 = knn_search(db1, q, 10)
    s2, i2 = knn_search(db2, q, 10)
    _check(s2, i2, db2, q, 10)
    _check(s1, i1, db1, q, 10)
    assert i1[0, 0] == r1 and i2[0, 0] == r2
