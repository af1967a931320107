"""Staggered row groups of the fused kNN kernel (csrc/knn_mfma.hip,
KNN_STAGGER): row group 1 runs half a stage behind row group 0, each group
stages its own corpus rows and row group 0 stages the query tile for both.
A fragment read that is placed one barrier interval too early, or a DMA one
interval too early, reads or overwrites a stale tile, so every case here is
bit-exact over the whole result.

Inputs are randint(-2, 3) / 8 in bf16: every product is a multiple of 1/64
and every partial sum of up to 1024 of them is exact in fp32, so the fp32
reference q @ db.T is exact in any summation order and the kernel has to
match it bit for bit. Scores tie often; the checks are the ones that hold
under ties: the returned scores are the reference's top 10, the score at
every returned index is the returned score, no index repeats, and every
strict winner (reference score above the query's 10th best) is returned.

Shapes: P = one panel (320 rows); 2, 3 and 7 panels (9 for the filtered
case); D = 64 (every prefetch crosses a panel boundary), 192 (rings out of
phase with the panel) and 1024; Q = 256 and 9; NORNICDB_KNN_GRID 1, 2 (two
blocks with different panel counts at 7 panels) and the default.
"""

import functools

import pytest
import torch

from nornicdb_amd.ops import knn_search, native_or_none
from nornicdb_amd.ops.knn import _knn_bm

P = _knn_bm()                                        # rows per panel
RG = int(getattr(native_or_none(), "KNN_RG", 1))     # row groups per panel
H = P // RG                                          # rows per row group

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(RG < 2, reason="built with one row group per panel"),
]

K = 10
DIMS = [64, 192, 1024]
QS = [256, 9]
GRIDS = ["1", "2", None]
NEG_INF = float("-inf")


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("NORNICDB_KNN_GRID", raising=False)
    else:
        monkeypatch.setenv("NORNICDB_KNN_GRID", grid)


@functools.lru_cache(maxsize=None)
def _exact(n, d, seed):
    """[n, d] bf16 on the GPU with values in {-2..2}/8, drawn on the CPU;
    cached, never modified in place."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (n, d), generator=g).float() / 8
    return x.to(torch.bfloat16).cuda()


@functools.lru_cache(maxsize=None)
def _case(panels, d, corpus_seed=None):
    """(db, q, exact fp32 scores [256, n]) of one shape; cached, read-only."""
    seed = 100 + d + panels if corpus_seed is None else corpus_seed
    db = _exact(panels * P, d, seed)
    q = _exact(256, d, 200 + d)
    return db, q, q.float() @ db.float().T


def _check_exact(s, i, ref, row_base=0):
    """(s, i) against the exact scores `ref` [Q, n] (-inf where masked)."""
    s_ref = torch.topk(ref, K, dim=-1).values
    assert s.shape == s_ref.shape and i.shape == s_ref.shape
    assert s.dtype == torch.float32 and i.dtype == torch.int64
    assert (s == s_ref).all(), (s != s_ref).nonzero()[:8]
    filled = s_ref > NEG_INF
    # unfilled slots are exactly (-inf, -1); filled ones carry a row index
    assert ((i >= 0) == filled).all()
    assert (i[~filled] == -1).all() and (s[~filled] == NEG_INF).all()
    loc = (i - row_base).clamp_min(0)
    assert (loc < ref.shape[1]).all()
    # the score at every returned index is the returned score
    assert (torch.gather(ref, 1, loc) == s)[filled].all()
    # no index twice in a row of results
    srt = torch.sort(torch.where(filled, i, -1 - torch.arange(
        K, device=i.device).expand_as(i)), dim=-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all()
    # every strict winner is returned
    returned = torch.zeros_like(ref, dtype=torch.bool)
    returned.scatter_(1, loc, filled)
    missed = (ref > s_ref[:, -1:]) & ~returned
    assert not missed.any(), missed.nonzero()[:8]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("panels", [2, 3, 7])
def test_every_piece_holds_a_strict_winner(panels, d):
    """Condition on the reference alone: at Q = 256 every 8-row piece of
    the corpus (the smallest unit one LDS-DMA instruction stages) contains
    a strict winner of some query, so a fault in any staged piece changes
    a result that test_whole_result_exact compares."""
    _, _, ref = _case(panels, d)
    kth = torch.topk(ref, K, dim=-1).values[:, -1:]
    wins = (ref > kth).any(dim=0)                     # [n]: row wins somewhere
    per_piece = wins.view(-1, 8).sum(dim=1)
    assert per_piece.shape[0] == panels * P // 8
    assert (per_piece >= 1).all(), (per_piece == 0).nonzero().flatten()


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("q_count", QS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("panels", [2, 3, 7])
def test_whole_result_exact(panels, d, q_count, grid, monkeypatch):
    _set_grid(monkeypatch, grid)
    db, q, ref = _case(panels, d)
    row_base = 1_000_003
    s, i = knn_search(db, q[:q_count], K, row_base=row_base)
    _check_exact(s, i, ref[:q_count], row_base=row_base)


def _mask(n, spans):
    allow = torch.zeros(n, dtype=torch.bool, device="cuda")
    for lo, hi in spans:
        allow[lo:hi] = True
    return allow


@pytest.mark.parametrize("q_count", QS)
@pytest.mark.parametrize("d", DIMS)
def test_filtered_exact(d, q_count, monkeypatch):
    """One workgroup walks 9 panels, the live ones separated by dead ones,
    so both row groups have to keep their barrier count across skips:

    panel 0 dead | 1 only row group 0 | 2 dead | 3 only row group 1 | 4, 5
    dead | 6 all | 7 every third row | 8 dead.

    Then three allowed rows in all (fewer than k): one in each row group of
    different panels and the last row of a row group 0."""
    monkeypatch.setenv("NORNICDB_KNN_GRID", "1")
    db, q, ref = _case(9, d)
    n = 9 * P
    allow = _mask(n, [(1 * P, 1 * P + H), (3 * P + H, 4 * P), (6 * P, 7 * P)])
    allow[7 * P:8 * P:3] = True
    few = _mask(n, [(1 * P + 3, 1 * P + 4), (3 * P + H + 5, 3 * P + H + 6),
                    (6 * P + H - 1, 6 * P + H)])
    for m in (allow, few):
        s, i = knn_search(db, q[:q_count], K, row_base=11, allow=m)
        _check_exact(s, i, ref[:q_count].masked_fill(~m, NEG_INF),
                     row_base=11)
        assert m[i[i >= 0] - 11].all()
    assert (i[:, 3:] == -1).all() and (i[:, :3] >= 0).all()


@pytest.mark.parametrize("d", [64, 1024])
def test_back_to_back_calls_exact(d, monkeypatch):
    """Two calls on different corpora of 7 panels on one stream, one
    workgroup each: the first call's unused tail prefetches and its
    leader's closing barrier must leave nothing behind for the second."""
    monkeypatch.setenv("NORNICDB_KNN_GRID", "1")
    db1, q, ref1 = _case(7, d)
    db2, _, ref2 = _case(7, d, corpus_seed=300 + d)
    s1, i1 = knn_search(db1, q, K)
    s2, i2 = knn_search(db2, q, K)
    _check_exact(s2, i2, ref2)
    _check_exact(s1, i1, ref1)
