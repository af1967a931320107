"""EmbeddingIndex metrics: cosine (as before), dot and euclidean.

Euclidean search ranks with the kNN kernels' inner product plus the per-row
bias -|x|^2/2 and re-scores the k hits exactly; scores are the reference's
EuclideanSimilarity, 1 / (1 + distance).
"""

import numpy as np
import pytest
import torch

from nornicdb_amd.search.embedding_index import EmbeddingIndex
from nornicdb_amd.search.ivf import IVFIndex
from nornicdb_amd.search.vectorspace import (COSINE, DOT, EUCLIDEAN,
                                             normalize_metric)

QUERY = [1.0, 0.0]
POINTS = {"a": [3.0, 3.0], "b": [0.1, 0.0], "c": [1.0, 0.5]}


def _three(metric):
    idx = EmbeddingIndex(2, device="cpu", metric=metric)
    idx.add_batch(list(POINTS), list(POINTS.values()))
    return idx


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_each_metric_has_its_winner():
    pid, score = _three("dot").search(QUERY, 1)[0]
    assert pid == "a" and score == pytest.approx(3.0)
    pid, score = _three("cosine").search(QUERY, 1)[0]
    assert pid == "b" and score == pytest.approx(1.0)
    pid, score = _three("euclidean").search(QUERY, 1)[0]
    assert pid == "c" and score == pytest.approx(1.0 / 1.5)
    # the default is cosine
    assert EmbeddingIndex(2, device="cpu").metric == COSINE


def test_euclidean_full_ranking_and_batch():
    idx = _three("Euclid")
    hits = idx.search(QUERY, 3)
    assert [p for p, _ in hits] == ["c", "b", "a"]
    want = [1 / 1.5, 1 / 1.9, 1 / (1 + np.sqrt(13.0))]
    assert [s for _, s in hits] == pytest.approx(want)
    both = idx.search_batch([QUERY, [3.0, 2.5]], 2)
    assert [p for p, _ in both[0]] == ["c", "b"]
    assert [p for p, _ in both[1]] == ["a", "c"]
    assert both[1][0][1] == pytest.approx(1 / 1.5)


def test_vectors_are_stored_as_given():
    for metric in ("dot", "euclidean"):
        idx = _three(metric)
        assert idx.get("a").tolist() == [3.0, 3.0]
        sub = dict(idx.score_subset(QUERY, ["a", "c"]))
        if metric == "dot":
            assert sub == pytest.approx({"a": 3.0, "c": 1.0})
        else:
            assert sub == pytest.approx({"a": 1 / (1 + np.sqrt(13.0)),
                                         "c": 1 / 1.5})
    # cosine still normalises
    assert _three("cosine").get("a").tolist() == pytest.approx(
        [2 ** -0.5, 2 ** -0.5])


def test_overwrite_refreshes_the_euclidean_bias():
    idx = _three("euclidean")
    assert idx.search(QUERY, 1)[0][0] == "c"
    idx.add("a", [1.0, 0.1])           # in place: same slot, new norm
    pid, score = idx.search(QUERY, 1)[0]
    assert pid == "a" and score == pytest.approx(1 / 1.1)
    idx.add_batch(["b"], [[1.0, 0.01]])
    pid, score = idx.search(QUERY, 1)[0]
    assert pid == "b" and score == pytest.approx(1 / 1.01)
    # the bias follows the rows through a capacity change
    small = EmbeddingIndex(2, device="cpu", capacity=2, metric="euclidean")
    small.add_batch(list(POINTS), list(POINTS.values()))
    small.add("d", [50.0, 50.0])
    assert [p for p, _ in small.search(QUERY, 4)] == ["c", "b", "a", "d"]


def test_remove_and_allow_ids_under_euclidean():
    idx = _three("euclidean")
    assert idx.remove("c")
    hits = idx.search(QUERY, 3)
    assert [p for p, _ in hits] == ["b", "a"]
    assert [p for p, _ in idx.search(QUERY, 3, allow_ids=["a"])] == ["a"]
    idx.add("c", POINTS["c"])
    assert [p for p, _ in idx.search(QUERY, 1, allow_ids=["a", "c"])] == ["c"]


def test_exact_duplicate_scores_one():
    rng = np.random.default_rng(0)
    mat = rng.normal(size=(50, 16)).astype(np.float32) * 3.0
    idx = EmbeddingIndex(16, device="cpu", metric="euclidean")
    idx.add_batch([f"p{i}" for i in range(50)], mat)
    for r in (0, 17, 49):
        pid, score = idx.search(mat[r], 1)[0]
        assert pid == f"p{r}" and score == 1.0


def test_quantised_or_ivf_need_cosine():
    with pytest.raises(ValueError):
        EmbeddingIndex(8, device="cpu", quant="int8", metric="dot")
    with pytest.raises(ValueError):
        EmbeddingIndex(8, device="cpu", quant="fp8", metric="euclidean")
    with pytest.raises(ValueError):
        IVFIndex(EmbeddingIndex(8, device="cpu", metric="euclidean"))
    IVFIndex(EmbeddingIndex(8, device="cpu"))       # cosine: as before


def test_normalize_metric():
    assert normalize_metric("Cosine") == COSINE == "cosine"
    assert normalize_metric("DOT") == DOT == "dot"
    for name in ("euclid", "Euclid", "EUCLIDEAN", "l2", "L2"):
        assert normalize_metric(name) == EUCLIDEAN == "euclidean"
    for bad in ("manhattan", "", "cos"):
        with pytest.raises(ValueError):
            normalize_metric(bad)
    with pytest.raises(ValueError):
        EmbeddingIndex(2, device="cpu", metric="manhattan")


# ---------------------------------------------------------------------------
# GPU: 700 x 128, norms 0.5..4, gemv (search) and MFMA (search_batch of 16)
# ---------------------------------------------------------------------------
N, D, K = 700, 128, 10
# tolerance of the MFMA bf16 route's scores (tests/test_ops_vector.py): an id
# is checked where the reference distances of its neighbours in the ranking
# differ from its own by more than this
ROUTE_TOL = 2e-2
RADII = [0.3, 0.45, 0.6, 0.75, 0.9]
PLANT = len(RADII)
_gpu = {}


def _gpu_case():
    if not _gpu:
        g = torch.Generator().manual_seed(42)
        rows = torch.nn.functional.normalize(torch.randn(N, D, generator=g),
                                             dim=-1)
        rows = rows * (0.5 + 3.5 * torch.rand(N, 1, generator=g))
        # queries of norm 1.5..2.5, each with PLANT rows planted around it
        # at the distances RADII (0.15 apart, far more than ROUTE_TOL), in
        # slots spread over the panels, both row groups and the tail. In 128
        # dimensions unrelated rows are sqrt(|q|^2 + |x|^2) > 1.5 away and
        # nearly equidistant: without the planted rows hardly any id would
        # be distinct enough to check. Planted norms stay within 0.6..3.4.
        q = torch.nn.functional.normalize(torch.randn(16, D, generator=g),
                                          dim=-1)
        q = q * (1.5 + torch.rand(16, 1, generator=g))
        slots = torch.randperm(N, generator=g)[:16 * PLANT].view(16, PLANT)
        slots[0, 0], slots[1, 0], slots[2, 0] = 0, 319, N - 1
        u = torch.nn.functional.normalize(
            torch.randn(16, PLANT, D, generator=g), dim=-1)
        rows[slots] = q[:, None, :] + u * torch.tensor(RADII)[None, :, None]
        idx = EmbeddingIndex(D, device="cuda", metric="euclidean")
        idx.add_batch([str(i) for i in range(N)], rows.numpy())
        stored = rows.to(torch.bfloat16).float()        # what the index holds
        # fp32 reference distances on the stored values, without the
        # |a|^2 + |b|^2 - 2ab shortcut
        dist = torch.cdist(q, stored,
                           compute_mode="donot_use_mm_for_euclid_dist")
        _gpu.update(idx=idx, q=q, dist=dist)
    return _gpu["idx"], _gpu["q"], _gpu["dist"]


def _check_hits(hits, dist_row):
    assert len(hits) == K
    ids = [int(p) for p, _ in hits]
    got = torch.tensor([1.0 / s - 1.0 for _, s in hits], dtype=torch.float64)
    assert len(set(ids)) == K
    scores = [s for _, s in hits]
    assert scores == sorted(scores, reverse=True)
    ref_d, ref_i = torch.topk(dist_row, K + 1, largest=False)
    checked = 0
    for r in range(K):
        lo_ok = r == 0 or ref_d[r] - ref_d[r - 1] > ROUTE_TOL
        hi_ok = ref_d[r + 1] - ref_d[r] > ROUTE_TOL
        if lo_ok and hi_ok:
            checked += 1
            assert ids[r] == int(ref_i[r]), (r, ids, ref_i.tolist())
    # every returned distance is that row's own fp32 distance, within the
    # fp32 bound of a D-term sum
    own = dist_row[ids].double()
    rel = ((got - own).abs() / own).max().item()
    print(f"ids checked {checked}/{K}, max rel distance err {rel:.3e}")
    assert rel <= D * 2.0 ** -23, rel
    return checked


@pytest.mark.gpu
def test_gpu_euclidean_search_gemv():
    idx, q, dist = _gpu_case()
    checked = sum(_check_hits(idx.search(q[r].numpy(), K), dist[r])
                  for r in (0, 3, 7, 12))
    assert checked >= 4 * (PLANT - 1)    # most planted rows at the least


@pytest.mark.gpu
def test_gpu_euclidean_search_batch_mfma():
    idx, q, dist = _gpu_case()
    outs = idx.search_batch(q.numpy(), K)
    assert len(outs) == 16
    checked = sum(_check_hits(outs[r], dist[r]) for r in range(16))
    assert checked >= 16 * (PLANT - 1)
