"""IVFIndex over an EmbeddingIndex, and its opt-in wiring into the vector
pipeline, SearchService and the HTTP search route."""

import numpy as np
import pytest
import torch

from nornicdb_amd.search import (EmbeddingIndex, IVFIndex, SearchService,
                                 VectorSearchPipeline)
from nornicdb_amd.search import ivf as ivf_mod
from nornicdb_amd.search import pipeline as pipeline_mod
from nornicdb_amd.storage.memory import MemoryEngine
from nornicdb_amd.storage.types import Node


def _unit(v):
    v = np.asarray(v, dtype=np.float32)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _filled(n=2000, d=64, seed=0, device="cpu"):
    rng = np.random.default_rng(seed)
    centres = _unit(rng.normal(size=(16, d)))
    mat = _unit(centres[rng.integers(0, 16, n)] + 0.15 * rng.normal(size=(n, d)))
    emb = EmbeddingIndex(d, device=device)
    ids = [f"v{i}" for i in range(n)]
    emb.add_batch(ids, mat)
    return emb, ids, mat, rng


def _built(**kw):
    emb, ids, mat, rng = _filled(**kw)
    ivf = IVFIndex(emb)
    ivf.build(n_lists=16)
    return emb, ivf, ids, mat, rng


# ---------------------------------------------------------------------------
# IVFIndex on a CPU EmbeddingIndex
# ---------------------------------------------------------------------------
def test_properties_and_unbuilt_delegates():
    emb, ids, mat, _ = _filled(n=300)
    ivf = IVFIndex(emb)
    assert not ivf.built and ivf.n_lists == 0 and ivf.nprobe == 8
    assert ivf.tail == 0 and ivf.stale == 0 and not ivf.needs_rebuild()
    assert ivf.search(mat[3], 5) == emb.search(mat[3], 5)
    assert ivf.search_batch(mat[:2], 5) == emb.search_batch(mat[:2], 5)
    ivf.build()
    assert ivf.built and ivf.n_lists == 12           # optimal_k(300)
    assert ivf.n_built == 300 and ivf._lock is emb._lock


def test_all_lists_equals_brute_force():
    emb, ivf, ids, mat, _ = _built()
    q = mat[:5] + 0.01
    for nprobe in (16, 50):                          # >= n_lists: delegates
        assert ivf.search(q[0], 10, nprobe=nprobe) == emb.search(q[0], 10)
        assert ivf.search_batch(q, 10, nprobe=nprobe) == \
            emb.search_batch(q, 10)
    # one list short of all of them: the IVF path itself; a query that is a
    # stored row finds that row first, with the brute-force score
    hits = ivf.search(mat[7], 10, nprobe=15)
    ref = emb.search(mat[7], 10)
    assert hits[0][0] == "v7" and hits[0][1] == pytest.approx(ref[0][1])
    assert len(hits) == 10
    assert [s for _, s in hits] == sorted((s for _, s in hits), reverse=True)


def test_ivf_path_matches_exact_search_of_probed_lists():
    emb, ivf, ids, mat, _ = _built()
    q = _unit(mat[11] + 0.02)
    hits = ivf.search(q, 10, nprobe=4)
    batch = ivf.search_batch(np.stack([q, mat[5]]), 10, nprobe=4)
    assert [i for i, _ in batch[0]] == [i for i, _ in hits]
    assert [s for _, s in batch[0]] == pytest.approx([s for _, s in hits],
                                                     abs=1e-6)
    # every hit's score is its exact inner product
    for id_, s in hits:
        assert s == pytest.approx(float(mat[int(id_[1:])] @ q), abs=1e-5)
    # recall against brute force on this clustered corpus
    ref = {i for i, _ in emb.search(q, 10)}
    assert len(ref & {i for i, _ in hits}) >= 9


def test_tail_removed_allow_and_stale():
    emb, ivf, ids, mat, rng = _built()
    n = len(ids)
    q = _unit(rng.normal(size=64))

    # an id added after build() is found through the tail, far from any
    # probed list or not
    emb.add("new", q)
    assert ivf.tail == 1 and ivf.stale == 0
    hits = ivf.search(q, 5, nprobe=1)
    assert hits[0][0] == "new" and hits[0][1] == pytest.approx(1.0, abs=1e-5)

    # a removed id is never returned and does not widen k
    emb.remove("new")
    hits = ivf.search(q, 5, nprobe=1)
    assert "new" not in [i for i, _ in hits] and len(hits) == 5
    top = ivf.search(mat[20], 3, nprobe=2)
    assert top[0][0] == "v20"
    emb.remove("v20")
    top2 = ivf.search(mat[20], 3, nprobe=2)
    assert "v20" not in [i for i, _ in top2] and len(top2) == 3
    assert [i for i, _ in top2][:2] == [i for i, _ in top[1:]]

    # allow_ids is honoured (and ANDed with the live mask)
    allowed = [f"v{i}" for i in range(0, n, 3)] + ["v20", "ghost"]
    got = ivf.search(mat[21], 10, nprobe=4, allow_ids=allowed)
    assert got and {i for i, _ in got} <= set(allowed) - {"v20", "ghost"}
    ref = [h for h in ivf.search(mat[21], 400, nprobe=4)
           if h[0] in set(allowed)][:10]
    assert [i for i, _ in got] == [i for i, _ in ref]

    # re-adding an existing id with a new vector: stays in its old list,
    # scored with the new vector, counted as stale
    assert ivf.stale == 0
    target = ivf.search(mat[30], 1, nprobe=1)[0][0]
    assert target == "v30"
    new_vec = _unit(mat[30] + 0.05 * rng.normal(size=64))
    emb.add("v30", new_vec)
    assert ivf.stale == 1
    emb.add("v30", new_vec)                           # same slot again
    assert ivf.stale == 1
    hit = dict(ivf.search(new_vec, 3, nprobe=1))
    assert hit["v30"] == pytest.approx(1.0, abs=1e-5)
    emb.add_batch(["v31", "fresh"], np.stack([mat[31], q]))
    assert ivf.stale == 2 and ivf.tail == 2           # "new" slot + "fresh"

    ivf.build(n_lists=16)                             # rebuild clears both
    assert ivf.stale == 0 and ivf.tail == 0
    assert ivf.n_built == emb._n
    # dead slots are in no list
    listed = set(ivf._lists.list_rows.tolist())
    assert not listed & emb._dead and len(listed) == len(emb)


def test_needs_rebuild_flips_at_ratio():
    emb, ivf, ids, mat, rng = _built(n=100, d=16)
    assert ivf.n_built == 100 and not ivf.needs_rebuild()
    for j in range(10):                               # 10 tail
        emb.add(f"t{j}", rng.normal(size=16))
    for j in range(10):                               # 10 stale
        emb.add(f"v{j}", rng.normal(size=16))
    assert ivf.tail + ivf.stale == 20
    assert not ivf.needs_rebuild()                    # 20 == 0.2 * 100
    emb.add("v50", rng.normal(size=16))
    assert ivf.needs_rebuild()                        # 21 > 20


def test_build_skips_dead_slots_and_empty_index():
    emb = EmbeddingIndex(8, device="cpu")
    ivf = IVFIndex(emb)
    ivf.build()
    assert not ivf.built
    assert ivf.search(np.ones(8), 3) == []
    emb.add_batch([f"a{i}" for i in range(50)],
                  np.random.default_rng(0).normal(size=(50, 8)))
    emb.remove("a3")
    ivf.build(n_lists=4)
    assert 3 not in ivf._lists.list_rows.tolist()
    assert ivf._lists.list_rows.numel() == 49
    assert all(i != "a3" for i, _ in ivf.search(emb.get("a4"), 49, nprobe=3))


# ---------------------------------------------------------------------------
# Pipeline and service wiring
# ---------------------------------------------------------------------------
def _forbid_ivf(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("IVF path taken")
    monkeypatch.setattr(ivf_mod.IVFIndex, "search", boom)
    monkeypatch.setattr(ivf_mod.IVFIndex, "build", boom)


def test_pipeline_without_ivf_is_unchanged(monkeypatch):
    emb, ivf, ids, mat, _ = _built(n=400)
    _forbid_ivf(monkeypatch)
    pipe = VectorSearchPipeline(emb)
    assert pipe.ivf is None
    assert pipe.search(mat[3], 5) == emb.search(mat[3], 5)
    assert pipe.search(mat[3], 5, nprobe=2) == emb.search(mat[3], 5)
    # an IVFIndex that is not built, or a small corpus without nprobe
    assert VectorSearchPipeline(emb, ivf=IVFIndex(emb)) \
        .search(mat[3], 5, nprobe=2) == emb.search(mat[3], 5)
    assert VectorSearchPipeline(emb, ivf=ivf).search(mat[3], 5) == \
        emb.search(mat[3], 5)


def test_pipeline_routes_to_ivf(monkeypatch):
    emb, ivf, ids, mat, _ = _built(n=400)
    calls = []
    real = ivf_mod.IVFIndex.search

    def spy(self, query, k, nprobe=None, allow_ids=None):
        calls.append((k, nprobe, allow_ids))
        return real(self, query, k, nprobe=nprobe, allow_ids=allow_ids)

    monkeypatch.setattr(ivf_mod.IVFIndex, "search", spy)
    pipe = VectorSearchPipeline(emb, ivf=ivf)
    hits = pipe.search(mat[9], 5, nprobe=3)
    assert calls == [(5, 3, None)] and hits[0][0] == "v9"
    pipe.search(mat[9], 5, allow_ids=["v1", "v2"], nprobe=3)
    assert calls[-1] == (5, 3, {"v1", "v2"})
    # above KMEANS_MIN no nprobe is needed
    monkeypatch.setattr(pipeline_mod, "KMEANS_MIN", 100)
    pipe.search(mat[9], 4)
    assert calls[-1] == (4, None, None)


def _service(ivf=None, n=300, dims=32):
    rng = np.random.default_rng(4)
    eng = MemoryEngine()
    kw = {} if ivf is None else {"ivf": ivf}
    svc = SearchService(eng, dims=dims, device="cpu", use_hnsw=False, **kw)
    vecs = _unit(rng.normal(size=(n, dims)))
    for i in range(n):
        eng.create_node(Node(id=f"n{i}", labels=["Even" if i % 2 == 0
                                                 else "Odd"],
                             properties={"title": f"doc {i}"},
                             embedding=vecs[i].tolist()))
    return eng, svc, vecs


def test_service_flag_off_is_unchanged(monkeypatch):
    monkeypatch.delenv("NORNICDB_SEARCH_IVF", raising=False)
    _forbid_ivf(monkeypatch)
    eng, svc, vecs = _service()
    assert svc.ivf is None and svc.pipeline.ivf is None
    svc.recluster()
    ref = svc.emb.search(vecs[5], 4)
    for res in (svc.vector_search(vecs[5], k=4),
                svc.vector_search(vecs[5], k=4, nprobe=2),
                svc.search(query_vec=vecs[5], k=4, nprobe=2)):
        assert [(r.id, r.score) for r in res] == ref
    assert SearchService(MemoryEngine(), dims=8, device="cpu",
                         ivf=False).ivf is None


@pytest.mark.parametrize("how", ["arg", "env"])
def test_service_flag_on_uses_ivf(monkeypatch, how):
    if how == "env":
        monkeypatch.setenv("NORNICDB_SEARCH_IVF", "1")
        eng, svc, vecs = _service()
    else:
        monkeypatch.delenv("NORNICDB_SEARCH_IVF", raising=False)
        eng, svc, vecs = _service(ivf=True)
    assert isinstance(svc.ivf, IVFIndex) and svc.pipeline.ivf is svc.ivf
    assert not svc.ivf.built
    # not built yet: brute force, nprobe or not
    assert svc.vector_search(vecs[5], k=3, nprobe=2)[0].id == "n5"
    svc.recluster(k=10)
    assert svc.ivf.built and svc.ivf.n_lists == 10
    assert svc.clusters.k == 10

    seen = []
    real = ivf_mod.ivf_search

    def spy(*a, **kw):
        seen.append(a[4].shape)                       # probes
        return real(*a, **kw)

    monkeypatch.setattr(ivf_mod, "ivf_search", spy)
    res = svc.vector_search(vecs[5], k=3, nprobe=2)
    assert seen == [(1, 2)] and res[0].id == "n5" and res[0].source == "vector"
    res = svc.vector_search(vecs[6], k=3, labels=["Even"], nprobe=3)
    assert seen[-1] == (1, 3) and res[0].id == "n6"
    assert all(int(r.id[1:]) % 2 == 0 for r in res)
    # hybrid search over-fetches max(4k, 40) through the same path
    res = svc.search(query_vec=vecs[7], k=3, nprobe=2)
    assert seen[-1] == (1, 2) and res[0].id == "n7"
    # small corpus and no nprobe: today's path
    n_calls = len(seen)
    assert svc.vector_search(vecs[5], k=3)[0].id == "n5"
    assert len(seen) == n_calls
    # deletes reach the IVF path through the shared live mask
    eng.delete_node("n5")
    assert "n5" not in [r.id for r in svc.vector_search(vecs[5], k=3,
                                                        nprobe=2)]


def test_http_nprobe_roundtrip(monkeypatch):
    from fastapi.testclient import TestClient

    from nornicdb_amd.db import open_db
    from nornicdb_amd.embed import MockEmbedder
    from nornicdb_amd.server import create_app

    monkeypatch.setenv("NORNICDB_SEARCH_IVF", "1")
    mgr = open_db(embedder=MockEmbedder(32), dims=32)
    try:
        with TestClient(create_app(mgr)) as client:
            for i in range(40):
                client.post("/nornicdb/store",
                            json={"content": f"note number {i} about item {i}",
                                  "title": f"t{i}"})
            rid = client.post("/nornicdb/store", json={
                "content": "the quick brown fox", "title": "fox"}).json()["id"]
            db = mgr.get()
            db.embed_queue.drain()
            assert db.search.ivf is not None
            db.search.recluster(k=6)
            assert db.search.ivf.built

            seen = []
            real = db.search.pipeline.search

            def spy(query, k, allow_ids=None, nprobe=None):
                seen.append(nprobe)
                return real(query, k, allow_ids=allow_ids, nprobe=nprobe)

            monkeypatch.setattr(db.search.pipeline, "search", spy)
            res = client.post("/nornicdb/search", json={
                "query": "quick brown fox", "nprobe": 2}).json()["results"]
            assert seen == [2] and res and res[0]["id"] == rid
            res = client.post("/nornicdb/search", json={
                "query": "quick brown fox"}).json()["results"]
            assert seen == [2, None] and res[0]["id"] == rid
            assert client.post("/nornicdb/search", json={
                "query": "fox", "nprobe": "many"}).status_code == 422
    finally:
        mgr.close()


# ---------------------------------------------------------------------------
# GPU: IVFIndex end to end over the fused kernel
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_ivf_index_end_to_end():
    from test_ivf import clustered

    x, q = clustered(0, 128)
    emb = EmbeddingIndex(128, device="cuda")
    ids = [f"v{i}" for i in range(x.shape[0])]
    emb.add_batch(ids, x.numpy())
    ivf = IVFIndex(emb)
    ivf.build(n_lists=32)
    assert ivf.built and ivf.n_lists == 32 and ivf.n_built == 4096
    assert ivf._lists.list_rows.is_cuda

    qn = q.numpy()
    assert ivf.search(qn[0], 10, nprobe=32) == emb.search(qn[0], 10)
    assert ivf.search_batch(qn[:4], 10, nprobe=32) == \
        emb.search_batch(qn[:4], 10)

    # recall floor at nprobe=4 against brute force, single and batched
    ref = emb.search_batch(qn, 10)
    got = ivf.search_batch(qn, 10, nprobe=4)
    hit = sum(len({i for i, _ in a} & {i for i, _ in b})
              for a, b in zip(got, ref))
    print(f"recall@10 at nprobe=4: {hit / 640:.4f}")
    assert hit / 640 >= 0.95
    one = ivf.search(qn[3], 10, nprobe=4)
    assert [i for i, _ in one] == [i for i, _ in got[3]]
    # hybrid search's over-fetch size runs on the K=64 kernel
    wide = ivf.search(qn[3], 40, nprobe=4)
    assert len(wide) == 40 and [i for i, _ in wide[:10]] == \
        [i for i, _ in one]

    # add -> tail, remove -> masked, overwrite -> stale
    fresh = np.zeros(128, dtype=np.float32)
    fresh[5] = 1.0
    emb.add("fresh", fresh)
    hits = ivf.search(fresh, 3, nprobe=1)
    assert hits[0][0] == "fresh" and hits[0][1] == pytest.approx(1.0, abs=1e-2)
    emb.remove("fresh")
    assert "fresh" not in [i for i, _ in ivf.search(fresh, 3, nprobe=1)]
    top = ivf.search(x[40].numpy(), 3, nprobe=2)
    assert top[0][0] == "v40"
    emb.remove("v40")
    assert "v40" not in [i for i, _ in ivf.search(x[40].numpy(), 3, nprobe=2)]
    got = ivf.search(x[41].numpy(), 5, nprobe=4,
                     allow_ids=[f"v{i}" for i in range(1, 4096, 2)])
    assert got[0][0] == "v41" and all(int(i[1:]) % 2 == 1 for i, _ in got)
    emb.add("v50", fresh)
    assert ivf.stale == 1 and ivf.tail == 1
    hit = dict(ivf.search(x[50].numpy(), 5, nprobe=2))
    assert "v50" not in hit or hit["v50"] < 0.9
