"""Filtered vector search above the kernels: EmbeddingIndex allow_ids and
tombstones, SearchService label filters, Qdrant REST filters and the
db.index.vector.queryNodes label filter."""

import numpy as np
import pytest
import torch

import nornicdb_amd.ops as ops_mod
import nornicdb_amd.search.pipeline as pipeline_mod
from nornicdb_amd.search.embedding_index import EmbeddingIndex
from nornicdb_amd.search.service import SearchService
from nornicdb_amd.storage import MemoryEngine
from nornicdb_amd.storage.types import Node

DIMS = 128     # D % 128 == 0: single-query searches run the gemv kernel on GPU
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


def _unit(x):
    x = np.asarray(x, dtype=np.float32)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _brute(idx, query, live_ids, k):
    """Exact top-k over the index's own stored values for the given ids."""
    q = torch.as_tensor(_unit(query), device=idx.device)
    q = q.to(idx.dtype).float()
    ids = list(live_ids)
    slots = torch.as_tensor([idx._id2slot[i] for i in ids], device=idx.device)
    scores = idx.matrix()[slots].float() @ q
    s, o = torch.topk(scores, min(k, len(ids)))
    return [ids[j] for j in o.tolist()], s.tolist()


# ---------------------------------------------------------------------------
# EmbeddingIndex
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
def test_index_allow_ids_far_from_query(device):
    rng = np.random.default_rng(0)
    query = _unit(rng.normal(size=DIMS))
    vecs = _unit(query + 0.5 * rng.normal(size=(300, DIMS)))
    far = [17, 95, 96, 200, 299]
    for j, r in enumerate(far):     # opposite side, distinct distances
        vecs[r] = _unit(-query + 0.1 * (j + 1) * rng.normal(size=DIMS))
    idx = EmbeddingIndex(DIMS, device=device, capacity=64)
    idx.add_batch([f"n{i}" for i in range(300)], vecs)
    allow = [f"n{r}" for r in far] + ["unknown-id"]
    hits = idx.search(query, 3, allow_ids=allow)
    want, want_s = _brute(idx, query, [f"n{r}" for r in far], 3)
    assert [h[0] for h in hits] == want
    assert np.allclose([h[1] for h in hits], want_s, atol=1e-2)
    # unfiltered, none of them is anywhere near the top
    assert not {h[0] for h in idx.search(query, 3)} & set(allow)
    # batch form, and fewer allowed ids than k
    both = idx.search_batch(np.stack([query, -query]), 10, allow_ids=allow)
    assert [h[0] for h in both[0]][:3] == want
    assert {h[0] for h in both[0]} == {h[0] for h in both[1]} == set(allow[:5])
    assert idx.search(query, 3, allow_ids=["unknown-id"]) == []


@pytest.mark.parametrize("device", DEVICES)
def test_index_tombstones_keep_k(device, monkeypatch):
    rng = np.random.default_rng(1)
    vecs = _unit(rng.normal(size=(300, DIMS)))
    query = vecs[7] + 0.3 * rng.normal(size=DIMS)
    ids = [f"n{i}" for i in range(300)]
    idx = EmbeddingIndex(DIMS, device=device)
    idx.add_batch(ids, vecs)
    # remove the 20 best hits, so every one of them would outrank a live row
    dead = [h[0] for h in idx.search(query, 20)]
    assert len(dead) == 20
    for d in dead:
        assert idx.remove(d)
    live = [i for i in ids if i not in set(dead)]

    asked = []
    real = ops_mod.knn_search

    def spy(db, q, k, *a, **kw):
        asked.append((k, kw.get("allow")))
        return real(db, q, k, *a, **kw)

    monkeypatch.setattr(ops_mod, "knn_search", spy)
    hits = idx.search(query, 10)
    assert [k for k, _ in asked] == [10]
    assert asked[0][1] is not None          # the live mask went to the kernel
    want, want_s = _brute(idx, query, live, 10)
    assert [h[0] for h in hits] == want
    assert np.allclose([h[1] for h in hits], want_s, atol=1e-2)

    # a re-added id becomes visible again
    idx.add(dead[0], vecs[int(dead[0][1:])])
    assert idx.search(query, 1)[0][0] == dead[0]
    # the live mask survives a _grow past the current capacity
    cap = idx._buf.shape[0]
    extra = _unit(rng.normal(size=(cap, DIMS)))
    idx.add_batch([f"x{i}" for i in range(cap)], extra)
    assert idx._buf.shape[0] > cap
    got = {h[0] for h in idx.search(query, 25)}
    assert not got & set(dead[1:])
    assert dead[0] in got
    want, _ = _brute(idx, query,
                     live + [dead[0]] + [f"x{i}" for i in range(cap)], 25)
    assert got == set(want)


def test_index_no_mask_without_tombstones_or_filter(monkeypatch):
    idx = EmbeddingIndex(16, device="cpu")
    idx.add_batch(["a", "b", "c"], np.eye(3, 16, dtype=np.float32))
    calls = []
    real = ops_mod.knn_search

    def spy(*a, **kw):
        calls.append((a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(ops_mod, "knn_search", spy)
    assert idx.search(np.eye(3, 16)[1], 2)[0][0] == "b"
    (args, kw), = calls
    # exactly the unfiltered call: (db, q, k), nothing else but allow=None
    assert len(args) == 3 and set(kw) <= {"allow"} and kw.get("allow") is None


# ---------------------------------------------------------------------------
# SearchService
# ---------------------------------------------------------------------------
def _rare_service(use_hnsw=True):
    rng = np.random.default_rng(2)
    query = _unit(rng.normal(size=32))
    eng = MemoryEngine()
    svc = SearchService(eng, dims=32, device="cpu", use_hnsw=use_hnsw)
    for i in range(98):
        v = _unit(query + 0.8 * rng.normal(size=32))
        eng.create_node(Node(id=f"c{i}", labels=["Common"],
                             embedding=v.tolist()))
    for j in range(2):     # the two farthest nodes of the store
        v = _unit(-query + 0.05 * (j + 1) * rng.normal(size=32))
        eng.create_node(Node(id=f"r{j}", labels=["Rare"],
                             embedding=v.tolist()))
    return eng, svc, query


def _ids(res):
    return [r.id for r in res]


def _check_rare(eng, svc, query):
    assert sorted(_ids(svc.vector_search(query, k=2, labels=["Rare"]))) == \
        ["r0", "r1"]
    # fewer matches than k
    assert sorted(_ids(svc.vector_search(query, k=5, labels=["Rare"]))) == \
        ["r0", "r1"]
    # hybrid search, vector leg only
    assert sorted(_ids(svc.search(query_vec=query, k=2, labels=["Rare"]))) == \
        ["r0", "r1"]
    # without labels: unchanged, the rare nodes are last
    assert not set(_ids(svc.vector_search(query, k=10))) & {"r0", "r1"}

    # a label change on update moves the node between sets
    n = eng.get_node("c0")
    n.labels = ["Rare"]
    eng.update_node(n)
    assert sorted(_ids(svc.vector_search(query, k=5, labels=["Rare"]))) == \
        ["c0", "r0", "r1"]
    assert "c0" not in _ids(svc.vector_search(query, k=98, labels=["Common"]))
    assert len(svc.vector_search(query, k=98, labels=["Common"])) == 97
    # union of two labels
    assert len(svc.vector_search(query, k=200,
                                 labels=["Common", "Rare"])) == 100
    # delete removes the node
    eng.delete_node("r0")
    assert sorted(_ids(svc.vector_search(query, k=5, labels=["Rare"]))) == \
        ["c0", "r1"]
    assert svc.vector_search(query, k=3, labels=["Nope"]) == []


def test_service_rare_label_brute_force():
    eng, svc, query = _rare_service()
    _check_rare(eng, svc, query)


def test_service_rare_label_hnsw_branch(monkeypatch):
    monkeypatch.setattr(pipeline_mod, "BRUTE_MAX", 10)
    eng, svc, query = _rare_service()
    assert len(svc.hnsw) == 100
    used = []
    real = svc.hnsw.search
    monkeypatch.setattr(svc.hnsw, "search",
                        lambda *a, **kw: used.append(1) or real(*a, **kw))
    _check_rare(eng, svc, query)
    assert used, "the HNSW branch did not run"


# ---------------------------------------------------------------------------
# Qdrant REST
# ---------------------------------------------------------------------------
@pytest.fixture
def qdrant():
    from fastapi.testclient import TestClient

    from nornicdb_amd.db import open_db
    from nornicdb_amd.embed import MockEmbedder
    from nornicdb_amd.server import create_app
    mgr = open_db(embedder=MockEmbedder(16), dims=16)
    with TestClient(create_app(mgr)) as c:
        rng = np.random.default_rng(3)
        query = _unit(rng.normal(size=8))
        c.put("/collections/places", json={"vectors": {"size": 8,
                                                       "distance": "Cosine"}})
        pts = []
        for i in range(50):
            if i in (4, 20, 41):
                v = _unit(-query + 0.05 * rng.normal(size=8))
                payload = {"city": "oslo"}
            else:
                v = _unit(query + 0.6 * rng.normal(size=8))
                payload = {"city": "bergen"}
            pts.append({"id": i, "vector": v.tolist(), "payload": payload})
        c.put("/collections/places/points", json={"points": pts})
        yield c, query.tolist()
    mgr.close()


OSLO = {"must": [{"key": "city", "match": {"value": "oslo"}}]}


def test_qdrant_search_honours_filter(qdrant):
    c, query = qdrant
    res = c.post("/collections/places/points/search", json={
        "vector": query, "limit": 3, "filter": OSLO}).json()["result"]
    assert sorted(p["id"] for p in res) == [4, 20, 41]
    assert all(p["payload"]["city"] == "oslo" for p in res)
    scores = [p["score"] for p in res]
    assert scores == sorted(scores, reverse=True)
    # without a filter: unchanged, the nearest points are not the oslo ones
    res = c.post("/collections/places/points/search", json={
        "vector": query, "limit": 3}).json()["result"]
    assert len(res) == 3
    assert not {p["id"] for p in res} & {4, 20, 41}
    scores = [p["score"] for p in res]
    assert scores == sorted(scores, reverse=True) and scores[0] > 0.5


def test_qdrant_query_honours_filter(qdrant):
    c, query = qdrant
    res = c.post("/collections/places/points/query", json={
        "query": query, "limit": 3, "filter": OSLO}).json()["result"]["points"]
    assert sorted(p["id"] for p in res) == [4, 20, 41]
    res = c.post("/collections/places/points/query", json={
        "query": query, "limit": 3}).json()["result"]["points"]
    assert len(res) == 3 and not {p["id"] for p in res} & {4, 20, 41}


def test_qdrant_grpc_search_selective_filter():
    """One matching point behind 11 nearer ones: limit*4 post-filtering
    never reached it."""
    import grpc

    from nornicdb_amd.server import qdrant_grpc as qg
    M = qg.M
    server, port, _ = qg.serve(port=0)
    ch = grpc.insecure_channel(f"127.0.0.1:{port}")
    try:
        def call(service, method, req, resp_name):
            return qg.stub(ch, service, method, type(req), M[resp_name])(req)

        req = M["CreateCollection"](collection_name="g")
        req.vectors_config.params.size = 4
        req.vectors_config.params.distance = 1
        call("Collections", "Create", req, "CollectionOperationResponse")
        up = M["UpsertPoints"](collection_name="g")
        for i in range(1, 13):
            p = up.points.add()
            p.id.num = i
            far = i == 7
            p.vectors.vector.data.extend(
                [-1, 0.1, 0, 0] if far else [1, 0.01 * i, 0, 0])
            p.payload["city"].string_value = "paris" if far else "berlin"
        call("Points", "Upsert", up, "PointsOperationResponse")
        sr = M["SearchPoints"](collection_name="g", limit=1)
        sr.vector.extend([1, 0, 0, 0])
        qg._payload_from_py(sr.filter.conditions.fields, {
            "must": [{"key": "city", "match": {"value": "paris"}}]})
        r = call("Points", "Search", sr, "SearchResponse")
        assert [h.id.num for h in r.result] == [7]
        sr = M["SearchPoints"](collection_name="g", limit=2)
        sr.vector.extend([1, 0, 0, 0])
        r = call("Points", "Search", sr, "SearchResponse")
        assert [h.id.num for h in r.result] == [1, 2]
    finally:
        ch.close()
        server.stop(0)


# ---------------------------------------------------------------------------
# db.index.vector.queryNodes
# ---------------------------------------------------------------------------
def test_query_nodes_filters_by_index_label():
    from nornicdb_amd.db import open_db
    from nornicdb_amd.embed import MockEmbedder
    mgr = open_db(embedder=MockEmbedder(32), dims=32)
    try:
        db = mgr.get()
        rng = np.random.default_rng(4)
        query = _unit(rng.normal(size=32))
        for i in range(40):
            v = _unit(query + 0.5 * rng.normal(size=32))
            db.engine.create_node(Node(id=f"o{i}", labels=["Other"],
                                       embedding=v.tolist()))
        for j in range(3):
            v = _unit(-query + 0.1 * rng.normal(size=32))
            db.engine.create_node(Node(id=f"p{j}", labels=["Paper"],
                                       embedding=v.tolist()))
        db.cypher("CALL db.index.vector.createNodeIndex("
                  "'paper_filtered_idx', 'Paper', 'embedding', 32, 'cosine')")
        call = ("CALL db.index.vector.queryNodes('%s', 3, $q) "
                "YIELD node, score RETURN node")
        rows = db.cypher(call % "paper_filtered_idx",
                         {"q": query.tolist()}).rows
        assert sorted(r[0].id for r in rows) == ["p0", "p1", "p2"]
        # an unknown index name searches unfiltered, as before
        rows = db.cypher(call % "no_such_idx", {"q": query.tolist()}).rows
        assert len(rows) == 3
        assert all(r[0].id.startswith("o") for r in rows)
    finally:
        mgr.close()
