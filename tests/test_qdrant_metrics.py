"""Qdrant collections score with the distance they were declared with
(REST and gRPC), keep it across a reopen, and the two Cypher
vector.similarity functions.

The three points tell the metrics apart for the query (1, 0):
a = (3, 3) wins under Dot (3), b = (0.1, 0) under Cosine (1),
c = (1, 0.5) under Euclid (distance 0.5, similarity 1 / 1.5).
"""

import grpc
import pytest
from fastapi.testclient import TestClient

from nornicdb_amd.cypher import Executor
from nornicdb_amd.db import open_db
from nornicdb_amd.embed import MockEmbedder
from nornicdb_amd.server import create_app
from nornicdb_amd.server import qdrant_grpc as qg
from nornicdb_amd.server.qdrant import QdrantRegistry
from nornicdb_amd.storage import MemoryEngine

QUERY = [1.0, 0.0]
POINTS = [(1, [3.0, 3.0]), (2, [0.1, 0.0]), (3, [1.0, 0.5])]   # a, b, c
# distance -> (winner id, its score, runner-up id)
WANT = {"Dot": (1, 3.0, 3), "Euclid": (3, 1 / 1.5, 2), "Cosine": (2, 1.0, 3)}


# ---------------------------------------------------------------------------
# REST
# ---------------------------------------------------------------------------
@pytest.fixture
def client():
    mgr = open_db(embedder=MockEmbedder(16), dims=16)
    with TestClient(create_app(mgr)) as c:
        yield c
    mgr.close()


def _rest_fill(c, name, distance):
    r = c.put(f"/collections/{name}",
              json={"vectors": {"size": 2, "distance": distance}})
    assert r.json()["status"] == "ok"
    r = c.put(f"/collections/{name}/points", json={"points": [
        {"id": i, "vector": v, "payload": {"n": i}} for i, v in POINTS]})
    assert r.json()["result"]["status"] == "completed"


@pytest.mark.parametrize("distance", ["Dot", "Euclid", "Cosine"])
def test_rest_search_scores_with_the_metric(client, distance):
    name = f"rest_{distance.lower()}"
    _rest_fill(client, name, distance)
    got = client.get(f"/collections/{name}").json()["result"]
    assert got["config"]["params"]["vectors"]["distance"] == distance
    res = client.post(f"/collections/{name}/points/search",
                      json={"vector": QUERY, "limit": 2,
                            "with_vector": True}).json()["result"]
    winner, score, second = WANT[distance]
    assert [h["id"] for h in res] == [winner, second]
    assert res[0]["score"] == pytest.approx(score)
    # vectors come back as they were sent, not normalised
    assert res[0]["vector"] == dict(POINTS)[winner]
    # the query endpoint ranks the same way
    res = client.post(f"/collections/{name}/points/query",
                      json={"query": QUERY, "limit": 1}).json()["result"]
    assert res["points"][0]["id"] == winner
    assert res["points"][0]["score"] == pytest.approx(score)


def test_rest_euclid_full_ranking(client):
    _rest_fill(client, "rest_euclid_all", "Euclid")
    res = client.post("/collections/rest_euclid_all/points/search",
                      json={"vector": QUERY, "limit": 3}).json()["result"]
    assert [h["id"] for h in res] == [3, 2, 1]
    assert [h["score"] for h in res] == pytest.approx(
        [1 / 1.5, 1 / 1.9, 1 / (1 + 13 ** 0.5)])


def test_rest_euclid_survives_reopen(tmp_path):
    d = str(tmp_path / "store")

    def client_of(mgr):
        app = create_app(mgr, auth=None)
        return TestClient(app.app if hasattr(app, "app") else app)

    mgr = open_db(d, embedder=MockEmbedder(8), dims=8)
    _rest_fill(client_of(mgr), "reopen_euclid", "Euclid")
    mgr.close()
    mgr2 = open_db(d, embedder=MockEmbedder(8), dims=8)
    c2 = client_of(mgr2)
    got = c2.get("/collections/reopen_euclid").json()["result"]
    assert got["config"]["params"]["vectors"]["distance"] == "Euclid"
    res = c2.post("/collections/reopen_euclid/points/search",
                  json={"vector": QUERY, "limit": 3}).json()["result"]
    assert [str(h["id"]) for h in res] == ["3", "2", "1"]
    assert res[0]["score"] == pytest.approx(1 / 1.5)
    mgr2.close()


def test_registry_rebuilt_on_its_engine_keeps_the_metric():
    eng = MemoryEngine()
    reg = QdrantRegistry(engine=eng)
    reg.create("rebuilt_euclid", 2, "Euclid")
    c = reg.get("rebuilt_euclid")
    for pid, vec in POINTS:
        c.vectors[str(pid)] = vec
        c.payloads[str(pid)] = {}
        c.index.add(str(pid), vec)
        c.persist_point(str(pid))
    reg2 = QdrantRegistry(engine=eng)
    c2 = reg2.get("rebuilt_euclid")
    assert c2.distance == "Euclid" and c2.index.metric == "euclidean"
    hits = c2.index.search(QUERY, 3)
    assert [p for p, _ in hits] == ["3", "2", "1"]
    assert hits[0][1] == pytest.approx(1 / 1.5)


def test_registry_device_default_and_manhattan():
    reg = QdrantRegistry()
    assert reg.device == "cpu"
    assert QdrantRegistry(device="cpu").device == "cpu"
    reg.create("dev_dot", 2, "Dot")
    idx = reg.get("dev_dot").index
    assert idx.device.type == "cpu" and idx.metric == "dot"
    # Manhattan is recorded as declared and scored as cosine, as before
    reg.create("dev_manhattan", 2, "Manhattan")
    c = reg.get("dev_manhattan")
    assert c.distance == "Manhattan" and c.index.metric == "cosine"
    with pytest.raises(ValueError):
        QdrantRegistry(device="tpu")


# ---------------------------------------------------------------------------
# gRPC
# ---------------------------------------------------------------------------
M = qg.M


@pytest.fixture
def served():
    server, port, svc = qg.serve(port=0)
    ch = grpc.insecure_channel(f"127.0.0.1:{port}")

    def call(service, method, req, resp_name):
        return qg.stub(ch, service, method, type(req), M[resp_name])(req)

    yield call
    ch.close()
    server.stop(0)


def _grpc_fill(call, name, distance):
    req = M["CreateCollection"](collection_name=name)
    req.vectors_config.params.size = 2
    req.vectors_config.params.distance = distance
    call("Collections", "Create", req, "CollectionOperationResponse")
    up = M["UpsertPoints"](collection_name=name)
    for pid, vec in POINTS:
        p = up.points.add()
        p.id.num = pid
        p.vectors.vector.data.extend(vec)
    call("Points", "Upsert", up, "PointsOperationResponse")


def _grpc_search(call, name, limit, threshold=None):
    sr = M["SearchPoints"](collection_name=name, limit=limit)
    sr.vector.extend(QUERY)
    if threshold is not None:
        sr.score_threshold = threshold
    return call("Points", "Search", sr, "SearchResponse").result


@pytest.mark.parametrize("num,distance", [(3, "Dot"), (2, "Euclid"),
                                          (1, "Cosine")])
def test_grpc_search_scores_with_the_metric(served, num, distance):
    name = f"grpc_{distance.lower()}"
    _grpc_fill(served, name, num)
    info = served("Collections", "Get",
                  M["GetCollectionInfoRequest"](collection_name=name),
                  "GetCollectionInfoResponse")
    assert info.result.config.params.vectors_config.params.distance == num
    res = _grpc_search(served, name, 2)
    winner, score, second = WANT[distance]
    assert [h.id.num for h in res] == [winner, second]
    assert res[0].score == pytest.approx(score)


def test_grpc_score_threshold_is_euclidean_similarity(served):
    _grpc_fill(served, "grpc_euclid_thr", 2)
    # similarities: c 0.667, b 0.526, a 0.217
    assert [h.id.num for h in _grpc_search(served, "grpc_euclid_thr", 3,
                                           threshold=0.5)] == [3, 2]
    assert [h.id.num for h in _grpc_search(served, "grpc_euclid_thr", 3,
                                           threshold=0.6)] == [3]
    assert len(_grpc_search(served, "grpc_euclid_thr", 3,
                            threshold=0.7)) == 0


# ---------------------------------------------------------------------------
# Cypher
# ---------------------------------------------------------------------------
def test_cypher_vector_similarity_functions():
    ex = Executor(MemoryEngine())
    r = ex.execute("RETURN vector.similarity.euclidean([0,0],[3,4]) AS s")
    assert r.rows[0][0] == pytest.approx(1 / 6)
    r = ex.execute("RETURN vector.similarity.cosine([1,0],[0,1]) AS s")
    assert r.rows[0][0] == pytest.approx(0.0)
    r = ex.execute("RETURN vector.similarity.cosine([1,2],[2,4]) AS s, "
                   "vector.similarity.euclidean([1.5,2],[1.5,2]) AS e")
    assert r.rows[0] == pytest.approx([1.0, 1.0])
    r = ex.execute("RETURN vector.similarity.cosine([1,0],[1,0,0]) AS a, "
                   "vector.similarity.euclidean([1,0],[1]) AS b, "
                   "vector.similarity.cosine(1, [1]) AS c, "
                   "vector.similarity.euclidean('x', null) AS d")
    assert r.rows[0] == [None, None, None, None]
