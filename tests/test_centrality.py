"""closeness_centrality / betweenness_centrality through the public
functions: the `device=` keyword and the threshold rule on the CPU, and under
the gpu mark the device route on graphs over the threshold, up to the apoc
procedure."""

import numpy as np
import pytest

from nornicdb_amd.graph import (algos, betweenness_centrality,
                                closeness_centrality, from_engine,
                                random_graph)

import centrality_cases as cc


@pytest.mark.parametrize("name", cc.CASES)
def test_device_keyword_on_the_cpu(name):
    g = cc.graph(name)
    assert closeness_centrality(g, device="cpu").tobytes() == \
        closeness_centrality(g).tobytes()
    assert closeness_centrality(g, [0, 3], device="cpu").tobytes() == \
        closeness_centrality(g, [0, 3]).tobytes()
    assert betweenness_centrality(g, device="cpu").tobytes() == \
        betweenness_centrality(g).tobytes()
    assert betweenness_centrality(g, samples=7, seed=3, device="cpu") \
        .tobytes() == betweenness_centrality(g, samples=7, seed=3).tobytes()


def test_small_graph_never_touches_the_extension(monkeypatch):
    def boom():
        raise AssertionError("native extension touched under the threshold")
    monkeypatch.setattr(algos, "native_or_none", boom)
    g = cc.graph("random")
    assert g.m < algos.GPU_MIN_EDGES
    assert closeness_centrality(g, range(5)).shape == (g.n,)
    assert betweenness_centrality(g, samples=3).shape == (g.n,)


def test_one_way_case_differs_from_its_transpose_everywhere():
    g = cc.graph("one_way")
    out = closeness_centrality(g, device="cpu")
    inn = closeness_centrality(cc.transposed(g), device="cpu")
    assert (out != inn).all()


def test_layered_reference_is_finite():
    ref = cc.betweenness_ref("layered", None)
    assert np.isfinite(ref).all() and ref.max() == 5040.0


# ------------------------------------------------------------------ device
_big = {}


def _over_threshold():
    if "g" not in _big:
        _big["g"] = random_graph(5000, 12, seed=2)
        assert _big["g"].m >= algos.GPU_MIN_EDGES
    return _big["g"]


@pytest.mark.gpu
def test_public_closeness_takes_the_device_route():
    g = _over_threshold()
    assert algos._use_gpu(g)
    got = closeness_centrality(g, nodes=range(70))
    ref = closeness_centrality(g, nodes=range(70), device="cpu")
    assert got.tobytes() == ref.tobytes()


@pytest.mark.gpu
def test_public_betweenness_takes_the_device_route():
    g = _over_threshold()
    got = betweenness_centrality(g, samples=4)
    ref = betweenness_centrality(g, samples=4, device="cpu")
    cc.check_betweenness(got, ref)


@pytest.mark.gpu
def test_apoc_closeness_procedure_on_the_device():
    """An engine-built graph over the threshold: 250 fan nodes with 200
    edges each into 250 sink nodes on a short chain, so that the CPU
    reference over all 500 nodes stays cheap (a BFS from a sink is tiny)."""
    from nornicdb_amd.db import NornicDB
    from nornicdb_amd.storage.memory import MemoryEngine
    from nornicdb_amd.storage.types import Edge, Node

    eng = MemoryEngine()
    db = NornicDB(eng, auto_embed=False)
    for i in range(500):
        db.engine.create_node(Node(id=f"n{i}", labels=["C"],
                                   properties={"name": f"n{i}"}))
    k = 0
    rng = np.random.default_rng(3)
    for i in range(250):
        for j in rng.permutation(250)[:200]:
            db.engine.create_edge(Edge(id=f"e{k}", type="R",
                                       start_node=f"n{i}",
                                       end_node=f"n{250 + int(j)}"))
            k += 1
    for j in range(250, 260):
        db.engine.create_edge(Edge(id=f"e{k}", type="R", start_node=f"n{j}",
                                   end_node=f"n{j + 1}"))
        k += 1
    g = from_engine(db.engine)
    assert g.m >= algos.GPU_MIN_EDGES and algos._use_gpu(g)
    ref = closeness_centrality(g, device="cpu")
    assert (ref > 0).sum() >= 250
    want = [[g.node_ids[i], float(ref[i])] for i in np.argsort(-ref)]
    rows = db.cypher("CALL apoc.algo.closenessCentrality() YIELD node, score "
                     "RETURN node.name, score").rows
    assert rows == want
