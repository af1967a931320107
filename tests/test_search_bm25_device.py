"""The opt-in device full-text index behind SearchService: text_search and
the full-text leg of hybrid search, storage events and maintenance."""

import numpy as np
import pytest

from nornicdb_amd.search import SearchService
from nornicdb_amd.search.bm25_device import DeviceFulltextIndex
from nornicdb_amd.storage.memory import MemoryEngine
from nornicdb_amd.storage.types import Node

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
N = 120
DIMS = 8
QUERIES = ["alpha", "alpha beta", "beta gamma gamma", "fill3 alpha"]


def _content(i):
    """Every document has its own length, so no two BM25 scores tie."""
    words = ["alpha"] * (1 + i % 3) + ["beta"] * (i % 2) + \
        ["gamma"] * (i % 5 == 0)
    return " ".join(words + [f"fill{j % 17}" for j in range(i + 2)])


def _service(device, **kw):
    rng = np.random.default_rng(3)
    eng = MemoryEngine()
    svc = SearchService(eng, dims=DIMS, device=device, use_hnsw=False, **kw)
    vecs = rng.normal(size=(N, DIMS)).astype(np.float32)
    for i in range(N):
        eng.create_node(Node(id=f"n{i}",
                             labels=["Even" if i % 2 == 0 else "Odd"],
                             properties={"content": _content(i)},
                             embedding=vecs[i].tolist()))
    return eng, svc, vecs


def _ids(results):
    return [r.id for r in results]


def _same_answers(on, off, vecs):
    for query in QUERIES:
        ref = off.text_search(query, k=40)
        scores = [r.score for r in ref]
        assert len(set(scores)) == len(scores) > 5, "corpus must not tie"
        got = on.text_search(query, k=40)
        assert _ids(got) == _ids(ref)
        assert [r.score for r in got] == pytest.approx(scores, rel=1e-5)
        assert all(r.source == "fulltext" for r in got)
        assert _ids(on.text_search(query, k=7, labels=["Odd"])) == \
            _ids(off.text_search(query, k=7, labels=["Odd"]))
        for kw in ({}, {"labels": ["Even"]}, {"mmr": True}):
            assert _ids(on.search(query, query_vec=vecs[4], k=10, **kw)) == \
                _ids(off.search(query, query_vec=vecs[4], k=10, **kw))
        assert _ids(on.search(query, k=10)) == _ids(off.search(query, k=10))


def test_option_off_is_the_default(monkeypatch):
    monkeypatch.delenv("NORNICDB_SEARCH_FULLTEXT_GPU", raising=False)
    svc = SearchService(MemoryEngine(), dims=DIMS, device="cpu")
    assert svc.fulltext_dev is None
    svc = SearchService(MemoryEngine(), dims=DIMS, device="cpu",
                        fulltext_gpu=False)
    assert svc.fulltext_dev is None
    svc.build_indexes()
    svc.recluster()


def test_environment_variable_enables_the_option(monkeypatch):
    monkeypatch.setenv("NORNICDB_SEARCH_FULLTEXT_GPU", "1")
    svc = SearchService(MemoryEngine(), dims=DIMS, device="cpu")
    assert isinstance(svc.fulltext_dev, DeviceFulltextIndex)
    assert svc.fulltext_dev.ft is svc.fulltext
    monkeypatch.setenv("NORNICDB_SEARCH_FULLTEXT_GPU", "0")
    assert SearchService(MemoryEngine(), dims=DIMS,
                         device="cpu").fulltext_dev is None


@pytest.mark.parametrize("device", DEVICES)
def test_service_answers_as_with_the_option_off(monkeypatch, device):
    monkeypatch.delenv("NORNICDB_SEARCH_FULLTEXT_GPU", raising=False)
    _, off, vecs = _service(device)
    eng, on, _ = _service(device, fulltext_gpu=True)
    dev = on.fulltext_dev
    assert dev.device.type == device
    # unbuilt: the host index answers
    assert not dev.built
    _same_answers(on, off, vecs)
    on.build_indexes()
    assert dev.built and dev.n_built == N and dev.tail == 0
    _same_answers(on, off, vecs)


@pytest.mark.parametrize("device", DEVICES)
def test_index_follows_storage_events_and_recluster_rebuilds(monkeypatch,
                                                             device):
    monkeypatch.delenv("NORNICDB_SEARCH_FULLTEXT_GPU", raising=False)
    eng_off, off, vecs = _service(device)
    eng_on, on, _ = _service(device, fulltext_gpu=True)
    on.build_indexes()
    dev = on.fulltext_dev

    def both(fn):
        fn(eng_off)
        fn(eng_on)

    both(lambda e: e.create_node(Node(
        id="late", labels=["Odd"],
        properties={"content": "alpha alpha beta gamma zulu"},
        embedding=vecs[0].tolist())))
    assert dev.tail == 1
    assert _ids(on.text_search("zulu")) == ["late"]
    both(lambda e: e.update_node(Node(
        id="n10", labels=["Even"],
        properties={"content": "gamma gamma gamma beta"},
        embedding=vecs[10].tolist())))
    both(lambda e: e.delete_node("n20"))
    assert dev.stale == 2 and dev.tail == 2
    assert "n20" not in _ids(on.text_search("alpha", k=200))
    assert "n10" not in _ids(on.text_search("alpha", k=200))
    assert "n10" in _ids(on.text_search("gamma", k=5))
    _same_answers(on, off, vecs)

    # below the ratio recluster() leaves the frozen postings alone
    on.recluster(k=4)
    assert dev.stale == 2 and dev.tail == 2
    for i in range(N // 5):
        both(lambda e: e.create_node(Node(
            id=f"x{i}", labels=["Odd"],
            properties={"content": _content(N + 7 * i)})))
    assert dev.needs_rebuild()
    on.recluster(k=4)
    off.recluster(k=4)
    assert not dev.needs_rebuild()
    assert dev.tail == 0 and dev.stale == 0
    assert dev.n_built == len(on.fulltext)
    _same_answers(on, off, vecs)
