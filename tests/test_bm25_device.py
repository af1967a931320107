"""DeviceFulltextIndex against the host FulltextIndex it follows, on CPU
tensors and, under the gpu mark, the same cases on the device."""

import random

import pytest

from nornicdb_amd.search.bm25 import FulltextIndex, tokenize
from nornicdb_amd.search.bm25_device import DeviceFulltextIndex

from bm25_cases import tolerance

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
WORDS = [f"w{j:02d}" for j in range(60)]
N_DOCS = 300
QUERIES = ["w00", "w01 w02", "w03 w03 w10", "w59", "w20 w21 w22 w23 w24",
           "w05 nosuchword", "nosuchword", "w07 w07 w07 w08"]


def _text(rng, lo=3, hi=14):
    # Zipf-like: low-numbered words are common
    return " ".join(WORDS[min(59, int(rng.paretovariate(0.7)) - 1)]
                    for _ in range(rng.randint(lo, hi)))


def _index(device):
    rng = random.Random(7)
    ft = FulltextIndex()
    for d in range(N_DOCS):
        ft.index(f"d{d}", _text(rng))
    ft.index("d5", "uniqold w00 w01")
    return ft, DeviceFulltextIndex(ft, device=device), rng


def _compare(ft, dev, queries=QUERIES, ks=(1, 10, 40), allow_ids=None):
    """The contract of tests/bm25_cases.py on (id, score) lists, with
    FulltextIndex.search as the reference."""
    for query in queries:
        ref = dict(ft.search(query, len(ft) + 1))
        if allow_ids is not None:
            ref = {d: s for d, s in ref.items() if d in allow_ids}
        top = sorted(ref.values(), reverse=True)
        t_count = len(set(tokenize(query)))
        tol = tolerance(t_count, top[0]) if top else 0.0
        for k in ks:
            hits = dev.search(query, k, allow_ids=allow_ids)
            assert len(hits) == min(k, len(ref)), (query, k, hits)
            ids = [d for d, _ in hits]
            assert len(set(ids)) == len(ids), "duplicate hit"
            scores = [s for _, s in hits]
            assert scores == sorted(scores, reverse=True)
            for j, (d, s) in enumerate(hits):
                assert d in ref, (query, d)
                assert abs(s - top[j]) <= tol, (query, j, s, top[j])
                assert abs(ref[d] - s) <= tol, (query, d, s, ref[d])
        batch = dev.search_batch([query, "w00 w01"], 10, allow_ids=allow_ids)
        assert len(batch) == 2
        assert [s for _, s in batch[0]] == \
            [s for _, s in dev.search(query, 10, allow_ids=allow_ids)]


@pytest.mark.parametrize("device", DEVICES)
def test_unbuilt_index_delegates_to_the_host(device):
    ft, dev, _ = _index(device)
    assert not dev.built and not dev.needs_rebuild()
    assert dev.tail == 0 and dev.stale == 0
    for query in QUERIES:
        assert dev.search(query, 10) == ft.search(query, 10)
    empty = DeviceFulltextIndex(FulltextIndex(), device=device)
    empty.build()
    assert not empty.built and empty.search("w00", 5) == []


@pytest.mark.parametrize("device", DEVICES)
def test_built_index_matches_the_host(device):
    ft, dev, _ = _index(device)
    dev.build()
    assert dev.built and dev.n_built == len(ft)
    assert dev.tail == 0 and dev.stale == 0
    _compare(ft, dev)
    _compare(ft, dev, ks=(70,))    # past the kernel's k


@pytest.mark.parametrize("device", DEVICES)
def test_index_follows_changes_without_a_rebuild(device):
    ft, dev, rng = _index(device)
    dev.build()
    n_built = dev.n_built

    # new documents land in the tail and are findable
    for d in range(5):
        ft.index(f"new{d}", _text(rng) + " w59 w00")
    assert dev.tail == 5 and dev.stale == 0
    assert {"new0", "new4"} <= {d for d, _ in dev.search("w59 w00", 400)}
    _compare(ft, dev)

    # a frozen document re-indexed with different text: the old text must
    # not score, the new text must
    assert [d for d, _ in dev.search("uniqold", 5)] == ["d5"]
    ft.index("d5", "uniqnew w02 w02 w03")
    assert dev.stale == 1 and dev.tail == 6
    assert dev.search("uniqold", 5) == []
    assert "d5" not in {d for d, _ in dev.search("w00", 400)}
    assert [d for d, _ in dev.search("uniqnew", 5)] == ["d5"]
    _compare(ft, dev, QUERIES + ["uniqnew w02", "uniqold"])

    # a frozen and a tail document removed
    ft.remove("d7")
    ft.remove("new1")
    assert dev.stale == 2 and dev.tail == 5
    for query in ("w00", "w59 w00"):
        got = {d for d, _ in dev.search(query, 400)}
        assert "d7" not in got and "new1" not in got
    _compare(ft, dev)

    # a term the frozen vocabulary lacks
    ft.index("fresh", "zebra w00 zebra")
    assert [d for d, _ in dev.search("zebra", 5)] == ["fresh"]
    _compare(ft, dev, QUERIES + ["zebra w00", "zebra uniqnew w01"])

    # removing what is already gone changes nothing
    ft.remove("d7")
    assert dev.stale == 2 and dev.n_built == n_built

    dev.build()
    assert dev.tail == 0 and dev.stale == 0 and dev.n_built == len(ft)
    _compare(ft, dev, QUERIES + ["zebra w00", "uniqnew"])


@pytest.mark.parametrize("device", DEVICES)
def test_allow_ids(device):
    ft, dev, rng = _index(device)
    dev.build()
    ft.index("new0", "w00 w01 w02")
    ft.index("new1", "w00 w03")
    ft.remove("d3")
    allow = {f"d{d}" for d in range(0, N_DOCS, 3)} | {"new1", "ghost"}
    _compare(ft, dev, allow_ids=allow)
    got = {d for d, _ in dev.search("w00", 400, allow_ids=allow)}
    assert got and got <= allow and "new1" in got and "d3" not in got
    assert dev.search("w00", 10, allow_ids=set()) == []


@pytest.mark.parametrize("device", DEVICES)
def test_needs_rebuild_flips_at_the_ratio(device):
    ft, dev, rng = _index(device)
    dev.build()
    n = dev.n_built
    limit = int(0.2 * n)            # tail + stale may reach this
    for d in range(limit // 2):
        ft.index(f"new{d}", "w00 w01")          # tail
    for d in range(limit - limit // 2):
        ft.remove(f"d{100 + d}")                # stale
    assert dev.tail + dev.stale == limit
    assert not dev.needs_rebuild()
    ft.index("one-more", "w02")
    assert dev.needs_rebuild()
    dev.build()
    assert not dev.needs_rebuild()
    assert dev.tail == 0 and dev.stale == 0 and dev.n_built == len(ft)
    _compare(ft, dev, ks=(10,))
