"""Graphs and CPU references shared by tests/test_centrality.py and
tests/test_centrality_kernels.py. A plain module, no fixtures: every graph is
built from fixed edge lists or a seeded generator, and every reference (the
CPU closeness / betweenness of graph/algos.py) is computed once per process
and never modified. Each graph is small enough that the CPU functions answer
in well under a second.
"""

import numpy as np

from nornicdb_amd.graph import (betweenness_centrality, closeness_centrality,
                                from_edges, random_graph)

_cache = {}


def _random():
    return random_graph(300, 5, seed=1)  # 1500 edges


def _path():
    """Directed path: more than 64 levels, and sources near the end stop
    early."""
    return from_edges(200, [(i, i + 1) for i in range(199)])


def _layered():
    """72 layers x 4 nodes, complete bipartite between consecutive layers:
    288 nodes, 1136 edges. sigma reaches 4^71, beyond fp32."""
    edges = [(4 * layer + a, 4 * (layer + 1) + b)
             for layer in range(71) for a in range(4) for b in range(4)]
    return from_edges(288, edges)


def _hub():
    """Rows of 64 and 65 edges in both CSRs, the boundary of the whole-wave
    row pass: 64 leaves -> 0 -> 2 -> 64 leaves -> (the first 64 of) 65 leaves
    -> 1 -> 3 -> 65 leaves. In-degrees of 0 / 1 are 64 / 65, out-degrees of
    2 / 3 are 64 / 65."""
    la = list(range(4, 68))         # 64 leaves into 0
    lc = list(range(68, 132))       # 64 leaves out of 2
    lb = list(range(132, 197))      # 65 leaves into 1
    ld = list(range(197, 262))      # 65 leaves out of 3
    edges = [(v, 0) for v in la] + [(0, 2)] + [(2, v) for v in lc]
    edges += [(lc[i], lb[i]) for i in range(64)]
    edges += [(v, 1) for v in lb] + [(1, 3)] + [(3, v) for v in ld]
    return from_edges(262, edges)


def _wide_hub():
    """Rows of more than a thousand edges in both CSRs, made of duplicate
    edges so that the graph stays at 82 nodes: the whole-wave pass takes its
    unrolled loop (8 x 64 edges a trip) and then the remainder loop. 40
    leaves -> 0 -> 1 -> 40 leaves -> the first leaves again."""
    la = list(range(2, 42))
    lb = list(range(42, 82))
    edges = [(0, 1)]
    for i in range(40):
        edges += [(la[i], 0)] * (20 + i % 15)
        edges += [(1, lb[i])] * (21 + i % 13)
        edges.append((lb[i], la[(i + 1) % 40]))
    g = from_edges(82, edges)
    g.with_in_edges()
    assert np.diff(g.in_row_ptr)[0] > 1024 and g.out_degrees()[1] > 1024
    return g


def _disconnected():
    """Two components (a 20-ring with chords, a 15-node two-way path) and 5
    isolated nodes."""
    edges = [(i, (i + 1) % 20) for i in range(20)]
    edges += [(i, (i + 7) % 20) for i in range(0, 20, 3)]
    for i in range(20, 34):
        edges += [(i, i + 1), (i + 1, i)]
    return from_edges(40, edges)


def _multigraph():
    """Duplicate edges and self-loops: [(0,1),(0,1),(1,2),(2,2)] carried on
    over 30 nodes."""
    edges = [(0, 1), (0, 1), (1, 2), (2, 2)]
    for i in range(2, 29):
        edges.append((i, i + 1))
        if i % 2 == 0:
            edges.append((i, i + 1))
        if i % 3 == 0:
            edges.append((i, i))
        if i % 5 == 0 and i + 3 < 30:
            edges += [(i, i + 3), (i, i + 3), (i, i + 3)]
    return from_edges(30, edges)


def _one_way():
    """u -> v without v -> u: closeness along out-edges and along in-edges
    differ at every node (checked in test_centrality.py), so a transposed
    CSR cannot pass."""
    n = 41
    edges = [(i, i + 1) for i in range(n - 1)]
    edges += [(i, i + 3) for i in range(0, n - 3, 2)]
    edges += [(i, i + 10) for i in range(0, 12)]
    return from_edges(n, edges)


BUILDERS = {
    "random": _random,
    "path": _path,
    "layered": _layered,
    "hub": _hub,
    "wide_hub": _wide_hub,
    "disconnected": _disconnected,
    "multigraph": _multigraph,
    "one_way": _one_way,
}
CASES = list(BUILDERS)


def graph(name):
    key = ("graph", name)
    if key not in _cache:
        _cache[key] = BUILDERS[name]()
    return _cache[key]


def transposed(g):
    rows = np.repeat(np.arange(g.n), np.diff(g.row_ptr))
    return from_edges(g.n, list(zip(g.col_idx.tolist(), rows.tolist())))


# Closeness node sets: one source, one short of a word, a full word, a word
# and one bit, three words with a partial last one, and a shuffled subset with
# a node listed twice. Indices wrap on graphs with fewer nodes, which repeats
# nodes there and keeps the batch shapes.
def _shuffled():
    rng = np.random.default_rng(11)
    pick = rng.permutation(150)[:45].tolist()
    return pick[:20] + [pick[3]] + pick[20:]


NODE_SETS = {
    "one": [0],
    "r63": list(range(63)),
    "r64": list(range(64)),
    "r65": list(range(65)),
    "r130": list(range(130)),
    "shuffled_repeat": _shuffled(),
}


def nodes_of(name, set_name):
    n = graph(name).n
    return [v % n for v in NODE_SETS[set_name]]


def closeness_ref(name, set_name):
    key = ("closeness", name, set_name)
    if key not in _cache:
        ref = closeness_centrality(graph(name), nodes_of(name, set_name),
                                   device="cpu")
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


SEED = 5
SAMPLES = [None, 7, 33]   # exact; a partial batch; two batches at B = 32


def betweenness_ref(name, samples):
    key = ("betweenness", name, samples)
    if key not in _cache:
        ref = betweenness_centrality(graph(name), samples=samples, seed=SEED,
                                     device="cpu")
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


BC_RTOL = 2.0 ** -22


def check_betweenness(got, ref):
    """|got - ref| <= 2^-22 |ref| per node, zeros exactly zero; returns the
    largest |got - ref| / |ref| seen. Every sigma, delta and bc is a sum of
    non-negative terms (no cancellation); the fp64 chains lose at most about
    (levels x max degree) x 2^-52, under 2^-29 for these graphs, and the two
    float32 output roundings are 2^-24 each."""
    assert got.dtype == np.float32 and got.shape == ref.shape
    g64, r64 = got.astype(np.float64), ref.astype(np.float64)
    assert np.isfinite(g64).all()
    zero = r64 == 0
    assert (g64[zero] == 0).all(), "a zero of the reference is not zero"
    err = np.abs(g64 - r64)
    ratio = float((err[~zero] / np.abs(r64[~zero])).max()) if (~zero).any() \
        else 0.0
    print(f"betweenness max relative error {ratio:.3e} "
          f"(bound {BC_RTOL:.3e})")
    assert (err <= BC_RTOL * np.abs(r64)).all(), ratio
    return ratio
