"""Graph algorithms: GPU (HIP kernels) for large graphs, numpy/python for
small graphs and behavioral parity.

Parity: reference apoc/algo/algo.go:32-417 (PageRank, Betweenness,
Closeness, Degree, AStar, Dijkstra, AllPairs, Cover) and
apoc/community/community.go:66-505 (Louvain, LabelProp, Modularity,
Triangles, ClusteringCoeff, ConnectedComponents).
"""

from __future__ import annotations

import heapq
import os
from collections import defaultdict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops import native_or_none
from .csr import CSRGraph

GPU_MIN_EDGES = 50_000  # below this the numpy path wins on latency


def _use_gpu(g: CSRGraph, device=None) -> bool:
    # the cheap tests first: a small graph never touches the extension
    return (device != "cpu" and g.m >= GPU_MIN_EDGES
            and torch.cuda.is_available() and native_or_none() is not None)


# ---------------------------------------------------------------- PageRank
def pagerank(g: CSRGraph, damping: float = 0.85, iters: int = 20,
             tol: float = 1e-6, device=None) -> np.ndarray:
    if _use_gpu(g, device):
        return _pagerank_gpu(g, damping, iters, tol)
    return _pagerank_np(g, damping, iters, tol)


def _pagerank_np(g: CSRGraph, damping, iters, tol) -> np.ndarray:
    n = g.n
    if n == 0:
        return np.zeros(0, np.float32)
    g.with_in_edges()
    outdeg = g.out_degrees().astype(np.float64)
    rank = np.full(n, 1.0 / n)
    rows = np.repeat(np.arange(n), np.diff(g.in_row_ptr))
    src = g.in_col_idx
    for _ in range(iters):
        contrib = np.where(outdeg > 0, rank / np.maximum(outdeg, 1), 0.0)
        dangling = rank[outdeg == 0].sum() / n
        new = np.full(n, (1 - damping) / n) + damping * dangling
        np.add.at(new, rows, damping * contrib[src])
        if np.abs(new - rank).sum() < tol:
            rank = new
            break
        rank = new
    return rank.astype(np.float32)


def _pagerank_gpu(g: CSRGraph, damping, iters, tol) -> np.ndarray:
    nat = native_or_none()
    dev = "cuda"
    n = g.n
    rp, ci = g.torch_csr(dev, in_edges=True)
    outdeg = torch.as_tensor(g.out_degrees(), dtype=torch.int32, device=dev)
    rank = torch.full((n,), 1.0 / n, device=dev)
    dangling_mask = outdeg == 0
    for _ in range(iters):
        contrib = nat.pagerank_contrib(rank, outdeg)
        dangling = float(rank[dangling_mask].sum()) / n
        base = (1 - damping) / n + damping * dangling
        new = nat.pagerank_gather(rp, ci, contrib, damping, base)
        if float((new - rank).abs().sum()) < tol:
            rank = new
            break
        rank = new
    return rank.cpu().numpy()


# ---------------------------------------------------------------- BFS / SSSP
def bfs_distances(g: CSRGraph, source: int, device=None) -> np.ndarray:
    if _use_gpu(g, device):
        return _bfs_gpu(g, source)
    n = g.n
    dist = np.full(n, -1, np.int32)
    dist[source] = 0
    frontier = [source]
    level = 0
    rp, ci = g.row_ptr, g.col_idx
    while frontier:
        nxt = []
        for u in frontier:
            for j in range(rp[u], rp[u + 1]):
                v = ci[j]
                if dist[v] < 0:
                    dist[v] = level + 1
                    nxt.append(v)
        frontier = nxt
        level += 1
    return dist


def _bfs_gpu(g: CSRGraph, source: int) -> np.ndarray:
    nat = native_or_none()
    dev = "cuda"
    rp, ci = g.torch_csr(dev)
    dist = torch.full((g.n,), -1, dtype=torch.int32, device=dev)
    dist[source] = 0
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    level = 0
    while True:
        changed.zero_()
        nat.bfs_level(rp, ci, dist, changed, 0, level)
        if int(changed.item()) == 0:
            break
        level += 1
    return dist.cpu().numpy()


def dijkstra(g: CSRGraph, source: int, target: int = None):
    """Weighted shortest paths; weights default 1. Returns (dist, prev)."""
    n = g.n
    w = g.weights if g.weights is not None else np.ones(g.m, np.float32)
    dist = np.full(n, np.inf)
    prev = np.full(n, -1, np.int64)
    dist[source] = 0.0
    pq = [(0.0, source)]
    rp, ci = g.row_ptr, g.col_idx
    while pq:
        d, u = heapq.heappop(pq)
        if d > dist[u]:
            continue
        if target is not None and u == target:
            break
        for j in range(rp[u], rp[u + 1]):
            v = ci[j]
            nd = d + w[j]
            if nd < dist[v]:
                dist[v] = nd
                prev[v] = u
                heapq.heappush(pq, (nd, v))
    return dist, prev


def astar(g: CSRGraph, source: int, target: int, heuristic) -> Tuple[float, List[int]]:
    w = g.weights if g.weights is not None else np.ones(g.m, np.float32)
    n = g.n
    dist = np.full(n, np.inf)
    prev = np.full(n, -1, np.int64)
    dist[source] = 0.0
    pq = [(heuristic(source), source)]
    rp, ci = g.row_ptr, g.col_idx
    while pq:
        _, u = heapq.heappop(pq)
        if u == target:
            break
        for j in range(rp[u], rp[u + 1]):
            v = ci[j]
            nd = dist[u] + w[j]
            if nd < dist[v]:
                dist[v] = nd
                prev[v] = u
                heapq.heappush(pq, (nd + heuristic(v), v))
    if not np.isfinite(dist[target]):
        return float("inf"), []
    path = [target]
    while path[-1] != source:
        path.append(int(prev[path[-1]]))
    return float(dist[target]), path[::-1]


def shortest_path(g: CSRGraph, source: int, target: int) -> List[int]:
    dist, prev = dijkstra(g, source, target)
    if not np.isfinite(dist[target]):
        return []
    path = [target]
    while path[-1] != source:
        path.append(int(prev[path[-1]]))
    return path[::-1]


# ------------------------------------------------------- components / labels
def connected_components(g: CSRGraph, device=None) -> np.ndarray:
    """Weakly connected components; returns component id per node."""
    if _use_gpu(g, device):
        return _wcc_gpu(g)
    n = g.n
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    rp, ci = g.row_ptr, g.col_idx
    for u in range(n):
        for j in range(rp[u], rp[u + 1]):
            a, b = find(u), find(int(ci[j]))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.fromiter((find(i) for i in range(n)), np.int64, n)


def _wcc_gpu(g: CSRGraph) -> np.ndarray:
    nat = native_or_none()
    dev = "cuda"
    rp, ci = g.torch_csr(dev)
    comp = torch.arange(g.n, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(64):
        changed.zero_()
        nat.wcc_hook(rp, ci, comp, changed, 0)
        # pointer jumping
        comp = comp[comp.long()].contiguous()
        comp = comp[comp.long()].contiguous()
        if int(changed.item()) == 0:
            break
    return comp.long().cpu().numpy()


def label_propagation(g: CSRGraph, iters: int = 20, device=None) -> np.ndarray:
    if _use_gpu(g, device):
        return _labelprop_gpu(g, iters)
    n = g.n
    labels = np.arange(n, dtype=np.int64)
    rp, ci = g.row_ptr, g.col_idx
    for _ in range(iters):
        changed = False
        new = labels.copy()
        for u in range(n):
            s, e = rp[u], rp[u + 1]
            if s == e:
                continue
            counts: Dict[int, int] = defaultdict(int)
            for j in range(s, e):
                counts[int(labels[ci[j]])] += 1
            # most frequent, ties -> smallest label
            mc = max(counts.values())
            best = min(lb for lb, c in counts.items() if c == mc)
            if best != labels[u]:
                new[u] = best
                changed = True
        labels = new
        if not changed:
            break
    return labels


def _labelprop_gpu(g: CSRGraph, iters: int) -> np.ndarray:
    nat = native_or_none()
    dev = "cuda"
    rp, ci = g.torch_csr(dev)
    labels = torch.arange(g.n, dtype=torch.int32, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(iters):
        changed.zero_()
        labels = nat.labelprop_step(rp, ci, labels, changed, 0)
        if int(changed.item()) == 0:
            break
    return labels.long().cpu().numpy()


# ---------------------------------------------------------------- centrality
def degree_centrality(g: CSRGraph) -> np.ndarray:
    deg = g.out_degrees().astype(np.float64)
    g.with_in_edges()
    deg = deg + np.diff(g.in_row_ptr)
    denom = max(g.n - 1, 1)
    return (deg / denom).astype(np.float32)


def closeness_centrality(g: CSRGraph, nodes: Sequence[int] = None,
                         device=None) -> np.ndarray:
    nodes = range(g.n) if nodes is None else nodes
    if _use_gpu(g, device):
        return _closeness_gpu(g, nodes)
    out = np.zeros(g.n, np.float32)
    for u in nodes:
        d = bfs_distances(g, u, device="cpu")
        reach = d[d >= 0]
        if len(reach) > 1:
            out[u] = (len(reach) - 1) / reach.sum()
    return out


def _closeness_gpu(g: CSRGraph, nodes: Sequence[int]) -> np.ndarray:
    """Multi-source BFS, 64 sources per uint64 word (held as int64): per
    level one `msbfs_level` launch over the in-edge CSR and one readback of
    the 64 per-source counts of newly reached vertices. The integer counts
    feed the same float64 quotient as the CPU path, so the result is
    bit-identical to it."""
    nat = native_or_none()
    dev = "cuda"
    n = g.n
    out = np.zeros(n, np.float32)
    nodes = np.asarray(list(nodes), dtype=np.int64)
    if n == 0 or nodes.size == 0:
        return out
    if nodes.min() < 0 or nodes.max() >= n:
        raise IndexError("closeness_centrality: node index out of range")
    rp, ci = g.torch_csr(dev, in_edges=True)
    frontier = torch.empty(n, dtype=torch.int64, device=dev)
    visited = torch.empty(n, dtype=torch.int64, device=dev)
    nxt = torch.empty(n, dtype=torch.int64, device=dev)
    level_count = torch.zeros(64, dtype=torch.int64, device=dev)
    for b0 in range(0, nodes.size, 64):
        batch = nodes[b0:b0 + 64]
        nb = batch.size
        # a node listed twice in one batch owns two bits of one word
        uniq, inv = np.unique(batch, return_inverse=True)
        words = np.zeros(uniq.size, np.uint64)
        np.bitwise_or.at(words, inv,
                         np.uint64(1) << np.arange(nb, dtype=np.uint64))
        # exactly the bits of the batch's real sources, as an int64 pattern
        full = int(np.bitwise_or.reduce(words, keepdims=True).view(np.int64)[0])
        idx = torch.as_tensor(uniq, device=dev)
        wt = torch.as_tensor(words.view(np.int64), device=dev)
        frontier.zero_()
        frontier[idx] = wt
        visited.copy_(frontier)
        sum_dist = np.zeros(64, np.int64)
        reach = np.ones(64, np.int64)
        level = 0
        while True:
            level_count.zero_()
            nat.msbfs_level(rp, ci, frontier, visited, nxt, level_count, full)
            cnt = level_count.cpu().numpy()
            if not cnt.any():
                break
            sum_dist += (level + 1) * cnt
            reach += cnt
            frontier, nxt = nxt, frontier
            level += 1
        for b in range(nb):
            if reach[b] > 1:
                out[batch[b]] = (int(reach[b]) - 1) / sum_dist[b]
    return out


def _bc_sources(n: int, samples: Optional[int], seed: int):
    """The sources and the scale of betweenness_centrality, shared by the
    CPU and the device route."""
    rng = np.random.default_rng(seed)
    sources = list(rng.choice(n, min(samples, n), replace=False)) \
        if samples else list(range(n))
    scale = (n / max(len(sources), 1)) if samples else 1.0
    return sources, scale


BC_BATCH_BUDGET = 1 << 30  # bytes of dist + sigma + delta state per batch


def _bc_batch(n_sources: int, n: int) -> int:
    """Sources per launch: at most 32, and dist (4) + sigma (8) + delta (8)
    = 20 bytes per source and vertex within the budget (1 GiB, or
    NORNICDB_BC_BATCH bytes)."""
    budget = int(os.environ.get("NORNICDB_BC_BATCH") or BC_BATCH_BUDGET)
    return max(1, min(n_sources, 32, budget // (20 * max(n, 1))))


def _betweenness_gpu(g: CSRGraph, sources: Sequence[int],
                     scale: float) -> np.ndarray:
    """Brandes' algorithm on the device, a batch of sources per launch:
    `bc_forward` levels over the in-edge CSR until nothing changes, then
    `bc_backward` from the deepest level down to 0 over the out-edge CSR and
    `bc_accumulate` into the float64 sum. No atomics; the result does not
    depend on the batch size."""
    nat = native_or_none()
    dev = "cuda"
    n = g.n
    sources = np.asarray(list(sources), dtype=np.int64)
    if n == 0 or sources.size == 0:
        return np.zeros(n, np.float32)
    rp, ci = g.torch_csr(dev)
    irp, ici = g.torch_csr(dev, in_edges=True)
    nbatch = _bc_batch(sources.size, n)
    dist = torch.empty(nbatch, n, dtype=torch.int32, device=dev)
    sigma = torch.empty(nbatch, n, dtype=torch.float64, device=dev)
    delta = torch.empty(nbatch, n, dtype=torch.float64, device=dev)
    bc = torch.zeros(n, dtype=torch.float64, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for b0 in range(0, sources.size, nbatch):
        src = torch.as_tensor(sources[b0:b0 + nbatch], device=dev)
        nb = src.numel()
        d, s, dl = dist[:nb], sigma[:nb], delta[:nb]
        rows = torch.arange(nb, device=dev)
        d.fill_(-1)
        s.zero_()
        dl.zero_()
        d[rows, src] = 0
        s[rows, src] = 1.0
        level = 0
        while True:
            changed.zero_()
            nat.bc_forward(irp, ici, d, s, changed, level)
            if int(changed.item()) == 0:
                break
            level += 1
        # `level` is the deepest level any source of the batch reached
        for lv in range(level - 1, -1, -1):
            nat.bc_backward(rp, ci, d, s, dl, lv)
        nat.bc_accumulate(dl, src, bc)
    return (bc.cpu().numpy() * scale).astype(np.float32)


def betweenness_centrality(g: CSRGraph, samples: int = None,
                           seed: int = 0, device=None) -> np.ndarray:
    """Brandes' algorithm (exact, or source-sampled approximation)."""
    n = g.n
    sources, scale = _bc_sources(n, samples, seed)
    if _use_gpu(g, device):
        return _betweenness_gpu(g, sources, scale)
    bc = np.zeros(n)
    rp, ci = g.row_ptr, g.col_idx
    for s in sources:
        stack = []
        preds = [[] for _ in range(n)]
        sigma = np.zeros(n)
        sigma[s] = 1
        dist = np.full(n, -1)
        dist[s] = 0
        q = [s]
        while q:
            nq = []
            for u in q:
                stack.append(u)
                for j in range(rp[u], rp[u + 1]):
                    v = int(ci[j])
                    if dist[v] < 0:
                        dist[v] = dist[u] + 1
                        nq.append(v)
                    if dist[v] == dist[u] + 1:
                        sigma[v] += sigma[u]
                        preds[v].append(u)
            q = nq
        delta = np.zeros(n)
        for v in reversed(stack):
            for u in preds[v]:
                delta[u] += sigma[u] / sigma[v] * (1 + delta[v])
            if v != s:
                bc[v] += delta[v]
        # (stack built in BFS order already)
    return (bc * scale).astype(np.float32)


# --------------------------------------------------------------- community
def triangle_count(g: CSRGraph) -> int:
    n = g.n
    neigh = [set() for _ in range(n)]
    rp, ci = g.row_ptr, g.col_idx
    for u in range(n):
        for j in range(rp[u], rp[u + 1]):
            v = int(ci[j])
            if v != u:
                neigh[u].add(v)
                neigh[v].add(u)
    count = 0
    for u in range(n):
        for v in neigh[u]:
            if v > u:
                count += len(neigh[u] & neigh[v] & set(range(v + 1, n)))
    return count


def clustering_coefficient(g: CSRGraph) -> np.ndarray:
    n = g.n
    neigh = [set() for _ in range(n)]
    rp, ci = g.row_ptr, g.col_idx
    for u in range(n):
        for j in range(rp[u], rp[u + 1]):
            v = int(ci[j])
            if v != u:
                neigh[u].add(v)
                neigh[v].add(u)
    out = np.zeros(n, np.float32)
    for u in range(n):
        k = len(neigh[u])
        if k < 2:
            continue
        links = sum(1 for v in neigh[u] for w in neigh[u]
                    if v < w and w in neigh[v])
        out[u] = 2.0 * links / (k * (k - 1))
    return out


def modularity(g: CSRGraph, communities: np.ndarray) -> float:
    """Newman modularity of a partition (undirected interpretation)."""
    m = g.m
    if m == 0:
        return 0.0
    deg = np.zeros(g.n)
    rp, ci = g.row_ptr, g.col_idx
    inside = 0.0
    for u in range(g.n):
        for j in range(rp[u], rp[u + 1]):
            v = int(ci[j])
            deg[u] += 1
            deg[v] += 1
            if communities[u] == communities[v]:
                inside += 2
    two_m = 2.0 * m
    q = inside / two_m
    for c in np.unique(communities):
        dc = deg[communities == c].sum()
        q -= (dc / two_m) ** 2
    return float(q)


def louvain_reference(g: CSRGraph, max_passes: int = 5) -> np.ndarray:
    """Single-level dict-based Louvain — kept as the small-graph oracle
    for the array implementation below."""
    n = g.n
    comm = np.arange(n)
    adj: List[Dict[int, float]] = [defaultdict(float) for _ in range(n)]
    rp, ci = g.row_ptr, g.col_idx
    w = g.weights if g.weights is not None else np.ones(g.m, np.float32)
    for u in range(n):
        for j in range(rp[u], rp[u + 1]):
            v = int(ci[j])
            if u == v:
                continue
            adj[u][v] += float(w[j])
            adj[v][u] += float(w[j])
    k = np.array([sum(adj[u].values()) for u in range(n)])
    two_m = k.sum()
    if two_m == 0:
        return comm
    sigma_tot = {c: k[c] for c in range(n)}
    for _ in range(max_passes):
        moved = False
        for u in range(n):
            cu = comm[u]
            links = defaultdict(float)
            for v, wv in adj[u].items():
                links[comm[v]] += wv
            sigma_tot[cu] -= k[u]
            best_c, best_gain = cu, 0.0
            for c, l_uc in links.items():
                gain = l_uc - sigma_tot.get(c, 0.0) * k[u] / two_m
                base = links.get(cu, 0.0) - sigma_tot.get(cu, 0.0) * k[u] / two_m
                if gain - base > best_gain + 1e-12:
                    best_gain = gain - base
                    best_c = c
            sigma_tot[best_c] = sigma_tot.get(best_c, 0.0) + k[u]
            if best_c != cu:
                comm[u] = best_c
                moved = True
        if not moved:
            break
    _, inv = np.unique(comm, return_inverse=True)
    return inv


def _louvain_local_moving(src, dst, w, k, n, two_m, max_passes, resolution,
                          rng, device="cpu"):
    """Vectorized local-moving phase over a symmetric edge list.

    Implemented in torch ops (multithreaded on CPU; runs unchanged on a
    GPU device for very large graphs): per pass, edges are keyed
    (u, comm[v]) and sorted; segment sums give the link weight from each
    node to each neighbouring community; scatter_reduce(amax) picks the
    best-gain move per node. The synchronous-update oscillation is
    avoided by applying moves to two random node halves alternately.
    Only the ACTIVE set (nodes adjacent to a move) is re-examined after
    the first pass.
    """
    import torch
    dev = torch.device(device)
    ts = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(dst)).to(dev)
    tw = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    tk = torch.from_numpy(np.ascontiguousarray(k)).to(dev)
    comm = torch.arange(n, dtype=torch.int64, device=dev)
    sigma = tk.clone()
    active = torch.ones(n, dtype=torch.bool, device=dev)
    inv2m = resolution / two_m
    for _p in range(max_passes):
        e_mask = active[ts]
        if not bool(e_mask.any()):
            break
        es, ed, ew = ts[e_mask], td[e_mask], tw[e_mask]
        total_moved = 0
        next_active = torch.zeros(n, dtype=torch.bool, device=dev)
        half_mask = torch.rand(n, generator=None, device=dev) < 0.5
        for half in (half_mask, ~half_mask):
            key = es * n + comm[ed]
            ks, order = key.sort(stable=True)
            ws = ew[order]
            bnd = torch.ones(ks.numel(), dtype=torch.bool, device=dev)
            bnd[1:] = ks[1:] != ks[:-1]
            starts = bnd.nonzero(as_tuple=True)[0]
            csum = ws.cumsum(0)
            ends = torch.cat([starts[1:], torch.tensor([ks.numel()],
                                                       device=dev)])
            l_uc = csum[ends - 1]
            l_uc[1:] = l_uc[1:] - csum[starts[1:] - 1]
            uu = torch.div(ks[starts], n, rounding_mode="floor")
            cc = ks[starts] - uu * n
            ku = tk[uu]
            cu = comm[uu]
            sig_c = torch.where(cc == cu, sigma[cc] - ku, sigma[cc])
            gain = l_uc - sig_c * ku * inv2m
            # baseline: gain of staying in the current community
            base = -(sigma[comm] - tk) * tk * inv2m
            is_cur = cc == cu
            base[uu[is_cur]] = gain[is_cur]
            # best candidate per node via scatter-amax, then first argmax
            gmax = torch.full((n,), -3.4e38, dtype=gain.dtype, device=dev)
            gmax.scatter_reduce_(0, uu, gain, reduce="amax")
            at_max = gain >= gmax[uu]
            pos = torch.full((n,), ks.numel(), dtype=torch.int64, device=dev)
            idx = at_max.nonzero(as_tuple=True)[0]
            pos.scatter_reduce_(0, uu[idx], idx, reduce="amin")
            best = pos[pos < ks.numel()]
            cand_u = uu[best]
            cand_c = cc[best]
            cand_g = gain[best]
            sel = (cand_g > base[cand_u] + 1e-12) & half[cand_u] \
                & (comm[cand_u] != cand_c)
            move_u = cand_u[sel]
            move_c = cand_c[sel]
            if move_u.numel() == 0:
                continue
            sigma.scatter_add_(0, comm[move_u], -tk[move_u])
            sigma.scatter_add_(0, move_c, tk[move_u])
            comm[move_u] = move_c
            next_active[move_u] = True
            total_moved += int(move_u.numel())
        # fractional convergence threshold only at scale — small graphs
        # legitimately move < 32 nodes per pass and must keep iterating
        if total_moved == 0 or (n > 10000 and total_moved < n // 200):
            break
        touched = next_active[td]
        next_active[ts[touched]] = True
        active = next_active
    _, inv = torch.unique(comm, return_inverse=True)
    return inv.cpu().numpy()


def louvain(g: CSRGraph, max_passes: int = 10, max_levels: int = 10,
            resolution: float = 1.0, seed: int = 0,
            device: str = "cpu") -> np.ndarray:
    """Multi-level Louvain, fully array-based (CSR + numpy) — scales to
    10M+ edge graphs in seconds where a dict-of-dict walk cannot
    (replaced unit: reference apoc/community/community.go:66-505;
    louvain_reference above is the small-graph oracle)."""
    n = g.n
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    rp, ci = g.row_ptr, g.col_idx
    w0 = (g.weights if g.weights is not None
          else np.ones(g.m, np.float32)).astype(np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    cols = ci.astype(np.int64)
    keep = rows != cols  # self-loops don't drive moves
    src = np.concatenate([rows[keep], cols[keep]])
    dst = np.concatenate([cols[keep], rows[keep]])
    w = np.concatenate([w0[keep], w0[keep]])
    two_m = w.sum()
    node_comm = np.arange(n, dtype=np.int64)
    if two_m == 0 or src.size == 0:
        return node_comm
    rng = np.random.default_rng(seed)

    # degrees INCLUDING intra-community weight, carried through levels
    # (self-loops are dropped from the edge list after aggregation, so
    # recomputing k from it would understate sigma at deeper levels)
    k = np.bincount(src, weights=w, minlength=n)
    cur_n = n
    for _level in range(max_levels):
        local = _louvain_local_moving(src, dst, w, k, cur_n, two_m,
                                      max_passes, resolution, rng, device)
        ncomm = int(local.max()) + 1
        node_comm = local[node_comm]
        if ncomm == cur_n:
            break
        # aggregate: communities become nodes, parallel edges sum,
        # intra-community edges become self-loops (dropped from the edge
        # list; their weight stays in the carried degree vector k).
        # torch's multithreaded sort: this is a full-m pass per level.
        import torch as _t
        tl = _t.from_numpy(local)
        key = tl[_t.from_numpy(src)] * ncomm + tl[_t.from_numpy(dst)]
        ks, order = key.sort(stable=True)
        ws = _t.from_numpy(w)[order]
        bnd = _t.ones(ks.numel(), dtype=_t.bool)
        bnd[1:] = ks[1:] != ks[:-1]
        starts = bnd.nonzero(as_tuple=True)[0]
        csum = ws.cumsum(0)
        ends = _t.cat([starts[1:], _t.tensor([ks.numel()])])
        wseg = csum[ends - 1].clone()
        wseg[1:] -= csum[starts[1:] - 1]
        ksg = ks[starts]
        s2 = _t.div(ksg, ncomm, rounding_mode="floor")
        d2 = ksg - s2 * ncomm
        keep2 = s2 != d2
        src = s2[keep2].numpy()
        dst = d2[keep2].numpy()
        w = wseg[keep2].numpy()
        k = np.bincount(local, weights=k, minlength=ncomm)
        cur_n = ncomm
        if src.size == 0:
            break
    _, inv = np.unique(node_comm, return_inverse=True)
    return inv
