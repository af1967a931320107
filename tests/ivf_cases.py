"""Scaffolding shared by tests/test_ivf.py and tests/test_ivf_quant.py: the
inverted lists, probes and decoy cases of the GPU scan tests, the contract
check of their results, and the clustered recall corpus. A plain module, no
fixtures; everything is deterministic and cached once per process.
"""

import torch

from nornicdb_amd.ops import IVFLists

NEG_INF = float("-inf")

N = 3000
C = 24
ROW_BASE = 1000
TAILS = [N, N - 1, N - 37]
# list 0 empty, 1..4 around the 16-lane group count, 5 long enough that a
# block strides through it several times at every Q of the sweeps; the rest
# random
FIXED = [0, 1, 15, 16, 17, 1200]
AWKWARD = [0, 1, 2, 3, 4, 5]

_cache = {}


def py_reach(lists, probes, n, tail_start):
    """bool [Q, n] from plain Python slices of the CSR arrays."""
    off = lists.list_off.tolist()
    rows = lists.list_rows.tolist()
    reach = torch.zeros(probes.shape[0], n, dtype=torch.bool)
    for qi, pr in enumerate(probes.tolist()):
        for c in pr:
            if 0 <= c < len(off) - 1:
                reach[qi, rows[off[c]:off[c + 1]]] = True
        reach[qi, tail_start:] = True
    return reach


def cpu_lists(tail_start):
    """CSR over a random permutation of rows [0, tail_start), on the CPU:
    rows are in random order inside every list."""
    key = ("lists", tail_start)
    if key not in _cache:
        g = torch.Generator().manual_seed(tail_start)
        rest = tail_start - sum(FIXED)
        cuts = torch.sort(torch.randint(0, rest + 1, (C - len(FIXED) - 1,),
                                        generator=g)).values.tolist()
        sizes = FIXED + [b - a for a, b in zip([0] + cuts, cuts + [rest])]
        assert len(sizes) == C and sum(sizes) == tail_start
        off = torch.zeros(C + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(torch.tensor(sizes), 0)
        rows = torch.randperm(tail_start, generator=g).to(torch.int32)
        _cache[key] = IVFLists(torch.zeros(C, 8), off, rows, tail_start,
                               max(sizes))
    return _cache[key]


def gpu_lists(tail_start):
    """(cpu_lists(tail_start) on the GPU, the same on the CPU)."""
    key = ("gpu lists", tail_start)
    if key not in _cache:
        cpu = cpu_lists(tail_start)
        gpu = IVFLists(cpu.centroids.cuda(), cpu.list_off.cuda(),
                       cpu.list_rows.cuda(), tail_start, cpu.max_len)
        _cache[key] = (gpu, cpu)
    return _cache[key]


def case_probes(q_count):
    """int32 [Q, 8]: six distinct lists per query with two -1 entries mixed
    in; query 0 probes the awkward lists, query 1 (if any) also carries an
    out-of-range id."""
    key = ("probes", q_count)
    if key not in _cache:
        g = torch.Generator().manual_seed(q_count)
        out = torch.full((q_count, 8), -1, dtype=torch.int32)
        for r in range(q_count):
            cols = torch.randperm(8, generator=g)[:6]
            pick = torch.tensor(AWKWARD) if r == 0 else \
                torch.randperm(C, generator=g)[:6]
            out[r, cols] = pick.to(torch.int32)
        if q_count > 1:
            out[1, (out[1] == -1).nonzero()[0, 0]] = C + 5
        _cache[key] = out
    return _cache[key]


def decoy_case(q_count, tail_start, masked):
    """(decoys int64 [Q], allow bool [N] or None, ok bool [Q, N]), on the
    CPU. decoys[r] is a row that query r must not return: a row of a list it
    does not probe, or (masked, odd queries) a disallowed row of a list it
    does probe. The tests use copies of these rows as queries."""
    key = ("case", q_count, tail_start, masked)
    if key in _cache:
        return _cache[key]
    reach = py_reach(cpu_lists(tail_start), case_probes(q_count), N,
                     tail_start)
    g = torch.Generator().manual_seed(q_count * 7 + tail_start)
    allow = None
    if masked:
        allow = torch.rand(N, generator=g) < 0.5
    decoys = []
    for r in range(q_count):
        pool = (~reach[r]).nonzero().flatten()
        if masked and r % 2 == 1:
            pool = reach[r].nonzero().flatten()
        row = int(pool[int(torch.randint(0, len(pool), (1,), generator=g))])
        if masked:
            allow[row] = False
        decoys.append(row)
    ok = reach if allow is None else reach & allow[None, :]
    decoys = torch.tensor(decoys)
    assert not ok[torch.arange(q_count), decoys].any()
    _cache[key] = (decoys, allow, ok)
    return _cache[key]


def gpu_case(name, corpus, q_count, tail_start, masked):
    """(q [Q, D], allow bool [N] or None, ok bool [Q, N]) on the GPU: the
    decoy_case whose queries are copies of the decoy rows of `corpus`, an
    [N, D] GPU tensor. Cached under `name`, the caller's key for corpus."""
    key = ("gpu case", name, q_count, tail_start, masked)
    if key not in _cache:
        decoys, allow, ok = decoy_case(q_count, tail_start, masked)
        _cache[key] = (corpus[decoys.cuda()].clone(),
                       None if allow is None else allow.cuda(), ok.cuda())
    return _cache[key]


def check(ref_scores, tol, ok, k, row_base, s, i):
    """ok: bool [Q, N], the rows each query may return. ref_scores is the
    fp32 [Q, N] product of the stored values."""
    torch.cuda.synchronize()
    q_count, n = ok.shape
    kk = min(k, n)
    assert s.shape == (q_count, kk) and i.shape == s.shape
    assert i.dtype == torch.int64 and s.dtype == torch.float32
    ref = ref_scores.masked_fill(~ok, NEG_INF)
    rs, _ = torch.topk(ref, kk, dim=-1)
    m = ok.sum(-1).clamp_max(kk)
    filled = torch.arange(kk, device=s.device)[None, :] < m[:, None]
    assert ((i == -1) == ~filled).all(), i
    assert (s[~filled] == NEG_INF).all(), s
    loc = torch.where(filled, i - row_base, 0)
    assert ((loc >= 0) & (loc < n)).all(), i
    assert (torch.gather(ok, 1, loc) | ~filled).all(), \
        "a row outside the probed, allowed set was returned"
    srt = torch.where(filled, loc, -1 - torch.arange(kk, device=s.device)) \
        .sort(dim=-1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "duplicate hit"
    err = (s - rs)[filled].abs().max().item() if filled.any() else 0.0
    own = (torch.gather(ref, 1, loc) - s)[filled].abs().max().item() \
        if filled.any() else 0.0
    print(f"Q={q_count} k={k}: rank err {err:.3e} own err {own:.3e}")
    assert err <= tol, err
    assert own <= tol, own
    assert (s[:, :-1] >= s[:, 1:]).all()


def clustered(seed, d, device="cpu", n=4096, n_centres=32, n_queries=64):
    """Unit-norm fp32 rows around 32 random unit centres, and queries that
    are perturbed rows."""
    g = torch.Generator().manual_seed(seed)
    nz = torch.nn.functional.normalize
    centres = nz(torch.randn(n_centres, d, generator=g), dim=-1)
    which = torch.randint(0, n_centres, (n,), generator=g)
    x = nz(centres[which] + 0.15 * torch.randn(n, d, generator=g), dim=-1)
    pick = torch.randperm(n, generator=g)[:n_queries]
    q = nz(x[pick] + 0.05 * torch.randn(n_queries, d, generator=g), dim=-1)
    return x.to(device), q.to(device)


def recall_at(got_idx, ref_idx):
    hits = sum(len(set(a) & set(b))
               for a, b in zip(got_idx.tolist(), ref_idx.tolist()))
    return hits / ref_idx.numel()
