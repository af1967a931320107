#!/usr/bin/env python3
"""Closeness and betweenness centrality on one GPU against the CPU loops.

Two parts, both on `random_graph`, generated from a seed:

`--part small`: `random_graph(6250, 8)`, m = 50 000, the size from which the
public functions take the device route. Closeness over all nodes and
betweenness with samples=64, device route against `device="cpu"`. The CPU
closeness loop is timed over every `--cpu-stride`-th node only (a full pass
is minutes per sample): per-source cost is independent of the other sources,
so that time is a lower bound of the full CPU pass, and the table also gives
it scaled to all nodes.

`--part large`: `random_graph(1_000_000, 10)`, GPU only: closeness with
nodes=range(4096) and betweenness with samples=256. Reported per variant: ms
per source and edge visits per second. Edge visits are counted from the
launches of one untimed call: a `msbfs_level` launch visits m edges for each
of the batch's sources, a `bc_forward` / `bc_backward` launch m edges for
each of its B sources. The split between kernel time and host readbacks
comes from a kernel trace of `--part large --repeats 1`, taken in a run of
its own; `wall_ms` of that run is the figure to set the kernel sum against.

Timing: a host clock around whole calls, which end in a device-to-host copy
of the result, after one warm-up call of every variant; the variants
alternate inside each of `--repeats` rounds. The table gives the median and
min..max. A run without a GPU is refused unless --rehearse is given.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


class _Counting:
    """Proxy of the native module that counts (launches, source-edge visits)
    per binding."""

    def __init__(self, nat, m):
        self._nat, self._m = nat, m
        self.launches, self.visits = {}, {}

    def __getattr__(self, name):
        fn = getattr(self._nat, name)

        def call(*a):
            if name == "msbfs_level":
                srcs = bin(a[6] & (2 ** 64 - 1)).count("1")
            elif name in ("bc_forward", "bc_backward"):
                srcs = a[2].shape[0]
            else:
                srcs = 0
            self.launches[name] = self.launches.get(name, 0) + 1
            self.visits[name] = self.visits.get(name, 0) + srcs * self._m
            return fn(*a)
        return call


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", choices=["small", "large", "all"], default="all")
    p.add_argument("--repeats", type=int, default=7, help="samples per variant")
    p.add_argument("--cpu-stride", type=int, default=25,
                   help="CPU closeness is timed over every n-th node")
    p.add_argument("--rehearse", action="store_true",
                   help="run the host logic on the CPU at a tiny shape")
    args = p.parse_args()

    from nornicdb_amd import ops
    from nornicdb_amd.graph import (algos, betweenness_centrality,
                                    closeness_centrality, random_graph)

    on_gpu = not args.rehearse
    if on_gpu:
        if not torch.cuda.is_available():
            sys.exit("centrality_bench: needs a GPU (or --rehearse)")
        ops.require_native()
    else:
        args.repeats = 2

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        if on_gpu:
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    total = {}  # name -> [calls, wall ms] over every call, timed or not

    def tally(variants):
        def wrap(name, fn):
            def call():
                t0 = time.perf_counter()
                r = fn()
                t = total.setdefault(name, [0, 0.0])
                t[0] += 1
                t[1] += (time.perf_counter() - t0) * 1e3
                return r
            return call
        return {name: wrap(name, fn) for name, fn in variants.items()}

    def run(variants):
        for fn in variants.values():
            fn()
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                samples[name].append(timed(fn))
        return samples

    def count(g, fn):
        """(launches, visits) of one untimed call of a device route."""
        if not on_gpu:
            return {}, {}
        real = algos.native_or_none
        proxy = _Counting(real(), g.m)
        algos.native_or_none = lambda: proxy
        try:
            fn()
        finally:
            algos.native_or_none = real
        return proxy.launches, proxy.visits

    out = []

    def report(title, g, samples, meta):
        print(f"# {title}: n={g.n} m={g.m}, {args.repeats} samples"
              + (" (REHEARSAL: not a measurement)" if not on_gpu else ""))
        print("| variant | ms median | min..max | sources | ms/source | "
              "G edge visits/s |")
        print("|---|---|---|---|---|---|")
        for name, xs in samples.items():
            med = statistics.median(xs)
            mt = meta.get(name, {})
            srcs = mt.get("sources")
            visits = sum(mt.get("visits", {}).values())
            per = f"{med / srcs:.4f}" if srcs else ""
            rate = f"{visits / med / 1e6:.2f}" if visits else ""
            print(f"| {name} | {med:.2f} | {min(xs):.2f}..{max(xs):.2f} | "
                  f"{srcs or ''} | {per} | {rate} |")
            out.append({"graph": title, "variant": name,
                        "ms_median": round(med, 3), "ms_min": round(min(xs), 3),
                        "ms_max": round(max(xs), 3), **mt})

    if args.part in ("small", "all"):
        n, deg = (6250, 8) if on_gpu else (400, 8)
        g = random_graph(n, deg)
        sub = list(range(0, g.n, args.cpu_stride))
        variants = {
            "closeness cpu, every %d-th node" % args.cpu_stride:
                lambda: closeness_centrality(g, sub, device="cpu"),
            "betweenness samples=64 cpu":
                lambda: betweenness_centrality(g, samples=64, device="cpu"),
        }
        meta = {"closeness cpu, every %d-th node" % args.cpu_stride:
                {"sources": len(sub)},
                "betweenness samples=64 cpu": {"sources": 64}}
        if on_gpu:
            assert algos._use_gpu(g)
            variants["closeness gpu, all nodes"] = \
                lambda: closeness_centrality(g)
            variants["betweenness samples=64 gpu"] = \
                lambda: betweenness_centrality(g, samples=64)
            for name, srcs in (("closeness gpu, all nodes", g.n),
                               ("betweenness samples=64 gpu", 64)):
                launches, visits = count(g, variants[name])
                meta[name] = {"sources": srcs, "launches": launches,
                              "visits": visits}
            assert closeness_centrality(g, sub).tobytes() == \
                closeness_centrality(g, sub, device="cpu").tobytes()
        samples = run(variants)
        report("random_graph(%d, %d)" % (n, deg), g, samples, meta)
        cpu = samples["closeness cpu, every %d-th node" % args.cpu_stride]
        print(f"closeness cpu scaled to all {g.n} nodes: median "
              f"{statistics.median(cpu) * g.n / len(sub):.0f} ms "
              f"(lower bound measured: {min(cpu):.0f} ms)")

    if args.part in ("large", "all") and on_gpu:
        g = random_graph(1_000_000, 10)
        g.with_in_edges()
        variants = tally({
            "closeness nodes=range(4096) gpu":
                lambda: closeness_centrality(g, nodes=range(4096)),
            "betweenness samples=256 gpu":
                lambda: betweenness_centrality(g, samples=256),
        })
        meta = {}
        for name, srcs in (("closeness nodes=range(4096) gpu", 4096),
                           ("betweenness samples=256 gpu", 256)):
            launches, visits = count(g, variants[name])
            meta[name] = {"sources": srcs, "launches": launches,
                          "visits": visits}
        samples = run(variants)
        report("random_graph(1000000, 10)", g, samples, meta)
        # what a kernel trace of this process is set against
        for name, (calls, wall) in total.items():
            print(f"all calls of {name}: {calls} calls, wall_ms {wall:.1f}")

    print(json.dumps({"rehearsal": not on_gpu, "repeats": args.repeats,
                      "results": out}))


if __name__ == "__main__":
    main()
