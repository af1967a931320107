#!/usr/bin/env python3
"""BM25 on the device: the bm25_scan kernel on synthetic postings, and the
device full-text index against the host one.

Part 1. Zipf postings built directly as tensors: `--docs` documents (4M) of
32..96 tokens (mean 64) drawn from a Zipf(1) vocabulary of `--vocab` terms.
`bm25_search` is timed for T = 1, 4, 8 query terms, rare terms (Zipf rank
20000 on, a few hundred postings each at 4M documents) and common ones
(rank 8 on, every third document), k = 10 and k = 40 (hybrid search's
over-fetch, the K = 64 kernel), Q = 1 and Q = 16 (every query its own
terms). Posting bytes are 8 B per posting of the queried lists plus 4 B
per doc_len gather, counted on the host from the CSR offsets; GB/s is those
bytes over the call time. The split between the scan and the merge kernel
comes from a kernel trace of this script, taken in a run of its own.

Timing: device events around `--iters` back-to-back calls per sample, after
a warm-up of every variant; the variants alternate inside each of
`--repeats` rounds. The table gives the median sample and min..max in ms
per call.

Part 2. A `--host-docs` (200k) document FulltextIndex of the same Zipf
text and the DeviceFulltextIndex over it. `FulltextIndex.search` and
`DeviceFulltextIndex.search` answer identical queries alternately, k = 40,
both on the host clock (the device search ends with a copy to the host).
The device path's median must lie below the host path's minimum for the
common-term queries; the script prints whether it does.

A run without a GPU is refused unless --rehearse is given.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

K1, B = 1.2, 0.75
RARE, COMMON = 20000, 8   # first Zipf rank of the rare / common query terms


def zipf_cdf(vocab, device):
    p = 1.0 / torch.arange(1, vocab + 1, dtype=torch.float64, device=device)
    return torch.cumsum(p / p.sum(), 0).float()


def build_postings(n, vocab, device, slab=1 << 19):
    """BM25Postings of n Zipf documents, and their term document counts."""
    from nornicdb_amd.ops import BM25Postings
    cdf = zipf_cdf(vocab, device)
    g = torch.Generator(device=device).manual_seed(0)
    keys, doc_len = [], []
    for d0 in range(0, n, slab):
        rows = min(slab, n - d0)
        ln = torch.randint(32, 97, (rows,), device=device, generator=g)
        u = torch.rand(rows, 96, device=device, generator=g)
        term = torch.searchsorted(cdf, u).clamp_max(vocab - 1)
        doc = torch.arange(d0, d0 + rows, device=device)[:, None]
        keep = torch.arange(96, device=device)[None, :] < ln[:, None]
        keys.append((term * n + doc)[keep])
        doc_len.append(ln)
    key, tf = torch.unique(torch.cat(keys), sorted=True, return_counts=True)
    del keys
    term = key // n
    df = torch.bincount(term, minlength=vocab)
    off = torch.zeros(vocab + 1, dtype=torch.int64, device=device)
    off[1:] = torch.cumsum(df, 0)
    post = BM25Postings(off, (key - term * n).to(torch.int32).contiguous(),
                        tf.to(torch.int32).contiguous(),
                        torch.cat(doc_len).to(torch.int32).contiguous(), n)
    return post, df.cpu()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--docs", type=int, default=4_000_000)
    p.add_argument("--vocab", type=int, default=100_000)
    p.add_argument("--host-docs", type=int, default=200_000)
    p.add_argument("--iters", type=int, default=50, help="calls per sample")
    p.add_argument("--repeats", type=int, default=7, help="samples per variant")
    p.add_argument("--host-iters", type=int, default=3,
                   help="calls per sample of part 2")
    p.add_argument("--skip-kernel", action="store_true", help="part 2 only")
    p.add_argument("--skip-index", action="store_true", help="part 1 only")
    p.add_argument("--rehearse", action="store_true",
                   help="run the host logic on the CPU at a tiny shape")
    args = p.parse_args()

    from nornicdb_amd import ops
    from nornicdb_amd.ops import bm25_search
    from nornicdb_amd.search.bm25 import FulltextIndex
    from nornicdb_amd.search.bm25_device import DeviceFulltextIndex

    if args.rehearse:
        device = torch.device("cpu")
        args.docs, args.host_docs = min(args.docs, 20000), \
            min(args.host_docs, 2000)
        args.iters, args.repeats, args.host_iters = 2, 2, 1
    else:
        if not torch.cuda.is_available():
            sys.exit("bm25_bench: needs a GPU (or --rehearse)")
        ops.require_native()
        device = torch.device("cuda:0")
    on_gpu = device.type == "cuda"
    note = "" if on_gpu else " (REHEARSAL: not a measurement)"

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    def timed(fn):
        """ms per call over args.iters calls."""
        if on_gpu:
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / args.iters
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    report = {"device": str(device), "rehearsal": not on_gpu}

    # ---- part 1: the kernel ----
    if not args.skip_kernel:
        n, vocab = args.docs, args.vocab
        t0 = time.perf_counter()
        post, df = build_postings(n, vocab, device)
        sync()
        build_s = time.perf_counter() - t0
        avg_len = float(post.doc_len.double().mean())
        c0, c1 = K1 * (1 - B), K1 * B / avg_len
        idf = torch.log(1 + (n - df.double() + 0.5) / (df.double() + 0.5))

        variants, meta = {}, {}
        for kind, first in (("rare", min(RARE, vocab // 2)),
                            ("common", COMMON)):
            for t in (1, 4, 8):
                for qn in (1, 16):
                    # query r takes ranks first + r*t .. first + (r+1)*t
                    ids = first + torch.arange(qn * t).view(qn, t)
                    w = (idf[ids] * (K1 + 1)).float()
                    postings = int(df[ids].sum())
                    q_terms = ids.to(torch.int32).to(device)
                    q_w = w.to(device)
                    for k in (10, 40):
                        name = f"{kind} T={t} Q={qn} k={k}"
                        meta[name] = {"postings": postings,
                                      "bytes": postings * 12}
                        variants[name] = (
                            lambda q_terms=q_terms, q_w=q_w, k=k: bm25_search(
                                post, q_terms, q_w, c0, c1, k))
                        s, i = variants[name]()
                        assert s.shape == (qn, k)
                        assert (i[:, 0] >= 0).all(), name
        for fn in variants.values():          # warm every variant
            for _ in range(3):
                fn()
        sync()
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                samples[name].append(timed(fn))
        print(f"# bm25_search: {n} documents, mean length {avg_len:.1f}, "
              f"V={vocab}, M={post.post_doc.shape[0]} postings, "
              f"{args.iters} calls/sample, {args.repeats} samples, "
              f"device={device}, postings built in {build_s:.1f} s{note}")
        print("| variant | postings | ms/call median | min..max | MB | GB/s |")
        print("|---|---|---|---|---|---|")
        out = []
        for name, xs in samples.items():
            med = statistics.median(xs)
            nb = meta[name]["bytes"]
            print(f"| {name} | {meta[name]['postings']} | {med:.4f} | "
                  f"{min(xs):.4f}..{max(xs):.4f} | {nb / 1e6:.2f} | "
                  f"{nb / med / 1e6:.0f} |")
            out.append({"variant": name, "ms_median": round(med, 5),
                        "ms_min": round(min(xs), 5),
                        "ms_max": round(max(xs), 5), **meta[name]})
        report["kernel"] = {"docs": n, "vocab": vocab,
                            "postings": int(post.post_doc.shape[0]),
                            "results": out}
        del post, variants

    # ---- part 2: host index against device index ----
    if not args.skip_index:
        n, vocab = args.host_docs, 20000
        rng = np.random.default_rng(0)
        cdf = zipf_cdf(vocab, torch.device("cpu")).numpy()
        ft = FulltextIndex()
        t0 = time.perf_counter()
        for d in range(n):
            ln = int(rng.integers(32, 97))
            ranks = np.minimum(np.searchsorted(cdf, rng.random(ln)), vocab - 1)
            ft.index(f"d{d}", " ".join(f"t{r}" for r in ranks))
        host_s = time.perf_counter() - t0
        dev = DeviceFulltextIndex(ft, device=str(device))
        t0 = time.perf_counter()
        dev.build()
        sync()
        dev_s = time.perf_counter() - t0
        rare0 = min(RARE, vocab) // 2
        queries = {
            "common T=1": f"t{COMMON}",
            "common T=4": " ".join(f"t{COMMON + j}" for j in range(4)),
            "common T=8": " ".join(f"t{COMMON + j}" for j in range(8)),
            "rare T=1": f"t{rare0}",
            "rare T=4": " ".join(f"t{rare0 + j}" for j in range(4)),
        }

        def clock(fn):
            t0 = time.perf_counter()
            for _ in range(args.host_iters):
                fn()
            return (time.perf_counter() - t0) * 1e3 / args.host_iters

        for q in queries.values():            # warm
            ft.search(q, 40)
            dev.search(q, 40)
        host = {name: [] for name in queries}
        devs = {name: [] for name in queries}
        for _ in range(args.repeats):
            for name, q in queries.items():
                host[name].append(clock(lambda q=q: ft.search(q, 40)))
                devs[name].append(clock(lambda q=q: dev.search(q, 40)))
        print(f"# FulltextIndex.search vs DeviceFulltextIndex.search: {n} "
              f"documents, k=40, {args.host_iters} calls/sample, "
              f"{args.repeats} samples, host clock, device={device}; host "
              f"index built in {host_s:.1f} s, device index in {dev_s:.1f} s"
              f"{note}")
        print("| query | host ms median | host min..max | device ms median | "
              "device min..max | device median < host min |")
        print("|---|---|---|---|---|---|")
        out, all_ok = [], True
        for name in queries:
            h, d = host[name], devs[name]
            ok = statistics.median(d) < min(h)
            if name.startswith("common"):
                all_ok &= ok
            print(f"| {name} | {statistics.median(h):.3f} | {min(h):.3f}.."
                  f"{max(h):.3f} | {statistics.median(d):.3f} | {min(d):.3f}.."
                  f"{max(d):.3f} | {'yes' if ok else 'NO'} |")
            out.append({"query": name,
                        "host_ms_median": round(statistics.median(h), 4),
                        "host_ms_min": round(min(h), 4),
                        "device_ms_median": round(statistics.median(d), 4),
                        "device_ms_max": round(max(d), 4), "ok": ok})
        print("# condition (device median below host minimum on every "
              f"common-term query): {'met' if all_ok else 'NOT met'}")
        report["index"] = {"docs": n, "results": out, "condition_met": all_ok}

    print(json.dumps(report))


if __name__ == "__main__":
    main()
