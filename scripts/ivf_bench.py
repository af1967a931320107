#!/usr/bin/env python3
"""IVF search vs brute force on one GPU.

Shape: 4M x 1024 bf16 (the shape ops/knn.py's dispatch was measured at),
C = optimal_k(N) = 1414 lists built by a few k-means iterations over the
corpus, k=10. Variants: `ivf_search` at Q=1 with nprobe 1 / 8 / 32 (and
nprobe 8 at k=40, the 64-entry top-k kernel), at Q=16 with nprobe 8, and
brute-force `knn_search` at Q=1 and Q=16 on the same tensor. For every IVF variant three things are timed on their own:
`ivf_route` (torch), `ivf_search` with the probes already made (scan +
merge kernels) and both together. Bytes scanned are the rows of the probed
lists times D*2, counted on the host from the CSR offsets outside the
timed window; GB/s is those bytes over the scan+merge time. The split
between the scan and merge kernels comes from a kernel trace of this
script, taken in a run of its own.

Timing: device events around `--iters` back-to-back calls per sample, after
a warm-up of every variant; the variants alternate inside each of
`--repeats` rounds. The table gives the median sample and min..max in ms
per call. A run without a GPU is refused unless --rehearse is given.

`--quant int8|fp8` quantises the same corpus (lists are still built from
the bf16 rows) and times, for every IVF variant, `ivf_search` (the fused
`ivf_scan_i8` / `ivf_scan_fp8` route, query quantisation included), the
kernel pair alone on a query quantised beforehand, and the torch gather
route (`ops.ivf._ivf_gather`) that scored these corpora before the kernels
existed. Bytes scanned are then rows times D (plus 4 per row for int8
scales).
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=4_000_000)
    p.add_argument("--dim", type=int, default=1024)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--kmeans-iters", type=int, default=4)
    p.add_argument("--iters", type=int, default=50, help="calls per sample")
    p.add_argument("--repeats", type=int, default=7, help="samples per variant")
    p.add_argument("--quant", choices=["bf16", "int8", "fp8"], default="bf16",
                   help="corpus format; int8 / fp8 also time the gather route")
    p.add_argument("--rehearse", action="store_true",
                   help="run the host logic on the CPU at a tiny shape")
    args = p.parse_args()

    from nornicdb_amd import ops
    from nornicdb_amd.ops import (ivf_build_lists, ivf_route, ivf_search,
                                  knn_search)
    from nornicdb_amd.ops.ivf import _ivf_gather, ivf_route_kind
    from nornicdb_amd.ops.knn import quantize_fp8, quantize_int8
    from nornicdb_amd.search.kmeans import kmeans, optimal_k

    if args.rehearse:
        device = torch.device("cpu")
        args.rows, args.iters, args.repeats = min(args.rows, 4096), 2, 2
    else:
        if not torch.cuda.is_available():
            sys.exit("ivf_bench: needs a GPU (or --rehearse)")
        ops.require_native()
        device = torch.device("cuda:0")
    on_gpu = device.type == "cuda"

    n, d, k = args.rows, args.dim, args.k
    db = torch.empty(n, d, device=device, dtype=torch.bfloat16)
    ops.fill_random_unit_(db)
    if not on_gpu:
        db = db.float()

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
        import time
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    import time
    c = optimal_k(n)
    t0 = time.perf_counter()
    cent, assign = kmeans(db, c, iters=args.kmeans_iters, seed=0)
    lists = ivf_build_lists(assign, cent.shape[0], n, cent)
    sync()
    build_s = time.perf_counter() - t0
    lens = (lists.list_off[1:] - lists.list_off[:-1]).cpu()

    quant = args.quant != "bf16"
    scales = None
    qdtype = db.dtype
    row_bytes = d * db.element_size()
    if quant:
        # quantise in slabs: the fp32 temporaries of a 4M-row corpus at once
        # would be several times the corpus
        store = torch.empty(n, d, device=device, dtype=torch.int8
                            if args.quant == "int8" else torch.float8_e4m3fn)
        if args.quant == "int8":
            scales = torch.empty(n, device=device)
        for r0 in range(0, n, 1 << 18):
            sl = slice(r0, min(r0 + (1 << 18), n))
            if args.quant == "int8":
                store[sl], scales[sl] = quantize_int8(db[sl])
            else:
                store[sl] = quantize_fp8(db[sl])
        db = store
        row_bytes = d + (4 if args.quant == "int8" else 0)
        sync()

    def search(q, kk, probes):
        return ivf_search(db, q, kk, lists, probes, n, scales=scales)

    def gather(q, kk, probes):
        return _ivf_gather(db, q, kk, lists, probes, n, 0, None, scales)

    def kernels_only(q, kk, probes):
        """The scan + merge pair on a query that is already quantised."""
        nat = ops.require_native()
        tail = (probes, lists.list_off, lists.list_rows, n, lists.max_len, 0,
                kk, None)
        if args.quant == "int8":
            qi, sq = quantize_int8(q)
            return lambda: nat.ivf_scan_i8(db, scales, qi, sq, *tail)
        qb = q.to(torch.float8_e4m3fn).view(torch.uint8)
        dbb = db.view(torch.uint8)
        return lambda: nat.ivf_scan_fp8(dbb, qb, *tail)

    variants = {}
    meta = {}
    for qn, nprobe in ((1, 1), (1, 8), (1, 32), (16, 8)):
        g = torch.Generator(device=device).manual_seed(qn)
        q = torch.nn.functional.normalize(
            torch.randn(qn, d, device=device, generator=g), dim=-1) \
            .to(qdtype)
        probes = ivf_route(lists, q, nprobe)
        rows = int(lens[probes.cpu().long()].sum())
        name = f"ivf Q={qn} nprobe={nprobe}"
        meta[name] = {"Q": qn, "nprobe": nprobe, "rows_scanned": rows,
                      "bytes_scanned": rows * row_bytes}
        variants[name + " route"] = \
            (lambda q=q, nprobe=nprobe: ivf_route(lists, q, nprobe))
        variants[name + " scan+merge"] = \
            (lambda q=q, probes=probes: search(q, k, probes))
        variants[name + " total"] = \
            (lambda q=q, nprobe=nprobe: search(
                q, k, ivf_route(lists, q, nprobe)))
        s, i = search(q, k, probes)
        assert s.shape == (qn, min(k, n)) and (i >= 0).all()
        ks = [k]
        if (qn, nprobe) == (1, 8):
            # hybrid search's over-fetch size: the K=64 instantiation
            meta[name + " k=40"] = dict(meta[name])
            variants[name + " k=40 scan+merge"] = \
                (lambda q=q, probes=probes: search(q, 40, probes))
            ks.append(40)
        for kk in ks if quant else ():
            tag = name + ("" if kk == k else f" k={kk}")
            meta.setdefault(tag, dict(meta[name]))
            if on_gpu:
                assert ivf_route_kind(db.dtype, d, kk) != "gather"
                variants[tag + " kernels"] = kernels_only(q, kk, probes)
            variants[tag + " gather"] = \
                (lambda q=q, probes=probes, kk=kk: gather(q, kk, probes))
            gs, gi = gather(q, kk, probes)
            ss, si = search(q, kk, probes)
            assert (gs - ss).abs().max() <= 1e-4, "routes disagree"
        if qn == 1:
            bq = q
        else:
            bq16 = q
    if not quant:
        variants["brute Q=1"] = lambda: knn_search(db, bq, k)
        variants["brute Q=16"] = lambda: knn_search(db, bq16, k)
        variants["brute Q=1 k=40"] = lambda: knn_search(db, bq, 40)
    full = n * d * db.element_size()

    for fn in variants.values():          # warm every variant
        for _ in range(3):
            fn()
    sync()
    samples = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            samples[name].append(timed(fn))

    med = {name: statistics.median(xs) for name, xs in samples.items()}
    print(f"# {n} x {d} {args.quant}, C={lists.n_lists} "
          f"(max list {lists.max_len}, mean {n / lists.n_lists:.0f}), "
          f"k={k}, {args.iters} calls/sample, {args.repeats} samples, device={device}, lists built in "
          f"{build_s:.1f} s"
          + (" (REHEARSAL: not a measurement)" if not on_gpu else ""))
    print("| variant | ms/call median | min..max | MB scanned | GB/s |")
    print("|---|---|---|---|---|")
    out = []
    for name, xs in samples.items():
        base = name.rsplit(" ", 1)[0]
        nbytes = None
        if name.endswith(("scan+merge", "kernels", "gather")):
            nbytes = meta[base]["bytes_scanned"]
        elif name.startswith("brute"):
            nbytes = full
        mb = "" if nbytes is None else f"{nbytes / 1e6:.1f}"
        gbs = "" if nbytes is None else f"{nbytes / med[name] / 1e6:.0f}"
        print(f"| {name} | {med[name]:.4f} | {min(xs):.4f}..{max(xs):.4f} | "
              f"{mb} | {gbs} |")
        out.append({"variant": name, "ms_median": round(med[name], 5),
                    "ms_min": round(min(xs), 5), "ms_max": round(max(xs), 5),
                    "bytes": nbytes})
    print(json.dumps({"rows": n, "dim": d, "k": k, "quant": args.quant,
                      "lists": lists.n_lists,
                      "max_len": lists.max_len, "device": str(device),
                      "rehearsal": not on_gpu, "variants": meta,
                      "results": out}))


if __name__ == "__main__":
    main()
