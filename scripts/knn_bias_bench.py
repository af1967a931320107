#!/usr/bin/env python3
"""What the per-row score bias costs the brute-force kNN routes on one GPU.

Shape: 4M x 1024 bf16 (the shape ops/knn.py's dispatch was measured at),
k=10. Variants: `knn_search` at Q=1 (gemv kernel), Q=16 and Q=256 (MFMA
kernel), each without and with `row_bias` (fp32 [N], uniform in [-0.5, 0]:
the size of a Euclidean bias -|x|^2/2 over rows of norm <= 1). The biased
call reads 4 B more per 2 KB row.

Timing as in scripts/ivf_bench.py: device events around `--iters`
back-to-back calls per sample, after a warm-up of every variant; the
variants alternate inside each of `--repeats` rounds. The table gives the
median sample and min..max in ms per call, and the corpus bytes over the
median. A run without a GPU is refused unless --rehearse is given.

`--root DIR` imports nornicdb_amd from another tree, to time another build
of the package with the same script; a build whose knn_search takes no
`row_bias` is timed without the biased variants.
"""

import argparse
import inspect
import json
import os
import statistics
import sys

import torch


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=4_000_000)
    p.add_argument("--dim", type=int, default=1024)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--iters", type=int, default=50, help="calls per sample")
    p.add_argument("--repeats", type=int, default=7, help="samples per variant")
    p.add_argument("--root", default=os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), help="tree to import nornicdb_amd from")
    p.add_argument("--rehearse", action="store_true",
                   help="run the host logic on the CPU at a tiny shape")
    args = p.parse_args()

    sys.path.insert(0, os.path.abspath(args.root))
    from nornicdb_amd import ops
    from nornicdb_amd.ops import knn_search, knn_search_exact

    has_bias = "row_bias" in inspect.signature(knn_search).parameters

    if args.rehearse:
        device = torch.device("cpu")
        args.rows, args.iters, args.repeats = min(args.rows, 4096), 2, 2
    else:
        if not torch.cuda.is_available():
            sys.exit("knn_bias_bench: needs a GPU (or --rehearse)")
        ops.require_native()
        device = torch.device("cuda:0")
    on_gpu = device.type == "cuda"

    n, d, k = args.rows, args.dim, args.k
    db = torch.empty(n, d, device=device, dtype=torch.bfloat16)
    ops.fill_random_unit_(db)
    if not on_gpu:
        db = db.float()
    g = torch.Generator(device=device).manual_seed(0)
    bias = -0.5 * torch.rand(n, device=device, generator=g)

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

    variants = {}
    for qn in (1, 16, 256):
        gq = torch.Generator(device=device).manual_seed(qn)
        q = torch.nn.functional.normalize(
            torch.randn(qn, d, device=device, generator=gq), dim=-1) \
            .to(db.dtype)
        variants[f"Q={qn} unbiased"] = lambda q=q: knn_search(db, q, k)
        if not has_bias:
            continue
        variants[f"Q={qn} biased"] = \
            lambda q=q: knn_search(db, q, k, row_bias=bias)
        # what is timed is also right: the biased hits against the fp32
        # reference on the corpus' first rows
        m = min(n, 1 << 16)
        s, i = knn_search(db[:m], q, k, row_bias=bias[:m])
        rs, ri = knn_search_exact(db[:m], q, k, row_bias=bias[:m])
        assert (s - rs).abs().max() <= 2e-2, "biased scores off"
        assert (i == ri).float().mean() >= 0.9, "biased hits off"

    for fn in variants.values():          # warm every variant
        for _ in range(3):
            fn()
    sync()
    samples = {name: [] for name in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            samples[name].append(timed(fn))

    full = n * d * 2
    med = {name: statistics.median(xs) for name, xs in samples.items()}
    print(f"# {n} x {d} bf16, k={k}, {args.iters} calls/sample, "
          f"{args.repeats} samples, device={device}, root={args.root}"
          + ("" if has_bias else " (this build has no row_bias)")
          + (" (REHEARSAL: not a measurement)" if not on_gpu else ""))
    print("| variant | ms/call median | min..max | corpus GB/s |")
    print("|---|---|---|---|")
    out = []
    for name, xs in samples.items():
        print(f"| {name} | {med[name]:.4f} | {min(xs):.4f}..{max(xs):.4f} | "
              f"{full / med[name] / 1e6:.0f} |")
        out.append({"variant": name, "ms_median": round(med[name], 5),
                    "ms_min": round(min(xs), 5), "ms_max": round(max(xs), 5)})
    print(json.dumps({"rows": n, "dim": d, "k": k, "device": str(device),
                      "rehearsal": not on_gpu, "row_bias": has_bias,
                      "results": out}))


if __name__ == "__main__":
    main()
