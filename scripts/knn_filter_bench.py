#!/usr/bin/env python3
"""Filtered vs unfiltered kNN call time on one GPU.

Shape: the one the dispatch comment in ops/knn.py was measured at —
4M x 1024 bf16, k=10, Q=1 (gemv kernel) and Q=256 (MFMA kernel). For each
Q the same corpus and queries are searched without a mask and with packed
allow-masks of four kinds: 100 %, 50 % and 1 % random rows, and 1 % as one
contiguous run. The mask is packed once outside the timed window (an index
keeps it packed between searches); pack time is reported on its own line.

Timing: device events around `--iters` back-to-back calls per sample, after
a warm-up of every variant; the variants alternate inside each of
`--repeats` rounds so drift on a shared host hits all of them alike. The
table gives the median sample and the min..max spread in ms per call.
A run without a GPU is refused unless --rehearse (tiny shape, no timings
worth reading) is given.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def make_masks(n, device, seed=0x6E6F726E):
    g = torch.Generator(device=device).manual_seed(seed)
    r = torch.rand(n, device=device, generator=g)
    run = torch.zeros(n, dtype=torch.bool, device=device)
    start = n // 3
    run[start:start + n // 100] = True
    return {
        "100% (all ones)": torch.ones(n, dtype=torch.bool, device=device),
        "50% random": r < 0.5,
        "1% random": r < 0.01,
        "1% contiguous": run,
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=4_000_000)
    p.add_argument("--dim", type=int, default=1024)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--iters", type=int, default=20, help="calls per sample")
    p.add_argument("--repeats", type=int, default=7, help="samples per variant")
    p.add_argument("--rehearse", action="store_true",
                   help="run the host logic on the CPU at a tiny shape")
    args = p.parse_args()

    from nornicdb_amd import ops
    from nornicdb_amd.ops.knn import knn_search, pack_allow_mask

    if args.rehearse:
        device = torch.device("cpu")
        args.rows, args.iters, args.repeats = min(args.rows, 4096), 2, 2
    else:
        if not torch.cuda.is_available():
            sys.exit("knn_filter_bench: needs a GPU (or --rehearse)")
        ops.require_native()
        device = torch.device("cuda:0")
    on_gpu = device.type == "cuda"

    n, d, k = args.rows, args.dim, args.k
    db = torch.empty(n, d, device=device, dtype=torch.bfloat16)
    ops.fill_random_unit_(db)
    if not on_gpu:
        db = db.float()

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

    bools = make_masks(n, device)
    pack_ms = timed(lambda: pack_allow_mask(bools["50% random"]))
    masks = {name: pack_allow_mask(b) for name, b in bools.items()}
    density = {name: float(b.float().mean()) for name, b in bools.items()}

    rows_out = []
    for qn in (1, 256):
        g = torch.Generator(device=device).manual_seed(qn)
        q = torch.nn.functional.normalize(
            torch.randn(qn, d, device=device, generator=g), dim=-1).to(db.dtype)
        variants = {"unfiltered": lambda: knn_search(db, q, k)}
        for name, w in masks.items():
            variants[name] = (lambda w=w: knn_search(db, q, k, allow=w))
        # results must agree where they can: all-ones mask == no mask
        s0, i0 = variants["unfiltered"]()
        s1, i1 = variants["100% (all ones)"]()
        assert torch.equal(i0, i1) and torch.equal(s0, s1)
        for fn in variants.values():      # warm every variant
            for _ in range(3):
                fn()
        if on_gpu:
            torch.cuda.synchronize()
        samples = {name: [] for name in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                samples[name].append(timed(fn))
        base = statistics.median(samples["unfiltered"])
        for name, xs in samples.items():
            med = statistics.median(xs)
            rows_out.append({
                "Q": qn, "mask": name,
                "density": density.get(name, 1.0),
                "ms_median": round(med, 4), "ms_min": round(min(xs), 4),
                "ms_max": round(max(xs), 4),
                "vs_unfiltered": round(med / base, 3),
                # bytes of the rows a perfect filter would still have to read
                "allowed_TBps": round(
                    density.get(name, 1.0) * n * d * 2 / med / 1e9, 3),
            })

    print(f"# {n} x {d} bf16, k={k}, {args.iters} calls/sample, "
          f"{args.repeats} samples, device={device}"
          + (" (REHEARSAL: not a measurement)" if not on_gpu else ""))
    print(f"# pack_allow_mask({n} bools): {pack_ms:.3f} ms")
    print("| Q | mask | ms/call median | min..max | vs unfiltered |")
    print("|---|---|---|---|---|")
    for r in rows_out:
        print(f"| {r['Q']} | {r['mask']} | {r['ms_median']:.3f} | "
              f"{r['ms_min']:.3f}..{r['ms_max']:.3f} | "
              f"{r['vs_unfiltered']:.2f}x |")
    print(json.dumps({"rows": n, "dim": d, "k": k, "device": str(device),
                      "rehearsal": not on_gpu, "pack_ms": round(pack_ms, 4),
                      "results": rows_out}))


if __name__ == "__main__":
    main()
