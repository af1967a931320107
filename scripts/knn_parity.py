#!/usr/bin/env python3
"""Bit-level record of what every kNN / IVF route returns, to compare two
builds of the package (a refactor against its parent commit).

    python scripts/knn_parity.py --out A.npz        # in each tree
    python scripts/knn_parity.py --compare A.npz B.npz

Inputs are seeded and generated on the device, so two trees on one machine
see identical bytes. Routes recorded, scores and ids each: gemv (Q=1 and
Q=8, plain and with mask + bias), bf16 MFMA (Q=100: plain, mask, bias, mask
+ bias), fp8 and int8 MFMA (Q=100, plain and masked), and the IVF scan over
bf16 / int8 / fp8 at k=10 and k=32 (Q=1 and Q=5, masked). Corpus heights
leave a tail behind the last kernel panel and give every block several
panels. --compare exits 1 unless every array is bit-equal (floats are
compared by their bits, so -inf and equal-looking roundings count).

A run without a GPU is refused unless --rehearse (tiny shape through the
CPU routes) is given.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for name in bad:
        print(f"MISSING in one file: {name}")
    for name in sorted(set(a.files) & set(b.files)):
        x, y = a[name], b[name]
        same = x.shape == y.shape and x.dtype == y.dtype and \
            x.tobytes() == y.tobytes()
        print(f"{'equal' if same else 'DIFFERENT':9s} {name} "
              f"{x.dtype}{list(x.shape)}")
        if not same:
            bad.append(name)
    print(f"{len(a.files)} arrays, {len(bad)} differ")
    return 1 if bad else 0


def record(device, n, d, n_ivf):
    from nornicdb_amd.ops import IVFLists, ivf_search
    from nornicdb_amd.ops.knn import (knn_search, knn_search_int8,
                                      quantize_fp8, quantize_int8)

    g = torch.Generator(device=device).manual_seed(0x6E6F726E)

    def unit(rows):
        return torch.nn.functional.normalize(
            torch.randn(rows, d, device=device, generator=g), dim=-1)

    out = {}

    def keep(name, si):
        if device.type == "cuda":
            torch.cuda.synchronize()
        out[name + "_scores"] = si[0].cpu().numpy()
        out[name + "_ids"] = si[1].cpu().numpy()

    x = unit(n)
    q = unit(100)
    allow = torch.rand(n, device=device, generator=g) < 0.3
    bias = -0.5 * torch.rand(n, device=device, generator=g)
    xb = x.to(torch.bfloat16) if device.type == "cuda" else x
    row_base = 1 << 33

    for qn in (1, 8):
        keep(f"gemv_q{qn}", knn_search(xb, q[:qn].to(xb.dtype), 10, row_base))
        keep(f"gemv_q{qn}_mask_bias",
             knn_search(xb, q[:qn].to(xb.dtype), 16, row_base, allow=allow,
                        row_bias=bias))
    for name, kw in (("", {}), ("_mask", {"allow": allow}),
                     ("_bias", {"row_bias": bias}),
                     ("_mask_bias", {"allow": allow, "row_bias": bias})):
        keep("mfma" + name, knn_search(xb, q.to(xb.dtype), 10, row_base, **kw))
    x8 = quantize_fp8(x)
    keep("fp8", knn_search(x8, q, 10, row_base))
    keep("fp8_mask", knn_search(x8, q, 10, row_base, allow=allow))
    xi, sa = quantize_int8(x)
    keep("int8", knn_search_int8(xi, sa, q, 10, row_base))
    keep("int8_mask", knn_search_int8(xi, sa, q, 10, row_base, allow=allow))

    # IVF: a random permutation of the rows below tail_start cut into 64
    # lists of random lengths; 8 random probes per query
    tail_start = n_ivf - 37
    cuts = torch.sort(torch.randint(0, tail_start + 1, (63,), device=device,
                                    generator=g)).values
    off = torch.cat([cuts.new_zeros(1), cuts,
                     cuts.new_full((1,), tail_start)]).to(torch.int32)
    rows = torch.randperm(tail_start, device=device, generator=g) \
        .to(torch.int32)
    max_len = int((off[1:] - off[:-1]).max())
    lists = IVFLists(torch.zeros(64, 8, device=device), off, rows,
                     tail_start, max_len)
    stores = {"bf16": (xb[:n_ivf], None), "int8": (xi[:n_ivf], sa[:n_ivf]),
              "fp8": (x8[:n_ivf], None)}
    for qn in (1, 5):
        probes = torch.randint(0, 64, (qn, 8), device=device, generator=g) \
            .to(torch.int32)
        for fmt, (db, scales) in stores.items():
            for k in (10, 32):
                keep(f"ivf_{fmt}_q{qn}_k{k}",
                     ivf_search(db.contiguous(), q[:qn], k, lists, probes,
                                tail_start, row_base=row_base,
                                allow=allow[:n_ivf].contiguous(),
                                scales=scales))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", help="write the routes' outputs to this .npz")
    p.add_argument("--compare", nargs=2, metavar=("A", "B"),
                   help="compare two recorded files bit by bit")
    p.add_argument("--rehearse", action="store_true",
                   help="run the host logic on the CPU at a tiny shape")
    args = p.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        p.error("give --out FILE or --compare A B")

    from nornicdb_amd import ops
    if args.rehearse:
        device = torch.device("cpu")
        n, d, n_ivf = 2007, 128, 1500
    else:
        if not torch.cuda.is_available():
            sys.exit("knn_parity: needs a GPU (or --rehearse)")
        ops.require_native()
        device = torch.device("cuda:0")
        # 4687 bf16 panels of 320 rows (18 per block at the default grid) /
        # 15625 quantised panels of 96 (2 per block), + 7 tail rows
        n, d, n_ivf = 1_500_007, 256, 60_000
    out = record(device, n, d, n_ivf)
    np.savez(args.out, **out)
    print(f"knn_parity: {len(out)} arrays -> {args.out}"
          + (" (REHEARSAL on the CPU)" if args.rehearse else ""))


if __name__ == "__main__":
    main()
