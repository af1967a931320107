#!/usr/bin/env python3
"""NornicDB-AMD flagship benchmark: end-to-end embed -> kNN serving step.

Measures the BASELINE.json north-star metric on MI355X:
  kNN QPS @ recall>=0.95 over a 100M x 1024 bge-m3-shaped corpus
  (+ embed docs/sec), 1/2/4/8 GPUs.

One step (per rank) =
  1. generate a fresh batch of B synthetic docs (random token ids, seq S)
  2. embed them with the bge-m3 encoder (bf16) -> B query vectors
  3. all-gather queries across ranks (RCCL over xGMI)
  4. score ALL world*B queries against the local corpus shard (fused HIP
     kNN / tiled hipBLASLt GEMM + top-k)
  5. exchange per-shard top-k and merge the final top-k for own queries

The corpus is FIXED at --corpus total vectors (default 100M x 1024 bf16,
the BASELINE config) and sharded across ranks; per-GPU scoring work is
world*B queries x corpus/world rows = B x corpus = constant, and per-GPU
embed work is B docs = constant, so this is weak scaling (per-GPU work
fixed; QPS should scale ~linearly with N).

A plain run sets up, warms up, times --steps steps and prints one JSON
result line. --dump-outputs DIR also writes what the last timed step
returned (query embeddings, top-k scores and row ids) as DIR/<name>.npy;
the seeds are fixed, so equal arguments give equal inputs run after run.

With --full, recall is measured (untimed, after the timed steps) against
full-precision fp32 exact search over the full corpus for a sample of
queries, and the embed/search phase split is printed; brute-force scoring
makes >=0.95 structural, the check guards the bf16 kernels. Without --full
the result line reports recall_at_k_vs_fp32_exact as null.

Data is synthetic (no network in the environment); encoder weights are
random-init at the exact bge-m3 / XLM-R-large shape.
"""

import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist


def log(rank, *a):
    if rank == 0:
        print(*a, file=sys.stderr, flush=True)


DUMP_BUDGET_BYTES = 64 << 20  # all --dump-outputs files together


def dump_outputs(out_dir, arrays):
    """Write {name: tensor} as out_dir/<name>.npy. Floating tensors are
    stored as float32 (float64 stays float64), integer ones as float64
    (row ids < 2^53 are exact). An array over its share of the budget is
    replaced by a fixed, seeded sample of its flattened elements."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(len(arrays), 1)
    for name, t in arrays.items():
        t = t.detach()
        wide = t.dtype == torch.float64 or not t.dtype.is_floating_point
        itemsize = 8 if wide else 4
        if t.numel() * itemsize > share:
            pick = np.sort(np.random.default_rng(0x6E6F726E).integers(
                0, t.numel(), size=share // itemsize))
            t = t.reshape(-1)[torch.from_numpy(pick).to(t.device)]
        a = t.to(torch.float64 if wide else torch.float32).cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)


def setup_dist(args):
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:
        rank = int(os.environ["RANK"])
        world = int(os.environ["WORLD_SIZE"])
        local_rank = int(os.environ.get("LOCAL_RANK", rank))
        backend = "nccl" if torch.cuda.is_available() else "gloo"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=backend)
        if torch.cuda.is_available():
            torch.cuda.set_device(local_rank)
        return rank, world, local_rank
    return 0, 1, 0


def build_corpus(n_rows, dim, device, row_base, seed=0x6E6F726E):
    """Allocate and fill the local shard with unit-norm synthetic vectors."""
    from nornicdb_amd.ops import fill_random_unit_

    shard = torch.empty(n_rows, dim, device=device, dtype=torch.bfloat16)
    # fill in slices to bound kernel grid sizes / allocator pressure
    step = 16 << 20
    for s in range(0, n_rows, step):
        e = min(s + step, n_rows)
        fill_random_unit_(shard[s:e], row_base=row_base + s, seed=seed)
    return shard


def exact_fp32_topk_regen(n_rows, dim, device, q, k, row_base,
                          chunk=1 << 20):
    """fp32 exact top-k against the TRUE corpus values, regenerated
    deterministically per chunk (used by --quant modes, where the stored
    corpus is quantized and the bf16 original is not kept)."""
    from nornicdb_amd.ops import fill_random_unit_
    best_s = best_i = None
    qf = q.float()
    tmp = torch.empty(chunk, dim, device=device, dtype=torch.bfloat16)
    for s in range(0, n_rows, chunk):
        e = min(s + chunk, n_rows)
        t = tmp[:e - s]
        fill_random_unit_(t, row_base=row_base + s)
        sc = qf @ t.float().T
        kk = min(k, e - s)
        bs, bi = torch.topk(sc, kk, dim=-1)
        bi = bi + (row_base + s)
        if best_s is None:
            best_s, best_i = bs, bi
        else:
            cs = torch.cat([best_s, bs], -1)
            ci = torch.cat([best_i, bi], -1)
            best_s, sel = torch.topk(cs, min(k, cs.shape[-1]), -1)
            best_i = torch.gather(ci, -1, sel)
    return best_s, best_i


def build_corpus_int8(n_rows, dim, device, row_base):
    """Build the shard directly as symmetric int8 + per-row scales —
    slice-wise so the transient bf16 stays bounded (~32 GB) and the
    1 B/element corpus fits alongside it."""
    from nornicdb_amd.ops import fill_random_unit_
    from nornicdb_amd.ops.knn import quantize_int8
    shard = torch.empty(n_rows, dim, device=device, dtype=torch.int8)
    scales = torch.empty(n_rows, device=device, dtype=torch.float32)
    # small slices: quantize_int8 makes fp32 transients (~3x slice bytes)
    step = 2 << 20
    tmp = torch.empty(min(step, n_rows), dim, device=device,
                      dtype=torch.bfloat16)
    for s in range(0, n_rows, step):
        e = min(s + step, n_rows)
        t = tmp[:e - s]
        fill_random_unit_(t, row_base=row_base + s)
        qi, sc = quantize_int8(t)
        shard[s:e] = qi
        scales[s:e] = sc
    del tmp
    torch.cuda.empty_cache()
    return shard, scales


def exact_fp32_topk(shard, q, k, row_base, chunk=1 << 20):
    """fp32 exact top-k of q against the local bf16 shard (upcast per chunk)."""
    best_s = best_i = None
    qf = q.float()
    for s in range(0, shard.shape[0], chunk):
        e = min(s + chunk, shard.shape[0])
        sc = qf @ shard[s:e].float().T
        kk = min(k, e - s)
        bs, bi = torch.topk(sc, kk, dim=-1)
        bi = bi + (row_base + s)
        if best_s is None:
            best_s, best_i = bs, bi
        else:
            cs = torch.cat([best_s, bs], -1)
            ci = torch.cat([best_i, bi], -1)
            best_s, sel = torch.topk(cs, min(k, cs.shape[-1]), -1)
            best_i = torch.gather(ci, -1, sel)
    return best_s, best_i


def merge_global_topk(local_s, local_i, k, world):
    """all-gather per-shard top-k and merge. local_*: [Qg, k]."""
    if world == 1:
        return local_s, local_i
    gs = [torch.empty_like(local_s) for _ in range(world)]
    gi = [torch.empty_like(local_i) for _ in range(world)]
    dist.all_gather(gs, local_s.contiguous())
    dist.all_gather(gi, local_i.contiguous())
    cs = torch.cat(gs, dim=-1)
    ci = torch.cat(gi, dim=-1)
    s, sel = torch.topk(cs, k, dim=-1)
    return s, torch.gather(ci, -1, sel)


def search_step(shard, queries, k, row_base, world, scales=None):
    """Score queries (already gathered, [Qg, D]) vs local shard, merge top-k.
    scales!=None -> shard is a symmetric int8 corpus (--quant int8)."""
    from nornicdb_amd.ops import knn_search

    if scales is not None:
        from nornicdb_amd.ops.knn import knn_search_int8
        s, i = knn_search_int8(shard, scales, queries.float(), k,
                               row_base=row_base)
    else:
        s, i = knn_search(shard, queries, k, row_base=row_base)
    return merge_global_topk(s, i, k, world)


def graph_bench(args, rank, world, local_rank):
    """BASELINE config #4: PageRank on a 1B-edge synthetic CSR, sharded
    across ranks with halo-exchange contrib traffic (parallel/graph.py).
    Prints one JSON line (its own metric, separate from the kNN headline).
    """
    from nornicdb_amd.parallel.graph import pagerank_sharded, shard_rows

    use_cuda = torch.cuda.is_available() and args.device != "cpu"
    device = torch.device(args.device or ("cuda:%d" % local_rank if use_cuda else "cpu"))
    n, m = args.graph_nodes, args.graph_edges
    if device.type == "cpu" and m > 10_000_000:
        n, m = 100_000, 1_000_000  # CPU dev mode
    deg = m // n
    lo, hi = shard_rows(n, rank, world)
    n_local = hi - lo
    g = torch.Generator(device=device).manual_seed(4242 + rank)
    log(rank, f"[graph] building shard: {n_local} rows x deg {deg} "
              f"({n_local * deg * 4 / 1e9:.1f} GB col_idx) ...")
    row_ptr = torch.arange(n_local + 1, device=device, dtype=torch.int64) * deg
    col_idx = torch.randint(0, n, (n_local * deg,), device=device,
                            generator=g, dtype=torch.int32)
    # global out-degree histogram (once; all-reduced across shards)
    outdeg = torch.zeros(n, device=device, dtype=torch.float32)
    ones = torch.ones(1, device=device).expand(col_idx.numel())
    outdeg.scatter_add_(0, col_idx.long(), ones)
    if world > 1:
        dist.all_reduce(outdeg)
    log(rank, "[graph] warmup ...")
    pagerank_sharded(row_ptr, col_idx, outdeg, n, lo, iters=max(args.warmup, 1),
                     tol=0.0)
    if world > 1:
        dist.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.time()
    r = pagerank_sharded(row_ptr, col_idx, outdeg, n, lo, iters=args.steps,
                         tol=0.0)
    if device.type == "cuda":
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.time() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device if device.type == "cuda" else None)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # sanity: ranks sum to ~1
    total = float(r.sum()) if world == 1 else float(r.sum())
    iters_per_s = args.steps / elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"pagerank": r})
    if rank == 0:
        out = {
            "metric": "PageRank iterations/s on 1B-edge synthetic CSR (GPU-sharded, halo exchange)",
            "value": round(iters_per_s, 3),
            "unit": "iters/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000.0, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "fp32",
            "data": "synthetic (uniform random CSR, fixed out-degree)",
            "config": {
                "model": "apoc.algo.pageRank (BASELINE config #4)",
                "nodes": n, "edges": m, "parallelism": f"row-sharded CSR x{world}, halo all_to_all",
                "edges_per_s": round(m * args.steps / elapsed / 1e9, 2),
                "unit_edges_per_s": "GTEPS",
                "rank_sum": round(total, 6),
            },
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--corpus", type=int, default=100_000_000,
                   help="TOTAL corpus vectors, sharded across ranks")
    p.add_argument("--dim", type=int, default=1024)
    p.add_argument("--batch", type=int, default=256, help="docs embedded+queried per rank per step")
    p.add_argument("--seq-len", type=int, default=256)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--layers", type=int, default=24)
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run the untimed extras: "
                        "the recall check against fp32 exact search and the "
                        "embed/search phase breakdown (a plain run only "
                        "sets up, warms up, times --steps steps and prints)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write what the last timed step computed as "
                        "DIR/<name>.npy (float32/float64)")
    p.add_argument("--skip-recall", action="store_true",
                   help="with --full: leave out the recall check")
    p.add_argument("--quant", choices=["none", "int8"], default="none",
                   help="int8: 1 B/elem corpus scored by the i8 MFMA "
                        "kernel (2x capacity; NOT the headline config — "
                        "dtype is reported as int8)")
    p.add_argument("--timing", action="store_true",
                   help="print phase breakdown (implied by --full)")
    p.add_argument("--no-pipeline", action="store_true",
                   help="disable embed/search stream overlap (sequential steps)")
    p.add_argument("--recall-queries", type=int, default=8)
    p.add_argument("--device", default=None)
    p.add_argument("--graph", action="store_true",
                   help="run the 1B-edge PageRank bench (BASELINE config #4) instead")
    p.add_argument("--graph-nodes", type=int, default=100_000_000)
    p.add_argument("--graph-edges", type=int, default=1_000_000_000)
    args = p.parse_args()

    rank, world, local_rank = setup_dist(args)
    if args.graph:
        graph_bench(args, rank, world, local_rank)
        return
    if args.gpus > 1 and world == 1:
        print("ERROR: --gpus>1 requires torchrun (WORLD_SIZE env)", file=sys.stderr)
        sys.exit(2)

    use_cuda = torch.cuda.is_available() and args.device != "cpu"
    device = torch.device(args.device or ("cuda:%d" % local_rank if use_cuda else "cpu"))
    if device.type == "cpu" and args.corpus > 1_000_000:
        args.corpus = 200_000  # CPU dev mode
        args.batch = min(args.batch, 8)
        args.layers = 2

    from nornicdb_amd.models import BgeM3Config, BgeM3Encoder
    from nornicdb_amd import ops as nops

    if device.type == "cuda" and not nops.HAS_NATIVE:
        nops.require_native()  # fail loudly: no eager fallback on GPU

    torch.manual_seed(1234 + rank)

    # --- model (bge-m3 / XLM-R-large shape, random init) ---
    cfg = BgeM3Config(num_layers=args.layers) if device.type == "cuda" else \
        BgeM3Config.tiny(num_layers=args.layers)
    log(rank, f"[bench] building encoder ({cfg.num_layers} layers) ...")
    dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
    with device:
        model = BgeM3Encoder(cfg).init_small().to(device=device, dtype=dtype).eval()

    # --- corpus shard ---
    shard_rows = args.corpus // world
    row_base = rank * shard_rows
    log(rank, f"[bench] generating corpus shard {shard_rows}x{args.dim} bf16 "
              f"({shard_rows * args.dim * 2 / 1e9:.1f} GB/GPU) ...")
    t0 = time.time()
    if device.type == "cuda":
        if args.quant == "int8":
            shard, shard_scales = build_corpus_int8(
                shard_rows, args.dim, device, row_base)
        else:
            shard = build_corpus(shard_rows, args.dim, device, row_base)
            shard_scales = None
        torch.cuda.synchronize()
    else:
        shard = torch.empty(shard_rows, args.dim, dtype=torch.float32)
        from nornicdb_amd.ops import fill_random_unit_
        bf = torch.empty(shard_rows, args.dim, dtype=torch.bfloat16)
        fill_random_unit_(bf, row_base=row_base)
        shard = bf.float() if device.type == "cpu" else bf
        shard_scales = None
    log(rank, f"[bench] corpus ready in {time.time()-t0:.1f}s")

    vocab = cfg.vocab_size
    h = cfg.hidden_size
    assert h == args.dim or device.type == "cpu", "corpus dim must match encoder hidden"
    if device.type == "cpu":
        args.dim = h
        shard = shard[:, :h].contiguous() if shard.shape[1] >= h else torch.randn(shard_rows, h)
    if args.quant == "int8" and shard_scales is None:
        from nornicdb_amd.ops.knn import quantize_int8
        shard, shard_scales = quantize_int8(shard)

    def embed_batch():
        tokens = torch.randint(0, vocab, (args.batch, args.seq_len), device=device)
        with torch.no_grad():
            q = model(tokens)  # [B, H] fp32 normalized
        return q.to(torch.bfloat16 if shard_scales is not None
                    else shard.dtype)

    def gather_queries(q):
        if world > 1:
            gathered = [torch.empty_like(q) for _ in range(world)]
            dist.all_gather(gathered, q.contiguous())
            return torch.cat(gathered, 0)
        return q

    def one_step():
        qg = gather_queries(embed_batch())
        s, i = search_step(shard, qg, args.k, row_base, world,
                           scales=shard_scales)
        return qg, s, i

    # serving pipeline: embed batch t on one HIP stream while batch t-1 is
    # searched on another. Every query is still embedded AND searched; the
    # pipeline just has one batch of latency (steady-state serving shape).
    pipelined = device.type == "cuda" and not args.no_pipeline
    if pipelined:
        # NOTE (measured, MI355X/ROCm 7.2): the two phases do NOT overlap
        # in practice — step == embed + search exactly, with or without
        # stream priority, and capping the search grid to free CUs only
        # slows the search without admitting encoder workgroups. Both
        # phases are CU-limited, so there is no free capacity to overlap
        # into; the pipeline is kept for its serving shape (1-batch
        # latency) and for hardware where dispatch interleaves.
        s_embed = torch.cuda.Stream(priority=-1)
        s_search = torch.cuda.Stream()

        def pipe_step(prev_q):
            with torch.cuda.stream(s_embed):
                q_new = embed_batch()
            results = [None]
            with torch.cuda.stream(s_search):
                results[0] = search_step(shard, prev_q, args.k, row_base,
                                         world, scales=shard_scales)
            torch.cuda.synchronize()
            return gather_queries(q_new), results[0]

    # --- warmup ---
    log(rank, f"[bench] warmup x{args.warmup} ...")
    last_q = None
    for _ in range(args.warmup):
        last_q, _, _ = one_step()
    if pipelined:
        if last_q is None:  # --warmup 0: the pipeline still needs a batch
            last_q = gather_queries(embed_batch())
        last_q, _ = pipe_step(last_q)  # warm both streams
    if device.type == "cuda":
        torch.cuda.synchronize()

    # --- timed region ---
    if world > 1:
        dist.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    t_start = time.time()
    last_out = None  # what the last timed step returned (--dump-outputs)
    if pipelined:
        for _ in range(args.steps):
            searched_q = last_q
            last_q, (top_s, top_i) = pipe_step(last_q)
            last_out = (last_q, searched_q, top_s, top_i)
    else:
        for _ in range(args.steps):
            qg, top_s, top_i = one_step()
            last_out = (qg, qg, top_s, top_i)
    if device.type == "cuda":
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.time() - t_start

    # max over ranks
    if world > 1:
        t = torch.tensor([elapsed], device=device if device.type == "cuda" else None)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if args.dump_outputs and rank == 0 and last_out is not None:
        new_q, searched_q, top_s, top_i = last_out
        dump_outputs(args.dump_outputs, {
            # embeddings of the last step's fresh batch
            "query_embeddings": new_q,
            # the batch the last step searched (pipelined: the one before)
            # and its top-k over the corpus
            "searched_embeddings": searched_q,
            "topk_scores": top_s,
            "topk_indices": top_i,
        })

    # --- untimed extras (--full): phase breakdown + recall check. They run
    # after the timed steps so that these see the same random stream (hence
    # the same inputs) with and without --full. ---
    if (args.full or args.timing) and device.type == "cuda":
        def _t(fn, iters=5):
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            return (time.time() - t0) / iters * 1000

        tok = torch.randint(0, vocab, (args.batch, args.seq_len), device=device)
        with torch.no_grad():
            qf = model(tok).to(torch.bfloat16 if shard_scales is not None
                               else shard.dtype)

            ms_embed = _t(lambda: model(tok))
            ms_search = _t(lambda: search_step(shard, qf, args.k, row_base,
                                               world, scales=shard_scales))
        log(rank, f"[timing] embed {ms_embed:.1f} ms/batch ({args.batch/ms_embed*1000:.0f} docs/s)  "
                  f"search {ms_search:.1f} ms/batch ({args.batch/ms_search*1000:.0f} qps; "
                  f"{shard_rows*args.dim*2/ms_search/1e9:.2f} TB/s shard read)")

    # recall check (untimed): production path vs fp32 exact over full corpus
    recall = None
    if args.full and not args.skip_recall:
        nq = args.recall_queries
        tokens = torch.randint(0, vocab, (nq, args.seq_len), device=device,
                               generator=torch.Generator(device=device).manual_seed(99))
        with torch.no_grad():
            qr = model(tokens).to(torch.bfloat16 if shard_scales is not None
                                  else shard.dtype)
        if world > 1:
            dist.broadcast(qr, src=0)
        ps, pi = search_step(shard, qr, args.k, row_base, world,
                             scales=shard_scales)
        if shard_scales is not None and device.type == "cuda":
            # true pre-quantization values, regenerated deterministically
            # (the GPU fill kernel is row-indexed, so regen == builder)
            es, ei = exact_fp32_topk_regen(shard.shape[0], args.dim, device,
                                           qr, args.k, row_base)
        elif shard_scales is not None:
            # CPU dev mode: the fill fallback is not slice-invariant, so
            # score against the dequantized stored corpus instead
            deq = shard.float() * shard_scales[:, None]
            es, ei = exact_fp32_topk(deq, qr, args.k, row_base)
        else:
            es, ei = exact_fp32_topk(shard, qr, args.k, row_base)
        es, ei = merge_global_topk(es, ei, args.k, world)
        hit = 0
        for r in range(nq):
            hit += len(set(pi[r].tolist()) & set(ei[r].tolist()))
        recall = hit / (nq * args.k)
        log(rank, f"[bench] recall@{args.k} vs fp32 exact (full corpus): {recall:.4f}")

    total_queries = args.steps * args.batch * world
    qps = total_queries / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if rank == 0:
        baseline_qps = 1000.0  # reference: CUDA A100, 1M x 1024 corpus, 1 ms/query
        out = {
            "metric": "kNN QPS @ recall>=0.95 on 100Mx1024 bge-m3 vectors + embed docs/sec",
            "value": round(qps, 2),
            "unit": "queries/s (each query embedded by bge-m3 then searched over full corpus)",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(qps / baseline_qps, 3) if device.type == "cuda" else None,
            "dtype": ("int8 (opt-in quantized corpus; headline config is bf16)"
                      if args.quant == "int8" else
                      "bf16" if device.type == "cuda" else "fp32 (cpu dev mode)"),
            "data": "synthetic (deterministic unit-norm corpus; random token ids; random-init bge-m3 weights)",
            "config": {
                "model": "bge-m3 (XLM-R-large shape: 24L/1024h/16heads, random init)",
                "global_batch": args.batch * world,
                "seq_len": args.seq_len,
                "parallelism": f"shard{world} (corpus row-sharded, RCCL all-gather top-k merge)"
                               + ("; embed/search HIP-stream pipelined (1-batch latency)"
                                  if pipelined else ""),
                "corpus_vectors": args.corpus,
                "dim": args.dim,
                "k": args.k,
                "embed_docs_per_s": round(args.batch * world * args.steps / elapsed, 2),
                "recall_at_k_vs_fp32_exact": recall,
                "baseline_analogue": "A100 CUDA 1000 qps on 1Mx1024 (docs/features/gpu-acceleration.md)",
            },
        }
        print(json.dumps(out), flush=True)

    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
