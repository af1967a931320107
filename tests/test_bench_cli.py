"""bench.py command line: plain vs --full runs and --dump-outputs.

Runs the benchmark's main() in-process in CPU dev mode on a toy
configuration (1-layer tiny encoder, 2000-row corpus), so each case
takes well under a second."""

import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOY = ["--gpus", "1", "--device", "cpu", "--corpus", "2000", "--batch", "4",
       "--seq-len", "16", "--layers", "1", "--k", "5"]
NAMES = ["query_embeddings", "searched_embeddings", "topk_scores",
         "topk_indices"]


def _run(monkeypatch, capsys, *extra):
    monkeypatch.syspath_prepend(REPO)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *TOY, *extra])
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1, lines  # exactly one JSON result line
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_repeatable_outputs(
        monkeypatch, capsys, tmp_path):
    outs = []
    for d in ("a", "b"):
        r = _run(monkeypatch, capsys, "--steps", "3", "--warmup", "1",
                 "--dump-outputs", str(tmp_path / d))
        assert r["steps"] == 3 and r["warmup"] == 1
        assert r["ms_per_step"] > 0
        assert r["value"] == pytest.approx(4 / (r["ms_per_step"] / 1000),
                                           rel=1e-2)
        for key in ("metric", "unit", "higher_is_better", "dtype"):
            assert key in r
        # the recall check belongs to --full
        assert r["config"]["recall_at_k_vs_fp32_exact"] is None
        assert sorted(os.listdir(tmp_path / d)) == sorted(
            n + ".npy" for n in NAMES)
        outs.append({n: np.load(tmp_path / d / (n + ".npy")) for n in NAMES})
    a, b = outs
    assert a["query_embeddings"].dtype == np.float32
    assert a["topk_scores"].dtype == np.float32
    assert a["topk_indices"].dtype == np.float64
    assert a["topk_scores"].shape == a["topk_indices"].shape == (4, 5)
    assert a["query_embeddings"].shape == a["searched_embeddings"].shape
    # same arguments -> same inputs -> same outputs, run after run
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
    # the dumped top-k really is the top-k of the dumped queries: scores
    # sorted descending, row ids inside the corpus
    assert (np.diff(a["topk_scores"], axis=1) <= 1e-6).all()
    assert ((a["topk_indices"] >= 0) & (a["topk_indices"] < 2000)).all()


def test_full_run_checks_recall_and_sees_the_same_inputs(
        monkeypatch, capsys, tmp_path):
    plain = _run(monkeypatch, capsys, "--steps", "2", "--warmup", "1",
                 "--dump-outputs", str(tmp_path / "p"))
    full = _run(monkeypatch, capsys, "--steps", "2", "--warmup", "1",
                "--full", "--dump-outputs", str(tmp_path / "f"))
    assert plain["config"]["recall_at_k_vs_fp32_exact"] is None
    assert full["config"]["recall_at_k_vs_fp32_exact"] >= 0.95
    for n in NAMES:
        assert np.array_equal(np.load(tmp_path / "p" / (n + ".npy")),
                              np.load(tmp_path / "f" / (n + ".npy"))), n


def test_dump_samples_large_outputs_within_budget(monkeypatch, tmp_path):
    monkeypatch.syspath_prepend(REPO)
    import bench
    import torch
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    big = torch.arange(10_000, dtype=torch.int64)
    small = torch.ones(3, 2, dtype=torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = (np.load(tmp_path / d / "big.npy") for d in ("a", "b"))
    assert a.dtype == np.float64 and a.nbytes <= 2048
    assert np.array_equal(a, b)            # fixed, seeded sample
    assert np.isin(a, big.numpy()).all()
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 2)
