"""The centrality kernels of csrc/centrality.hip (msbfs_level, bc_forward,
bc_backward, bc_accumulate) through `_closeness_gpu` / `_betweenness_gpu`,
called directly so that the 50 000-edge rule of the public functions does
not hide the small shapes, against the CPU functions on the graphs of
tests/centrality_cases.py."""

import numpy as np
import pytest
import torch

from nornicdb_amd.graph import algos

import centrality_cases as cc

pytestmark = pytest.mark.gpu


def _betweenness(name, samples):
    g = cc.graph(name)
    sources, scale = algos._bc_sources(g.n, samples, cc.SEED)
    return algos._betweenness_gpu(g, sources, scale)


@pytest.mark.parametrize("set_name", list(cc.NODE_SETS))
@pytest.mark.parametrize("name", cc.CASES)
def test_closeness_is_bit_identical(name, set_name):
    """Integer level counts feed the same float64 quotient as the CPU path."""
    g = cc.graph(name)
    nodes = cc.nodes_of(name, set_name)
    got = algos._closeness_gpu(g, nodes)
    ref = cc.closeness_ref(name, set_name)
    assert got.dtype == np.float32 and got.shape == (g.n,)
    assert got.tobytes() == ref.tobytes(), \
        np.flatnonzero(got != ref)[:10].tolist()
    asked = np.zeros(g.n, bool)
    asked[nodes] = True
    assert (got[~asked] == 0).all()


@pytest.mark.parametrize("samples", cc.SAMPLES)
@pytest.mark.parametrize("name", cc.CASES)
def test_betweenness_within_bound(name, samples):
    got = _betweenness(name, samples)
    cc.check_betweenness(got, cc.betweenness_ref(name, samples))


def test_layered_sigma_is_beyond_fp32():
    """The layered case is finite on the device although its path counts
    reach 4^71; the CPU maximum is 5040."""
    got = _betweenness("layered", None)
    assert np.isfinite(got).all() and got.max() == 5040.0


@pytest.mark.parametrize("name", ["random", "layered"])
def test_betweenness_is_independent_of_the_batch(name, monkeypatch):
    g = cc.graph(name)
    monkeypatch.setenv("NORNICDB_BC_BATCH", str(20 * g.n))
    assert algos._bc_batch(g.n, g.n) == 1
    one = _betweenness(name, None)
    monkeypatch.delenv("NORNICDB_BC_BATCH")
    assert algos._bc_batch(g.n, g.n) == 32
    many = _betweenness(name, None)
    assert one.tobytes() == many.tobytes()


@pytest.mark.parametrize("name", ["random", "hub", "wide_hub", "layered"])
def test_two_calls_are_bit_identical(name):
    g = cc.graph(name)
    nodes = cc.nodes_of(name, "r130")
    assert algos._closeness_gpu(g, nodes).tobytes() == \
        algos._closeness_gpu(g, nodes).tobytes()
    assert _betweenness(name, 33).tobytes() == _betweenness(name, 33).tobytes()


# ---------------------------------------------------------------- bindings
def _ok_args(dev="cuda"):
    """Valid arguments of the four bindings on the one_way graph."""
    from nornicdb_amd.ops import require_native
    nat = require_native()
    g = cc.graph("one_way")
    n, nb = g.n, 3
    rp, ci = g.torch_csr(dev)
    i64 = dict(dtype=torch.int64, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    ms = [rp, ci, torch.zeros(n, **i64), torch.zeros(n, **i64),
          torch.zeros(n, **i64), torch.zeros(64, **i64), 7]
    dist = torch.full((nb, n), -1, dtype=torch.int32, device=dev)
    fw = [rp, ci, dist, torch.zeros(nb, n, **f64),
          torch.zeros(1, dtype=torch.int32, device=dev), 0]
    bw = [rp, ci, dist, torch.zeros(nb, n, **f64), torch.zeros(nb, n, **f64),
          0]
    ac = [torch.zeros(nb, n, **f64), torch.zeros(nb, **i64),
          torch.zeros(n, **f64)]
    return nat, n, nb, {"msbfs_level": ms, "bc_forward": fw,
                        "bc_backward": bw, "bc_accumulate": ac}


def test_bindings_accept_valid_arguments():
    nat, _, _, args = _ok_args()
    for fn, a in args.items():
        getattr(nat, fn)(*a)
    torch.cuda.synchronize()


def _tensor_slots(a):
    return [i for i, x in enumerate(a) if isinstance(x, torch.Tensor)]


def test_bindings_reject_wrong_dtypes():
    nat, _, _, args = _ok_args()
    for fn, a in args.items():
        for i in _tensor_slots(a):
            bad = list(a)
            bad[i] = a[i].to(torch.float32 if a[i].dtype != torch.float32
                             else torch.int32)
            with pytest.raises(RuntimeError):
                getattr(nat, fn)(*bad)


def test_bindings_reject_cpu_tensors():
    nat, _, _, args = _ok_args()
    for fn, a in args.items():
        for i in _tensor_slots(a):
            bad = list(a)
            bad[i] = a[i].cpu()
            with pytest.raises(RuntimeError):
                getattr(nat, fn)(*bad)


def test_bindings_reject_state_of_the_wrong_length():
    nat, n, nb, args = _ok_args()
    for fn, a in args.items():
        # every tensor after the CSR pair is state (bc_accumulate has no CSR)
        first = 0 if fn == "bc_accumulate" else 2
        for i in _tensor_slots(a)[first:]:
            for shape in ([s + 1 for s in a[i].shape],
                          [max(s - 1, 0) for s in a[i].shape]):
                bad = list(a)
                bad[i] = torch.zeros(shape, dtype=a[i].dtype, device="cuda")
                with pytest.raises(RuntimeError):
                    getattr(nat, fn)(*bad)
