"""The k-means kernels of csrc/kmeans.hip against float64, at all eight
dimensions the dispatch has, plus the argument checks of their wrappers and
search/kmeans.py end to end at d = 1536. Cases, references and bounds are
in tests/kernel_cases.py; each table also runs through the torch fp32 path
of search/kmeans.py on the CPU.
"""

import pytest
import torch

import kernel_cases as kc
from nornicdb_amd.search.kmeans import ClusterIndex, kmeans

ASSIGN_CASES = [(n, d) for d in kc.KM_DIMS for n in kc.KM_NS] + \
    [(kc.KM_STRIDE_N, 512)]


def _nat():
    from nornicdb_amd.ops import require_native
    return require_native()


# ---------------------------------------------------------------------------
# assign
# ---------------------------------------------------------------------------

def _torch_assign(x, cent, cnorm2):
    """The expression of the torch path of kmeans()."""
    xf, cf = x.float(), cent.float()
    d2 = (xf * xf).sum(-1, keepdim=True) + cnorm2[None] - 2.0 * (xf @ cf.T)
    m, a = d2.min(dim=1)
    return a, m.clamp_min(0)


@pytest.mark.parametrize("n,d", ASSIGN_CASES)
def test_kmeans_assign_bound_cpu(n, d):
    for k in kc.KM_KS:
        case = kc.assign_case(n, d, k)
        a, d2 = _torch_assign(*case[:3])
        kc.check_assign(f"cpu assign n{n} d{d} k{k}", a, d2, case, False)


@pytest.mark.gpu
@pytest.mark.parametrize("n,d", ASSIGN_CASES)
def test_kmeans_assign_gpu(n, d):
    nat = _nat()
    for k in kc.KM_KS:
        case = kc.assign_case(n, d, k)
        x, cent, cnorm2 = (t.cuda() for t in case[:3])
        a, d2 = nat.kmeans_assign(x, cent, cnorm2)
        assert a.dtype == torch.int32 and d2.dtype == torch.float32
        kc.check_assign(f"gpu assign n{n} d{d} k{k}", a, d2, case, True)


# ---------------------------------------------------------------------------
# accumulate, finalize
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", kc.ACCUM_CASES, ids=str)
def test_kmeans_accum_bound_cpu(case):
    x, assign, ref, bound, counts = kc.accum_case(*case)
    sums = torch.zeros(case[2], case[1])
    sums.index_add_(0, assign.long(), x.float())
    kc.check(f"cpu accum {case}", sums, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.ACCUM_CASES, ids=str)
def test_kmeans_accum_gpu(case):
    x, assign, ref, bound, ref_counts = kc.accum_case(*case)
    sums, counts = _nat().kmeans_accum(x.cuda(), assign.cuda(), case[2])
    assert torch.equal(counts.cpu(), ref_counts)
    kc.check(f"gpu accum {case}", sums, ref, bound)


@pytest.mark.parametrize("d", kc.FINALIZE_DIMS)
def test_kmeans_finalize_bound_cpu(d):
    sums, counts, old, new, b_new, drift, b_drift = kc.finalize_case(d)
    got = sums / counts.float().clamp_min(1)[:, None]
    got[counts == 0] = old[counts == 0]
    kc.check(f"cpu finalize d{d}", got, new, b_new)
    kc.check(f"cpu drift d{d}", ((got - old) ** 2).sum(-1), drift, b_drift)


@pytest.mark.gpu
@pytest.mark.parametrize("d", kc.FINALIZE_DIMS)
def test_kmeans_finalize_gpu(d):
    sums, counts, old, new, b_new, drift, b_drift = kc.finalize_case(d)
    got, drift2 = _nat().kmeans_finalize(sums.cuda(), counts.cuda(),
                                         old.cuda())
    kc.check(f"gpu finalize d{d}", got, new, b_new)
    kc.check(f"gpu drift d{d}", drift2, drift, b_drift)
    empty = counts == 0
    assert torch.equal(got.cpu()[empty], old[empty]), "empty cluster moved"
    assert (drift2.cpu()[empty] == 0).all()


# ---------------------------------------------------------------------------
# k-means++ min-distance update
# ---------------------------------------------------------------------------

def _check_pp(name, d2, start, ref, tol):
    d2 = d2.detach().cpu()
    even = torch.arange(kc.PP_N) % 2 == 0
    assert torch.equal(d2[even], start[even]), \
        f"{name}: an entry that was already smaller changed"
    err = (d2[~even].double() - ref[~even]).abs() / tol[~even]
    print(f"RATIO {name} {float(err.max()):.3f}")
    assert err.max() <= 1.0, f"{name}: row {2 * int(err.argmax()) + 1}"
    assert (d2 >= 0).all()
    for s in kc.PP_SEEDS:
        assert d2[s] <= tol[s]


@pytest.mark.parametrize("d", kc.KM_DIMS)
def test_kmeanspp_update_bound_cpu(d):
    x, start, ref, tol = kc.pp_case(d)
    xf = x.float()
    x_sq = (xf * xf).sum(-1)
    d2 = start.clone()
    for s in kc.PP_SEEDS:   # the expression of the torch path of _kmeanspp
        c = xf[s]
        nd = (x_sq + (c * c).sum() - 2.0 * (xf @ c)).clamp_min_(0)
        d2 = torch.minimum(d2, nd)
    _check_pp(f"cpu kmeanspp d{d}", d2, start, ref, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("d", kc.KM_DIMS)
def test_kmeanspp_update_gpu(d):
    nat = _nat()
    x, start, ref, tol = kc.pp_case(d)
    xg = x.cuda()
    d2 = start.cuda()
    for s in kc.PP_SEEDS:
        nat.kmeanspp_update(xg, xg[s].contiguous(),
                            float((x[s].double() ** 2).sum()), d2)
    _check_pp(f"gpu kmeanspp d{d}", d2, start, ref, tol)


# ---------------------------------------------------------------------------
# single-point update
# ---------------------------------------------------------------------------

class _Cpu:
    """kmeans_point_update through the torch path of ClusterIndex."""

    def __init__(self, cent, counts):
        self.ci = ClusterIndex()
        self.ci.centroids, self.ci.counts = cent, counts

    def __call__(self, cent, counts, v, c, sign):
        self.ci._point_update(c, v.float(), sign)


def _point_update_checks(update, cent, counts, v, name):
    """`update` changes cent and counts in place."""
    cent0, vf = cent.cpu().clone(), v.cpu().float()

    def state():
        return cent.cpu(), counts.cpu().tolist()

    # add to the empty cluster 0: the centroid becomes the point
    update(cent, counts, v, 0, 1)
    c, n = state()
    assert n == [1, 1, 7, 0]
    assert torch.equal(c[0], vf) and torch.equal(c[1:], cent0[1:])
    # remove it again: the count is 0, the centroid stays where it is
    update(cent, counts, v, 0, -1)
    c, n = state()
    assert n == [0, 1, 7, 0] and torch.equal(c[0], vf)
    # remove from count 0: stays 0
    update(cent, counts, v, 3, -1)
    c, n = state()
    assert n == [0, 1, 7, 0] and torch.equal(c[3], cent0[3])
    # add to and remove from the cluster of 7
    update(cent, counts, v, 2, 1)
    c, n = state()
    assert n == [0, 1, 8, 0]
    moved = (cent0[2].double() * 7 + vf.double()) / 8
    bound = kc.EPS_ACC * (cent0[2].double().abs() * 7 + vf.double().abs())
    kc.check(f"{name} add", c[2], moved, bound)
    update(cent, counts, v, 2, -1)
    c, n = state()
    assert n == [0, 1, 7, 0]
    kc.check(f"{name} add, remove", c[2], cent0[2].double(), bound)
    assert torch.equal(c[1], cent0[1]) and torch.equal(c[3], cent0[3])


@pytest.mark.parametrize("d", kc.POINT_DIMS)
def test_kmeans_point_update_bound_cpu(d):
    cent, counts, v = kc.point_case(d)
    cent, counts = cent.clone(), counts.clone()
    _point_update_checks(_Cpu(cent, counts), cent, counts, v,
                         f"cpu point d{d}")


@pytest.mark.gpu
@pytest.mark.parametrize("d", kc.POINT_DIMS)
def test_kmeans_point_update_gpu(d):
    cent, counts, v = kc.point_case(d)
    _point_update_checks(_nat().kmeans_point_update, cent.cuda(),
                         counts.cuda(), v.cuda(), f"gpu point d{d}")


# ---------------------------------------------------------------------------
# argument checks: a wrong dtype, shape or index is an exception, not an
# out-of-bounds access
# ---------------------------------------------------------------------------

@pytest.mark.gpu
def test_kmeans_argument_checks_gpu():
    nat = _nat()
    dev = "cuda"
    f32 = dict(device=dev, dtype=torch.float32)
    i32 = dict(device=dev, dtype=torch.int32)
    bf = dict(device=dev, dtype=torch.bfloat16)
    sums, counts, old = (torch.zeros(5, 8, **f32), torch.zeros(5, **i32),
                         torch.zeros(5, 8, **f32))
    nat.kmeans_finalize(sums, counts, old)       # the good call works
    for bad in [
        (sums.double(), counts, old),            # dtype
        (sums, counts.long(), old),
        (sums, counts, old.to(torch.bfloat16)),
        (sums, counts[:4], old),                 # shapes
        (sums, counts, old[:, :4].contiguous()),
        (sums.t().contiguous().t(), counts, old),   # not contiguous
        (sums[0], counts, old),                  # not 2-D
        (sums.cpu(), counts, old),
    ]:
        with pytest.raises(RuntimeError):
            nat.kmeans_finalize(*bad)

    cent, cnt, v = (torch.zeros(4, 512, **f32), torch.zeros(4, **i32),
                    torch.zeros(512, **bf))
    nat.kmeans_point_update(cent, cnt, v, 3, 1)
    for bad in [
        (cent, cnt, v, 4, 1),                    # c out of range
        (cent, cnt, v, -1, 1),
        (cent, cnt, v, 0, 2),                    # sign
        (cent, cnt, v.float(), 0, 1),            # dtypes
        (cent.to(torch.bfloat16), cnt, v, 0, 1),
        (cent, cnt.long(), v, 0, 1),
        (cent, cnt, v[:256], 0, 1),              # lengths
        (cent, cnt[:3], v, 0, 1),
        (cent, cnt, torch.zeros(1024, **bf)[::2], 0, 1),   # not contiguous
        (cent[0], cnt, v, 0, 1),
    ]:
        with pytest.raises(RuntimeError):
            nat.kmeans_point_update(*bad)
    assert cnt.tolist() == [0, 0, 0, 1]

    x, d2 = torch.zeros(6, 512, **bf), torch.zeros(6, **f32)
    nat.kmeanspp_update(x, v, 0.0, d2)
    for bad in [
        (x, v.float(), 0.0, d2),                 # seed dtype
        (x, v[:256], 0.0, d2),                   # seed length
        (x, torch.zeros(1024, **bf)[::2], 0.0, d2),
        (x, v, 0.0, d2.double()),                # d2 dtype
        (x, v, 0.0, d2[:5]),                     # d2 length
        (x, v, 0.0, d2.cpu()),
        (torch.zeros(6, 520, **bf), torch.zeros(520, **bf), 0.0, d2),
    ]:
        with pytest.raises(RuntimeError):
            nat.kmeanspp_update(*bad)

    a = torch.zeros(6, **i32)
    nat.kmeans_accum(x, a, 2)
    for bad in [(x, a.long(), 2), (x, a[:5], 2), (x, a, 0), (x, a.cpu(), 2)]:
        with pytest.raises(RuntimeError):
            nat.kmeans_accum(*bad)

    c2 = torch.zeros(3, 512, **bf)
    n2 = torch.zeros(3, **f32)
    nat.kmeans_assign(x, c2, n2)
    for bad in [(x, c2, n2.double()), (x, c2, n2[:2]), (x, c2, n2.cpu()),
                (x, c2[:0], n2[:0]), (x, torch.zeros(3, 1024, **bf), n2),
                (torch.zeros(6, 520, **bf), torch.zeros(3, 520, **bf), n2)]:
        with pytest.raises(RuntimeError):
            nat.kmeans_assign(*bad)


# ---------------------------------------------------------------------------
# end to end at d = 1536, a dimension the dispatch used to lack
# ---------------------------------------------------------------------------

def test_kmeans_blobs_cpu():
    x, labels = kc.blobs()
    torch.manual_seed(0)
    c, a = kmeans(x, 6, iters=20, seed=1)
    assert c.shape == (6, 1536) and kc.same_partition(a, labels)


@pytest.mark.gpu
def test_kmeans_blobs_1536_gpu():
    x, labels = kc.blobs()
    torch.manual_seed(0)
    c, a = kmeans(x.cuda(), 6, iters=20, seed=1)
    assert c.shape == (6, 1536) and c.is_cuda
    assert kc.same_partition(a.cpu(), labels)
    # each centroid is the mean of its blob, as rounded to bf16
    xb = x.to(torch.bfloat16).double()
    for j in range(6):
        rows = xb[a.cpu() == j]
        mean = rows.mean(0)
        bound = kc.EPS_ACC * rows.abs().mean(0) + 2.0 ** -21 * mean.abs()
        kc.check(f"gpu blobs centroid {j}", c[j], mean, bound)


@pytest.mark.gpu
def test_cluster_index_add_remove_1536_gpu():
    x, labels = kc.blobs()
    ids = [f"n{i}" for i in range(x.shape[0])]
    torch.manual_seed(0)
    ci = ClusterIndex()
    ci.cluster(ids, x.cuda(), k=6, seed=1)
    assert ci.counts.tolist() == [50] * 6
    assert sorted(len(m) for m in ci.members) == [50] * 6
    before = ci.centroids.clone()
    v = (x[120] + 0.01).to(torch.bfloat16).float().numpy()   # in blob 2
    home = ci._id2cluster["n120"]
    ci.add("new", v)
    assert ci._id2cluster["new"] == home
    assert "new" in ci.members[home] and len(ci.members[home]) == 51
    want = [50] * 6
    want[home] = 51
    assert ci.counts.tolist() == want
    assert float((ci.centroids[home] - before[home]).abs().sum()) > 0
    ci.remove("new", v)
    assert "new" not in ci.members[home] and "new" not in ci._id2cluster
    assert ci.counts.tolist() == [50] * 6
    assert sum(len(m) for m in ci.members) == int(ci.counts.sum()) == 300
    bound = kc.EPS_ACC * (before[home].abs() * 50 + torch.as_tensor(v).cuda()
                          .abs())
    assert ((ci.centroids[home] - before[home]).abs() <= bound).all()
    others = [j for j in range(6) if j != home]
    assert torch.equal(ci.centroids[others], before[others])
