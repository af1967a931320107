"""Case tables, inputs and float64 references shared by
tests/test_gemm_kernels.py, tests/test_kmeans_kernels.py and
tests/test_encoder_ops_kernels.py. A plain module, no fixtures; every input
is seeded, built on the CPU and cached once per process together with its
reference, so the CPU check of a bound and the GPU test of the kernel see
the same tensors.

How every comparison is made: the reference is float64 arithmetic on exactly
the values the kernel reads (inputs already rounded to bf16; gamma, beta and
bias too, because the wrappers convert them). The bound is per element:
EPS_OUT * |ref| for the one bf16 rounding of the output (round-to-nearest is
off by at most half an ulp, which just above a power of two is 2^-8 of the
value), plus EPS_ACC times the sum of the absolute values of the terms that
were accumulated in fp32. NOTES.md, "Kernel test bounds", has the
derivations and the measured error/bound ratios.
"""

import math

import torch

EPS_OUT = 2.0 ** -8
EPS_ACC = 2.0 ** -18
GELU_LIP = 1.13          # sup |gelu'|: an error made before GELU grows by this

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def randn_bf16(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def gelu64(x):
    """erf GELU in float64; erfc keeps the digits of the negative tail."""
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def check(name, y, ref, bound):
    """Assert |y - ref| <= bound for every element and return the largest
    error/bound ratio, which is also printed for NOTES.md."""
    y = y.detach().cpu().double()
    assert y.shape == ref.shape, (name, tuple(y.shape), tuple(ref.shape))
    assert torch.isfinite(y).all(), f"{name}: non-finite output"
    if y.numel() == 0:
        return 0.0
    err = (y - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), ratio)
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst),
                                                    ratio.shape))
    top = float(ratio.flatten()[worst])
    print(f"RATIO {name} {top:.3f}")
    assert top <= 1.0, (
        f"{name}: {int((err > bound).sum())} of {err.numel()} elements out "
        f"of bound, worst at {idx}: got {float(y[idx])!r}, ref "
        f"{float(ref[idx])!r}, err {float(err[idx]):.3e}, bound "
        f"{float(bound[idx]):.3e}")
    return top


def first_mismatch(y, want):
    """None if bit-identical, else a message naming the first wrong (i, j)."""
    y = y.detach().cpu()
    if torch.equal(y, want):
        return None
    bad = (y != want).nonzero()
    i, j = (int(v) for v in bad[0])
    return (f"{bad.shape[0]} of {want.numel()} wrong, first at ({i}, {j}): "
            f"got {float(y[i, j])!r}, want {float(want[i, j])!r}")


# ---------------------------------------------------------------------------
# GEMM: C = act(A W^T + bias)
# ---------------------------------------------------------------------------

# (M, N, K, act, has_bias). Variant A (256x256 tile) by a direct native
# call: M % 256 == 0 and M % 96 != 0. tiles = (M / 256) * (N / 256).
GEMM_A_DIRECT = [
    (256, 256, 128, 0, False),    # 1 tile; K = 128: prologue, no steady state
    (256, 768, 256, 1, True),     # 3 tiles
    (512, 768, 1024, 0, True),    # 6 tiles, long K loop
    (1280, 256, 256, 1, False),   # 5 tiles, remainder band only
    (2048, 256, 128, 0, True),    # 8 tiles: nwg & 7 == 0, one full band
    (1280, 768, 128, 1, True),    # 15 tiles
    (512, 256, 1024, 0, False),   # 2 tiles
]
# Variant A through ops.gemm.gemm_nt with NORNICDB_GEMM_KERNEL=256.
GEMM_A_ENV = [
    (1000, 256, 256, 1, True),    # pads to 1024: 4 tiles
    (768, 768, 128, 0, False),    # 9 tiles; variant B without the variable
    (768, 256, 1024, 1, False),   # 3 tiles
]
# Variant B (96x256 tile) by a direct native call; row tiles = M / 96.
GEMM_B = [
    (96, 256, 64, 0, False),      # 1 row tile, K = 64: one loop trip
    (960, 256, 128, 1, True),     # 10: remainder band only
    (1536, 512, 128, 0, True),    # 16: exactly one band
    (1632, 256, 128, 1, False),   # 17: a band plus one
    (3168, 256, 64, 0, True),     # 33
    (3168, 512, 128, 1, True),    # 33, two column tiles
    (96, 768, 512, 0, True),      # K = 512
    (192, 256, 512, 1, False),
]
# (M, N, K) of the exact one-hot layout tests.
ONEHOT_A = [(256, 256, 128), (512, 768, 256), (2048, 256, 128),
            (256, 768, 1024), (1280, 768, 128)]
ONEHOT_A_ENV = [(1000, 256, 256), (768, 768, 128)]
ONEHOT_B = [(96, 256, 64), (960, 256, 128), (1632, 512, 128),
            (3168, 256, 64), (3168, 512, 128), (96, 768, 512)]


def gemm_inputs(m, n, k):
    """bf16 A [m, k], W [n, k], bias [n]; products of size about 1."""
    def make():
        s = k ** -0.25
        return (randn_bf16((m, k), 7 * m + n + k, s),
                randn_bf16((n, k), 11 * n + m + k + 1, s),
                randn_bf16((n,), 13 * n + k + 2))
    return cached(("gemm in", m, n, k), make)


def gemm_ref(a, w, bias, act, mid_round=False):
    """(ref, bound) of act(a w^T + bias) in float64. mid_round: the product
    was rounded to bf16 before bias and GELU (the library path)."""
    ad, wd = a.double(), w.double()
    prod = ad @ wd.T
    mag = ad.abs() @ wd.abs().T
    pre, acc = prod, EPS_ACC * mag
    if bias is not None:
        pre = pre + bias.double()
        acc = acc + EPS_ACC * bias.double().abs()
    if mid_round:
        acc = acc + EPS_OUT * prod.abs()
    if act:
        return gelu64(pre), EPS_OUT * gelu64(pre).abs() + GELU_LIP * acc
    return pre, EPS_OUT * pre.abs() + acc


def gemm_case(m, n, k, act, has_bias):
    """(a, w, bias or None, ref, bound), cached."""
    def make():
        a, w, b = gemm_inputs(m, n, k)
        b = b if has_bias else None
        return (a, w, b) + gemm_ref(a, w, b, act)
    return cached(("gemm", m, n, k, act, has_bias), make)


def onehot_case(m, n, k, which):
    """which = "a": A one-hot, A[i, i % k] = 1, W random; the product is
    C[i, j] = W[j, i % k] exactly. which = "w": W[j, j % k] = 1, A random,
    C[i, j] = A[i, j % k]. Returns (a, w, want)."""
    def make():
        a, w, _ = gemm_inputs(m, n, k)
        if which == "a":
            a = torch.zeros(m, k, dtype=torch.bfloat16)
            a[torch.arange(m), torch.arange(m) % k] = 1
            want = w[:, torch.arange(m) % k].T.contiguous()
        else:
            w = torch.zeros(n, k, dtype=torch.bfloat16)
            w[torch.arange(n), torch.arange(n) % k] = 1
            want = a[:, torch.arange(n) % k].contiguous()
        return a, w, want
    return cached(("onehot", m, n, k, which), make)


# ---------------------------------------------------------------------------
# k-means
# ---------------------------------------------------------------------------

# every case of both dispatch switches (d / 512 = 1 .. 8)
KM_DIMS = [512, 1024, 1536, 2048, 2560, 3072, 3584, 4096]
KM_NS = [1, 3, 5, 1000]
KM_KS = [1, 2, 33]
KM_STRIDE_N = 32771        # at d = 512: past 8192 blocks x 4 waves
DUP_LO, DUP_HI = 5, 20     # k = 33: centroid rows 5 and 20 are identical


def assign_case(n, d, k):
    """x [n, d], cent [k, d] bf16, cnorm2 [k] fp32 (what is passed to the
    kernel), ref_d2 [n, k] float64 from those, tol [n] float64.

    x[0] equals the last centroid. With k = 2 the two centroids are the same
    row, so every point ties and index 0 must win; with k = 33 rows DUP_LO
    and DUP_HI are the same and x[1] (if any) equals them."""
    def make():
        x = randn_bf16((n, d), 3 * n + d + k)
        cent = randn_bf16((k, d), 5 * k + d + n + 1)
        if k == 2:
            cent[1] = cent[0]
        if k > DUP_HI:
            cent[DUP_HI] = cent[DUP_LO]
            if n > 1:
                x[1] = cent[DUP_LO]
        x[0] = cent[k - 1]
        cnorm2 = (cent.float() ** 2).sum(-1)
        xd, cd = x.double(), cent.double()
        xsq = (xd * xd).sum(-1)
        ref_d2 = cnorm2.double()[None] - 2.0 * xd @ cd.T + xsq[:, None]
        tol = EPS_ACC * (xsq + (cd * cd).sum(-1).max())
        return x, cent, cnorm2, ref_d2, tol
    return cached(("assign", n, d, k), make)


def check_assign(name, a, d2, case, lower_wins):
    """The chosen centroid is within tol of the best one and the reported
    distance within tol of the chosen one's, for every point."""
    x, cent, cnorm2, ref_d2, tol = case
    n, k = ref_d2.shape
    a = a.detach().cpu().long()
    d2 = d2.detach().cpu().double()
    assert a.shape == (n,) and d2.shape == (n,)
    assert ((a >= 0) & (a < k)).all(), f"{name}: index out of range"
    assert (d2 >= 0).all(), f"{name}: negative distance"
    chosen = ref_d2.gather(1, a[:, None])[:, 0]
    gap = (chosen - ref_d2.min(1).values) / tol
    err = (d2 - chosen).abs() / tol
    print(f"RATIO {name} choice {float(gap.max()):.3f} "
          f"distance {float(err.max()):.3f}")
    assert gap.max() <= 1.0, f"{name}: point {int(gap.argmax())} not nearest"
    assert err.max() <= 1.0, f"{name}: point {int(err.argmax())} distance off"
    # the point that equals a centroid
    assert d2[0] <= tol[0], f"{name}: d2 of a point on its centroid"
    if lower_wins:
        if k == 2:
            assert (a == 0).all(), f"{name}: tie not won by the lower index"
        if k > DUP_HI:
            assert (a != DUP_HI).all(), f"{name}: duplicate row won"
            if n > 1:
                assert a[1] == DUP_LO
    return float(max(gap.max(), err.max()))


# (n, d, k, assignment): all in one cluster past the 4096-block grid; empty
# clusters at a d that is no multiple of the block; k = 1.
ACCUM_CASES = [
    (4100, 512, 3, "one"),
    (1000, 520, 7, "sparse"),
    (37, 8, 1, "one"),
]


def accum_case(n, d, k, kind):
    """x bf16 [n, d], assign int32 [n], ref_sums [k, d], bound, ref_counts."""
    def make():
        x = randn_bf16((n, d), n + d + k)
        if kind == "one":
            assign = torch.full((n,), k // 2, dtype=torch.int32)
        else:
            g = torch.Generator().manual_seed(n)
            assign = torch.tensor([0, 2, 5], dtype=torch.int32)[
                torch.randint(0, 3, (n,), generator=g)]
        xd = x.double()
        sums = torch.zeros(k, d, dtype=torch.float64)
        mag = torch.zeros(k, d, dtype=torch.float64)
        sums.index_add_(0, assign.long(), xd)
        mag.index_add_(0, assign.long(), xd.abs())
        counts = torch.bincount(assign.long(), minlength=k).int()
        return x, assign, sums, EPS_ACC * mag, counts
    return cached(("accum", n, d, k, kind), make)


FINALIZE_DIMS = [8, 520]


def finalize_case(d):
    """k = 5 (not a multiple of the 4 waves of a block), clusters 1 and 4
    empty. sums, old fp32; counts int32; float64 ref_new, ref_drift2 and
    their bounds: the quotient is within 2.5 ulp (2^-21 of the value), the
    drift a sum of d squares of (|new| + |old|)-sized terms."""
    def make():
        g = torch.Generator().manual_seed(d)
        sums = torch.randn(5, d, generator=g) * 9
        old = torch.randn(5, d, generator=g)
        counts = torch.tensor([3, 0, 1, 11, 0], dtype=torch.int32)
        cd = counts.double()[:, None]
        new = torch.where(cd > 0, sums.double() / cd.clamp_min(1),
                          old.double())
        drift = ((new - old.double()) ** 2).sum(-1)
        b_new = 2.0 ** -21 * new.abs()
        b_drift = EPS_ACC * ((new.abs() + old.double().abs()) ** 2).sum(-1)
        return sums, counts, old, new, b_new, drift, b_drift
    return cached(("finalize", d), make)


PP_N = 257                 # not a multiple of the 4 waves of a block
PP_SEEDS = (3, 101)        # odd rows
PP_SMALL = 2.0 ** -40      # even rows start here: already smaller


def pp_case(d):
    """x bf16 [PP_N, d]; the two seeds are rows of x. d2 starts at 3.4e38 in
    the odd rows and at PP_SMALL in the even ones. Returns x, d2_start,
    float64 ref [n] (min of the two distances) and tol [n]."""
    def make():
        x = randn_bf16((PP_N, d), d + 17)
        xd = x.double()
        start = torch.full((PP_N,), 3.4e38)
        start[0::2] = PP_SMALL
        dist = torch.stack([((xd - xd[s]) ** 2).sum(-1) for s in PP_SEEDS])
        xsq = (xd * xd).sum(-1)
        tol = EPS_ACC * (xsq + max(float(xsq[s]) for s in PP_SEEDS))
        return x, start, dist.min(0).values, tol
    return cached(("pp", d), make)


POINT_DIMS = [512, 4096]
POINT_COUNTS = [0, 1, 7, 0]


def point_case(d):
    """cent fp32 [4, d], counts int32 [4], point bf16 [d]."""
    def make():
        g = torch.Generator().manual_seed(d + 1)
        cent = torch.randn(4, d, generator=g)
        return (cent, torch.tensor(POINT_COUNTS, dtype=torch.int32),
                randn_bf16((d,), d + 2))
    return cached(("point", d), make)


def blobs(d=1536, per=50, seed=9):
    """Six well-separated blobs: x fp32 [6 * per, d] and the labels."""
    def make():
        g = torch.Generator().manual_seed(seed)
        centers = torch.randn(6, d, generator=g) * 5
        x = centers.repeat_interleave(per, 0) + \
            0.1 * torch.randn(6 * per, d, generator=g)
        return x, torch.arange(6).repeat_interleave(per)
    return cached(("blobs", d, per, seed), make)


def same_partition(assign, labels):
    """True when assign equals labels up to a permutation of the names."""
    pairs = {(int(a), int(b)) for a, b in zip(assign.tolist(),
                                              labels.tolist())}
    return (len(pairs) == len({a for a, _ in pairs})
            == len({b for _, b in pairs}) == int(labels.max()) + 1)


# ---------------------------------------------------------------------------
# encoder element-wise ops
# ---------------------------------------------------------------------------

LN_EPS = 1e-5
# (rows, D); the last is the grid-stride second trip (4096 blocks x 4 waves)
LN_SHAPES = [(1, 8), (5, 520), (333, 1024), (3, 8192), (16390, 64)]
LN_TORCH_DIMS = [8200, 12]          # ops.add_layernorm takes the torch path
# (rows, D, |mean| / std). The kernel sums a row a second time, shifted,
# when |mean| > 2 std: 1.5 and 3 are the two sides of that switch.
LN_OFFSET = [(64, 1024, 32.0), (64, 1024, 256.0), (5, 520, 32.0),
             (5, 520, 256.0), (64, 1024, 1.5), (64, 1024, 3.0)]


def _ln_ref(xd, g, be):
    mean = xd.mean(-1, keepdim=True)
    var = xd.var(-1, unbiased=False, keepdim=True)
    n = (xd - mean) / torch.sqrt(var + LN_EPS)
    ng = n * g.double()
    ref = ng + be.double()
    # against the terms, not the result: n * g + be may cancel
    bound = EPS_OUT * ref.abs() + EPS_ACC * (ng.abs() + be.double().abs())
    return ref, bound, mean, var


def ln_case(shape, with_b):
    """a, b (or None) bf16 of `shape`; gamma, beta fp32 holding bf16 values;
    float64 ref and bound."""
    def make():
        d = shape[-1]
        seed = sum(shape) + 100 * with_b
        a = randn_bf16(shape, seed)
        b = randn_bf16(shape, seed + 1) if with_b else None
        g = randn_bf16((d,), seed + 2).float()
        be = randn_bf16((d,), seed + 3).float()
        xd = a.double() if b is None else a.double() + b.double()
        return (a, b, g, be) + _ln_ref(xd, g, be)[:2]
    return cached(("ln", tuple(shape), with_b), make)


def ln_offset_case(rows, d, ratio):
    """Rows of std 1 around +-ratio: the offset, exact in bf16, is `a`, the
    noise is `b`. Noise below 2^-8 is zeroed, so that a + b is exact in fp32
    and the float64 reference starts from what the kernel has. Returns
    a, b, g, be, ref, bound and mean_term, the rounding of a row mean that
    fp32 code without a shift cannot avoid, in units of the output."""
    def make():
        seed = rows + d + int(2 * ratio)
        sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)
        a = (sign * ratio)[:, None].expand(rows, d).to(torch.bfloat16)
        a = a.contiguous()
        assert torch.equal(a.float().abs(), torch.full((rows, d), ratio))
        b = randn_bf16((rows, d), seed)
        b = torch.where(b.float().abs() < 2.0 ** -8, torch.zeros_like(b), b)
        g = randn_bf16((d,), seed + 2).float()
        be = randn_bf16((d,), seed + 3).float()
        xd = a.double() + b.double()
        assert torch.equal((a.float() + b.float()).double(), xd)
        ref, bound, mean, var = _ln_ref(xd, g, be)
        mean_term = 2.0 ** -24 * mean.abs() / var.sqrt() * g.double().abs()
        return a, b, g, be, ref, bound, mean_term
    return cached(("ln offset", rows, d, ratio), make)


def all_finite_bf16():
    """Every finite bf16 value once, as [8192, 8]; the 256 slots of the
    infinities and NaNs hold zero."""
    def make():
        bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
        x = bits.view(torch.bfloat16).clone()
        x[~torch.isfinite(x.float())] = 0
        assert int((x.float() != 0).sum()) == 65536 - 256 - 2
        return x.reshape(8192, 8)
    return cached("all bf16", make)


GELU_FLOOR = 1e-6   # 1 + erf cancels in fp32 for x below about -5
# the last has 8 390 160 elements: a second grid-stride trip whose step
# (4096 * 256 * 8) is no multiple of D
GELU_SHAPES = [(1, 8), (1000, 4096), (8130, 1032)]


def gelu_ref(x, bias):
    """(ref, bound) of gelu(x + bias): the fp32 sum of two bf16 numbers is
    one more EPS_ACC-sized term before GELU."""
    pre = x.double() + bias.double()
    ref = gelu64(pre)
    acc = EPS_ACC * (x.double().abs() + bias.double().abs())
    return ref, EPS_OUT * ref.abs() + GELU_LIP * acc + GELU_FLOOR


def gelu_case(shape):
    def make():
        x = randn_bf16(shape, sum(shape), 2.0)
        bias = randn_bf16((shape[-1],), sum(shape) + 1).float()
        return (x, bias) + gelu_ref(x, bias)
    return cached(("gelu", tuple(shape)), make)


POOL_SHAPES = [(1, 1, 8), (3, 7, 2056), (8, 128, 1024)]
POOL_MASKS = ["none", "ones", "ragged", "bool", "int64", "masked_row"]


def pool_case(shape, kind):
    """x bf16 [B, S, D]; mask (or None) as passed; float64 ref [B, D], the
    bound, and which rows are not empty."""
    def make():
        bsz, s, d = shape
        x = randn_bf16(shape, sum(shape))
        g = torch.Generator().manual_seed(s)
        ragged = (torch.rand(bsz, s, generator=g) < 0.6).to(torch.int32)
        ragged[:, s // 2] = 1       # holes, and no row empty
        mask = {"none": None,
                "ones": torch.ones(bsz, s, dtype=torch.int32),
                "ragged": ragged,
                "bool": ragged.bool(),
                "int64": ragged.long(),
                "masked_row": ragged.clone()}[kind]
        if kind == "masked_row":
            mask[0] = 0
        m = torch.ones(bsz, s, dtype=torch.float64) if mask is None \
            else mask.double()
        xd = x.double()
        count = m.sum(1)
        pooled = (xd * m[..., None]).sum(1) / count.clamp_min(1)[:, None]
        norm = pooled.norm(dim=-1, keepdim=True)
        live = count > 0
        ref = torch.where(live[:, None], pooled / norm.clamp_min(1e-300),
                          torch.zeros_like(pooled))
        mag = (xd.abs() * m[..., None]).sum(1)
        bound = EPS_ACC * mag / (count.clamp_min(1)[:, None]
                                 * norm.clamp_min(1e-300)) + 2.0 ** -20
        bound = torch.where(live[:, None], bound, torch.zeros_like(bound))
        return x, mask, ref, bound, live
    return cached(("pool", tuple(shape), kind), make)
