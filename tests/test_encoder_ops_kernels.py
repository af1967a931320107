"""The element-wise encoder kernels of csrc/encoder_ops.hip (add_layernorm,
bias_gelu, mean_pool_l2norm) against float64 at the shapes, masks and
layouts where they can go wrong. Cases, references and bounds are in
tests/kernel_cases.py; each table also runs through the torch fp32 path of
ops/encoder.py on the CPU.
"""

import pytest
import torch

import kernel_cases as kc
from nornicdb_amd.ops.encoder import add_layernorm, bias_gelu, mean_pool_l2norm


def _nat():
    from nornicdb_amd.ops import require_native
    return require_native()


def _cuda(t):
    return None if t is None else t.cuda()


def _f32(t):
    return None if t is None else t.float()


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------------------
# add_layernorm
# ---------------------------------------------------------------------------

LN_ALL = kc.LN_SHAPES + [(2, 3, 64)] + [(5, d) for d in kc.LN_TORCH_DIMS]


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("shape", LN_ALL, ids=_ids)
def test_add_layernorm_bound_cpu(shape, with_b):
    a, b, g, be, ref, bound = kc.ln_case(shape, with_b)
    y = add_layernorm(a.float(), _f32(b), g, be, kc.LN_EPS)
    kc.check(f"cpu layernorm {shape} b {with_b}", y, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("shape", kc.LN_SHAPES + [(2, 3, 64)], ids=_ids)
def test_add_layernorm_gpu(shape, with_b):
    a, b, g, be, ref, bound = kc.ln_case(shape, with_b)
    y = _nat().add_layernorm(a.cuda(), _cuda(b), g.cuda(), be.cuda(),
                             kc.LN_EPS)
    assert y.dtype == torch.bfloat16
    kc.check(f"gpu layernorm {shape} b {with_b}", y, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("with_b", [True, False])
def test_add_layernorm_noncontiguous_gpu(with_b):
    """`a` (and `b`) are transposed views; the result is that of the
    contiguous copy."""
    a, b, g, be, ref, bound = kc.ln_case((5, 520), with_b)
    at = a.t().contiguous().cuda().t()
    bt = None if b is None else b.t().contiguous().cuda().t()
    assert not at.is_contiguous()
    y = _nat().add_layernorm(at, bt, g.cuda(), be.cuda(), kc.LN_EPS)
    assert y.shape == (5, 520)
    kc.check(f"gpu layernorm non-contiguous b {with_b}", y, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("d", kc.LN_TORCH_DIMS)
def test_add_layernorm_torch_path_gpu(d):
    """D = 8200 is past the kernel's limit and D = 12 no multiple of 8:
    ops.add_layernorm computes them with torch, inside the same bound."""
    a, b, g, be, ref, bound = kc.ln_case((5, d), True)
    y = add_layernorm(a.cuda(), b.cuda(), g.cuda(), be.cuda(), kc.LN_EPS)
    assert y.dtype == torch.bfloat16
    kc.check(f"gpu layernorm torch path D {d}", y, ref, bound)
    with pytest.raises(RuntimeError, match="D % 8"):
        _nat().add_layernorm(a.cuda(), b.cuda(), g.cuda(), be.cuda(),
                             kc.LN_EPS)


@pytest.mark.parametrize("case", kc.LN_OFFSET, ids=_ids)
def test_add_layernorm_offset_bound_cpu(case):
    """Rows far from zero, against the bound of the GPU test. At
    |mean| / std = 256 fp32 code that does not shift the row first cannot
    meet it where n * g + be cancels: the row mean alone is rounded to 2^-24
    of its size. There, and only there, the torch path is held to the bound
    plus four such roundings (NOTES.md, "Kernel test bounds")."""
    a, b, g, be, ref, bound, mean_term = kc.ln_offset_case(*case)
    y = add_layernorm(a.float(), b.float(), g, be, kc.LN_EPS)
    if case[2] == 256.0:
        bound = bound + 4 * mean_term
    kc.check(f"cpu layernorm offset {case}", y, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.LN_OFFSET, ids=_ids)
def test_add_layernorm_offset_gpu(case):
    """|mean| / std up to 256, inside the same bound as every other row: the
    kernel sums a row with |mean| > 2 std again, shifted by its first
    element."""
    a, b, g, be, ref, bound, _ = kc.ln_offset_case(*case)
    y = _nat().add_layernorm(a.cuda(), b.cuda(), g.cuda(), be.cuda(),
                             kc.LN_EPS)
    kc.check(f"gpu layernorm offset {case}", y, ref, bound)


# ---------------------------------------------------------------------------
# bias_gelu
# ---------------------------------------------------------------------------

def _exhaustive():
    """Every finite bf16 value as x, zero bias: x, ref, bound."""
    x = kc.all_finite_bf16()
    ref = kc.gelu64(x.double())
    return x, ref, kc.EPS_OUT * ref.abs() + kc.GELU_FLOOR


def test_bias_gelu_exhaustive_bound_cpu():
    x, ref, bound = _exhaustive()
    kc.check("cpu gelu every bf16", bias_gelu(x.float(), torch.zeros(8)),
             ref, bound)


@pytest.mark.gpu
def test_bias_gelu_exhaustive_gpu():
    x, ref, bound = _exhaustive()
    y = _nat().bias_gelu(x.cuda(), torch.zeros(8, device="cuda"))
    kc.check("gpu gelu every bf16", y, ref, bound)


@pytest.mark.parametrize("shape", kc.GELU_SHAPES, ids=_ids)
def test_bias_gelu_bound_cpu(shape):
    x, bias, ref, bound = kc.gelu_case(shape)
    kc.check(f"cpu gelu {shape}", bias_gelu(x.float(), bias), ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", kc.GELU_SHAPES, ids=_ids)
def test_bias_gelu_gpu(shape):
    x, bias, ref, bound = kc.gelu_case(shape)
    y = _nat().bias_gelu(x.cuda(), bias.cuda())
    assert y.dtype == torch.bfloat16
    kc.check(f"gpu gelu {shape}", y, ref, bound)


@pytest.mark.gpu
def test_bias_gelu_3d_noncontiguous_gpu():
    x, bias, ref, bound = kc.gelu_case((6, 4, 48))
    xt = x.transpose(0, 1).contiguous().cuda().transpose(0, 1)
    assert not xt.is_contiguous() and xt.shape == (6, 4, 48)
    y = _nat().bias_gelu(xt, bias.cuda())
    assert y.shape == (6, 4, 48)
    kc.check("gpu gelu 3d non-contiguous", y, ref, bound)


def test_bias_gelu_3d_bound_cpu():
    x, bias, ref, bound = kc.gelu_case((6, 4, 48))
    kc.check("cpu gelu 3d", bias_gelu(x.float(), bias), ref, bound)


# ---------------------------------------------------------------------------
# mean_pool_l2norm
# ---------------------------------------------------------------------------

def _check_pool(name, y, case):
    x, mask, ref, bound, live = case
    assert y.dtype == torch.float32
    kc.check(name, y, ref, bound)
    norm = y.detach().cpu().double().norm(dim=-1)
    assert ((norm[live] - 1).abs() <= kc.EPS_ACC).all(), f"{name}: norm"
    assert (y.detach().cpu()[~live] == 0).all(), f"{name}: masked row"


@pytest.mark.parametrize("kind", kc.POOL_MASKS)
@pytest.mark.parametrize("shape", kc.POOL_SHAPES, ids=_ids)
def test_mean_pool_bound_cpu(shape, kind):
    case = kc.pool_case(shape, kind)
    _check_pool(f"cpu pool {shape} {kind}",
                mean_pool_l2norm(case[0].float(), case[1]), case)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", kc.POOL_MASKS)
@pytest.mark.parametrize("shape", kc.POOL_SHAPES, ids=_ids)
def test_mean_pool_gpu(shape, kind):
    case = kc.pool_case(shape, kind)
    y = _nat().mean_pool_l2norm(case[0].cuda(), _cuda(case[1]))
    _check_pool(f"gpu pool {shape} {kind}", y, case)


# ---------------------------------------------------------------------------
# empty inputs: an empty result of the right shape, nothing launched
# ---------------------------------------------------------------------------

def _empty_checks(dev, dtype):
    g, be = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    for shape in [(0, 64), (2, 0, 64)]:
        a = torch.zeros(shape, device=dev, dtype=dtype)
        for b in (a, None):
            y = add_layernorm(a, b, g, be)
            assert y.shape == shape and y.dtype == dtype
        y = bias_gelu(a, be)
        assert y.shape == shape and y.dtype == dtype
    y = mean_pool_l2norm(torch.zeros(0, 5, 64, device=dev, dtype=dtype))
    assert y.shape == (0, 64) and y.dtype == torch.float32
    y = mean_pool_l2norm(torch.zeros(0, 5, 64, device=dev, dtype=dtype),
                         torch.ones(0, 5, device=dev, dtype=torch.int64))
    assert y.shape == (0, 64)


def test_empty_inputs_cpu():
    _empty_checks("cpu", torch.float32)


@pytest.mark.gpu
def test_empty_inputs_gpu():
    _empty_checks("cuda", torch.bfloat16)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_encoder_ops_argument_checks_gpu():
    """gamma, beta and bias of the wrong length would be read out of
    bounds; the wrappers refuse them."""
    nat = _nat()
    a = torch.zeros(4, 64, device="cuda", dtype=torch.bfloat16)
    g64, g32 = torch.ones(64, device="cuda"), torch.ones(32, device="cuda")
    with pytest.raises(RuntimeError, match="gamma"):
        nat.add_layernorm(a, None, g32, g64, 1e-5)
    with pytest.raises(RuntimeError, match="gamma"):
        nat.add_layernorm(a, None, g64, g32, 1e-5)
    with pytest.raises(RuntimeError, match="b must"):
        nat.add_layernorm(a, a[:2], g64, g64, 1e-5)
    with pytest.raises(RuntimeError, match="b must"):
        nat.add_layernorm(a, a.float(), g64, g64, 1e-5)
    with pytest.raises(RuntimeError, match="bias"):
        nat.bias_gelu(a, g32)
    x = torch.zeros(2, 3, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="mask"):
        nat.mean_pool_l2norm(x, torch.ones(2, 4, device="cuda"))
