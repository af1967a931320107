"""Both hand-written GEMM kernels of csrc/gemm.hip against float64: variant A
(256x256 tile, k_gemm_nt) and variant B (96x256 tile, k_gemm_nt96). Every
GPU test asserts through _C.gemm_nt_variant which of the two it ran. The
cases, references and bounds are in tests/kernel_cases.py; each table is also
pushed through the torch fp32 path on the CPU, which checks the bound and
the inputs where there is no GPU.
"""

import pytest
import torch
import torch.nn.functional as F

import kernel_cases as kc
from nornicdb_amd.ops import gemm as G

ENV = "NORNICDB_GEMM_KERNEL"


def _nat():
    from nornicdb_amd.ops import require_native
    return require_native()


def _cuda(t):
    return None if t is None else t.cuda()


def _name(tag, case):
    return tag + " " + "x".join(str(v) for v in case)


# ---------------------------------------------------------------------------
# CPU: the torch fp32 path stays inside every bound
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", kc.GEMM_A_DIRECT + kc.GEMM_A_ENV + kc.GEMM_B,
                         ids=lambda c: "x".join(map(str, c)))
def test_gemm_bound_cpu(case):
    a, w, b, ref, bound = kc.gemm_case(*case)
    y = G.linear_act(a.float(), w.float(),
                     None if b is None else b.float(), case[3])
    kc.check(_name("cpu gemm", case), y, ref, bound)


@pytest.mark.parametrize("which", ["a", "w"])
@pytest.mark.parametrize("shape", kc.ONEHOT_A + kc.ONEHOT_A_ENV + kc.ONEHOT_B,
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_onehot_cpu(shape, which):
    a, w, want = kc.onehot_case(*shape, which)
    y = G.linear_act(a.float(), w.float()).to(torch.bfloat16)
    assert kc.first_mismatch(y, want) is None


def test_gemm_bias_only_cpu():
    a, w, b = kc.gemm_inputs(256, 256, 128)
    a0 = torch.zeros_like(a)
    for act in (0, 1):
        ref, bound = kc.gemm_ref(a0, w, b, act)
        y = G.linear_act(a0.float(), w.float(), b.float(), act)
        kc.check(f"cpu bias only act {act}", y, ref, bound)


def test_gemm_variant_query(monkeypatch):
    """gemm_nt_variant answers as the launch chooses, with and without the
    environment variable; needs the extension, not a GPU."""
    nat = _nat()
    monkeypatch.delenv(ENV, raising=False)
    assert [nat.gemm_nt_variant(m) for m in (0, 96, 256, 768, 1000, 1280)] \
        == [96, 96, 256, 96, 256, 256]
    monkeypatch.setenv(ENV, "256")
    assert [nat.gemm_nt_variant(m) for m in (0, 96, 768, 1024)] == [256] * 4
    monkeypatch.setenv(ENV, "96")
    assert nat.gemm_nt_variant(768) == 96 and nat.gemm_nt_variant(256) == 256


# ---------------------------------------------------------------------------
# GPU: random-data numerics, all four (ACT, HAS_BIAS) kernels of each variant
# ---------------------------------------------------------------------------

def _run_direct(case, variant):
    nat = _nat()
    a, w, b, ref, bound = kc.gemm_case(*case)
    assert nat.gemm_nt_variant(case[0]) == variant
    y = nat.gemm_nt(a.cuda(), w.cuda(), _cuda(b), case[3])
    kc.check(_name(f"gpu gemm {variant}", case), y, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.GEMM_A_DIRECT,
                         ids=lambda c: "x".join(map(str, c)))
def test_gemm_variant_a_direct_gpu(case, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    _run_direct(case, 256)


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.GEMM_A_ENV,
                         ids=lambda c: "x".join(map(str, c)))
def test_gemm_variant_a_env_gpu(case, monkeypatch):
    """Through ops.gemm.gemm_nt with the variable set: M = 1000 pads to 1024,
    M = 768 would be variant B without it."""
    nat = _nat()
    monkeypatch.setenv(ENV, "256")
    a, w, b, ref, bound = kc.gemm_case(*case)
    padded = (case[0] + 255) // 256 * 256
    assert nat.gemm_nt_variant(padded) == 256
    assert nat.gemm_nt_variant(case[0]) == 256
    y = G.gemm_nt(a.cuda(), w.cuda(), _cuda(b), case[3])
    kc.check(_name("gpu gemm 256 env", case), y, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.GEMM_B,
                         ids=lambda c: "x".join(map(str, c)))
def test_gemm_variant_b_gpu(case, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    _run_direct(case, 96)


@pytest.mark.gpu
def test_gemm_ops_pads_to_variant_b_gpu(monkeypatch):
    """Without the variable ops.gemm.gemm_nt pads M = 1000 to 1056 rows and
    runs variant B."""
    nat = _nat()
    monkeypatch.delenv(ENV, raising=False)
    case = (1000, 256, 256, 1, True)
    a, w, b, ref, bound = kc.gemm_case(*case)
    assert nat.gemm_nt_variant(1056) == 96
    y = G.gemm_nt(a.cuda(), w.cuda(), b.cuda(), 1)
    assert y.shape == (1000, 256)
    kc.check(_name("gpu gemm 96 ops", case), y, ref, bound)


# ---------------------------------------------------------------------------
# GPU: exact layout. One-hot operands make the product a gather, so equality
# pins the swizzle, the K-tile order, the XCD and band remaps and that every
# tile is written.
# ---------------------------------------------------------------------------

def _run_onehot(shape, which, variant, through_ops):
    nat = _nat()
    a, w, want = kc.onehot_case(*shape, which)
    if through_ops:
        assert nat.gemm_nt_variant((shape[0] + 255) // 256 * 256) == variant
        y = G.gemm_nt(a.cuda(), w.cuda(), None, 0)
    else:
        assert nat.gemm_nt_variant(shape[0]) == variant
        y = nat.gemm_nt(a.cuda(), w.cuda(), None, 0)
    bad = kc.first_mismatch(y, want)
    assert bad is None, f"variant {variant} {shape} one-hot {which}: {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["a", "w"])
@pytest.mark.parametrize("shape", kc.ONEHOT_A,
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_onehot_variant_a_gpu(shape, which, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    _run_onehot(shape, which, 256, False)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["a", "w"])
@pytest.mark.parametrize("shape", kc.ONEHOT_A_ENV,
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_onehot_variant_a_env_gpu(shape, which, monkeypatch):
    monkeypatch.setenv(ENV, "256")
    _run_onehot(shape, which, 256, True)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["a", "w"])
@pytest.mark.parametrize("shape", kc.ONEHOT_B,
                         ids=lambda s: "x".join(map(str, s)))
def test_gemm_onehot_variant_b_gpu(shape, which, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    _run_onehot(shape, which, 96, False)


# ---------------------------------------------------------------------------
# GPU: bias only (A = 0)
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("m,variant", [(256, 256), (96, 96)])
def test_gemm_bias_only_gpu(m, variant, monkeypatch):
    nat = _nat()
    monkeypatch.delenv(ENV, raising=False)
    _, w, b = kc.gemm_inputs(256, 256, 128)
    a0 = torch.zeros(m, 128, dtype=torch.bfloat16)
    assert nat.gemm_nt_variant(m) == variant
    y0 = nat.gemm_nt(a0.cuda(), w.cuda(), b.cuda(), 0)
    assert torch.equal(y0.cpu(), b[None].expand(m, 256)), \
        "act 0: the bias must come through bit for bit"
    ref, bound = kc.gemm_ref(a0, w, b, 1)
    y1 = nat.gemm_nt(a0.cuda(), w.cuda(), b.cuda(), 1)
    kc.check(f"gpu bias only gelu {variant}", y1, ref, bound)


# ---------------------------------------------------------------------------
# GPU: the host checks raise before anything is launched
# ---------------------------------------------------------------------------

@pytest.mark.gpu
def test_gemm_host_checks_raise_gpu(monkeypatch):
    nat = _nat()
    monkeypatch.delenv(ENV, raising=False)

    def bf(*shape):
        return torch.zeros(*shape, device="cuda", dtype=torch.bfloat16)

    with pytest.raises(RuntimeError, match="N % 256"):
        nat.gemm_nt(bf(96, 128), bf(128, 128), None, 0)
    with pytest.raises(RuntimeError, match="bias"):
        nat.gemm_nt(bf(96, 128), bf(256, 128),
                    torch.zeros(256, device="cuda"), 0)
    with pytest.raises(RuntimeError, match="contiguous"):
        nat.gemm_nt(bf(128, 96).t(), bf(256, 128), None, 0)
    with pytest.raises(RuntimeError, match="act"):
        nat.gemm_nt(bf(96, 128), bf(256, 128), None, 2)
    with pytest.raises(RuntimeError, match="M tiling"):
        nat.gemm_nt(bf(100, 128), bf(256, 128), None, 0)
    with pytest.raises(RuntimeError, match="K mismatch"):
        nat.gemm_nt(bf(96, 128), bf(256, 256), None, 0)
    with pytest.raises(RuntimeError, match="empty"):
        nat.gemm_nt(bf(96, 0), bf(256, 0), None, 0)
    # K = 64 is one trip of variant B but less than variant A's prologue
    with pytest.raises(RuntimeError, match="K tiling"):
        nat.gemm_nt(bf(256, 64), bf(256, 64), None, 0)
    monkeypatch.setenv(ENV, "256")
    with pytest.raises(RuntimeError, match="K tiling"):
        nat.gemm_nt(bf(768, 64), bf(256, 64), None, 0)
    with pytest.raises(RuntimeError, match="M tiling"):
        nat.gemm_nt(bf(96, 128), bf(256, 128), None, 0)


# ---------------------------------------------------------------------------
# GPU: linear_act dispatch
# ---------------------------------------------------------------------------

def _linear_inputs(n):
    x = kc.randn_bf16((2, 48, 128), 21, 128 ** -0.25)
    w = kc.randn_bf16((n, 128), 22 + n, 128 ** -0.25)
    b = kc.randn_bf16((n,), 23 + n)
    return x, w, b


@pytest.mark.gpu
@pytest.mark.parametrize("has_bias", [True, False])
def test_linear_act_hand_falls_back_gpu(has_bias, monkeypatch):
    """_FORCE_HAND with N = 200, which does not tile: the library product,
    rounded to bf16, then bias and GELU. A 3-D input keeps its shape."""
    monkeypatch.setattr(G, "_FORCE_LIB", False)
    monkeypatch.setattr(G, "_FORCE_HAND", True)
    x, w, b = _linear_inputs(200)
    b = b if has_bias else None
    ref, bound = kc.gemm_ref(x.reshape(96, 128), w, b, 1, mid_round=True)
    y = G.linear_act(x.cuda(), w.cuda(), _cuda(b), G.ACT_GELU)
    assert y.shape == (2, 48, 200) and y.dtype == torch.bfloat16
    kc.check(f"gpu linear_act fallback bias {has_bias}", y.reshape(96, 200),
             ref, bound)


@pytest.mark.gpu
def test_linear_act_hand_3d_gpu(monkeypatch):
    """_FORCE_HAND with a shape that tiles: 2 x 48 rows are one variant-B
    tile, no rounding between product and GELU."""
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.setattr(G, "_FORCE_LIB", False)
    monkeypatch.setattr(G, "_FORCE_HAND", True)
    x, w, b = _linear_inputs(256)
    assert _nat().gemm_nt_variant(96) == 96
    ref, bound = kc.gemm_ref(x.reshape(96, 128), w, b, 1)
    y = G.linear_act(x.cuda(), w.cuda(), b.cuda(), G.ACT_GELU)
    assert y.shape == (2, 48, 256)
    kc.check("gpu linear_act hand 3d", y.reshape(96, 256), ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("has_bias", [True, False])
def test_linear_act_library_gelu_gpu(has_bias, monkeypatch):
    """The default serving path: library GEMM, then the bias_gelu kernel
    (with a bias) or torch's GELU (without)."""
    monkeypatch.setattr(G, "_FORCE_LIB", True)
    monkeypatch.setattr(G, "_FORCE_HAND", False)
    x, w, b = _linear_inputs(256)
    b = b if has_bias else None
    ref, bound = kc.gemm_ref(x.reshape(96, 128), w, b, 1, mid_round=True)
    y = G.linear_act(x.cuda(), w.cuda(), _cuda(b), G.ACT_GELU)
    assert y.shape == (2, 48, 256)
    kc.check(f"gpu linear_act library bias {has_bias}", y.reshape(96, 256),
             ref, bound)


def test_linear_act_bound_cpu():
    """The inputs and bounds of the linear_act GPU tests, on the CPU."""
    for n in (200, 256):
        x, w, b = _linear_inputs(n)
        for bias in (b, None):
            ref, bound = kc.gemm_ref(x.reshape(96, 128), w, bias, 1)
            y = G.linear_act(x.float(), w.float(),
                             None if bias is None else bias.float(),
                             G.ACT_GELU)
            assert y.shape == (2, 48, n)
            kc.check(f"cpu linear_act {n}", y.reshape(96, n), ref, bound)
