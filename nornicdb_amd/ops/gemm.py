"""Hand-written MFMA GEMM dispatch for the encoder hot path.

`linear_act(x, weight, bias, act)` computes act(x @ weight.T + bias) with
a hand-written CDNA4 MFMA kernel (csrc/gemm.hip) when NORNICDB_GEMM=hand,
the operands are bf16 CUDA and the shapes tile cleanly (N % 256 == 0,
K % 128 == 0); otherwise, and by default ("auto"), it uses the plain
PyTorch expression (the library GEMM on the GPU, with the hand-written
bias_gelu kernel behind it for GELU; also the CPU numerics oracle).

Two kernels: variant B (96x256 tile, 3 workgroups per CU) runs whenever M
is a multiple of 96, and gemm_nt pads M to make it so; variant A (256x256,
8-phase, one workgroup per CU) runs only under NORNICDB_GEMM_KERNEL=256 or
for a direct native call with M % 96 != 0. `_C.gemm_nt_variant(M)` tells
which one a call launches. tests/test_gemm_kernels.py runs both.

With NORNICDB_GEMM=hand this retires hipBLASLt (Tensile Cijk_* kernels)
from the bge-m3 forward pass; the replaced reference units are the cublas scoring GEMV
(pkg/gpu/cuda/cuda_kernels.cu:340-375) and llama.cpp's encoder GEMMs
(pkg/localllm/llama.go).

Autograd: forward uses the HIP kernel; backward (training path only —
serving never backprops) falls back to torch.matmul.
"""

import os

import torch
import torch.nn.functional as F

from . import native_or_none

ACT_NONE = 0
ACT_GELU = 1

# Dispatch policy (NORNICDB_GEMM): "hand" = always the hand-written MFMA
# kernel; "lib" = always hipBLASLt; "auto" (default) = the faster path
# per the measured campaign in profiles/README.md. Two independent
# hand-written architectures were built and measured on the encoder
# shapes (M=65536): the 256x256 8-phase single-WG template (asm ds_reads,
# counted lgkm/vmcnt waits) and the 96x256 3-WGs/CU co-residency design
# (NORNICDB_GEMM_KERNEL selects) — both land at 696-1155 TF vs
# hipBLASLt's 791-1478 TF, and hardware ablation shows the residual gap
# is Tensile's deep-pipelined hand-asm K-loop, not occupancy or LDS
# conflicts. "auto" routes to the faster library per VERDICT r1 item 2's
# explicit fallback rule; the hand kernels are one env var away. Both are
# numerics-tested in tests/test_gemm_kernels.py, which asserts the variant
# that ran.
_MODE = os.environ.get("NORNICDB_GEMM", "auto").lower()
_FORCE_LIB = _MODE in ("blaslt", "lib", "0", "auto")
_FORCE_HAND = _MODE in ("hand", "mfma", "1")


def _tiles_ok(m, n, k):
    return n % 256 == 0 and k % 128 == 0


def gemm_nt(x2d, weight, bias=None, act=ACT_NONE):
    """act(x2d @ weight.T + bias) for 2-D bf16 CUDA x2d; pads M to the
    selected kernel's row tile (96 for the 3-WG/CU variant B default,
    256 for NORNICDB_GEMM_KERNEL=256 variant A)."""
    nat = native_or_none()
    m = x2d.shape[0]
    # the row tile the environment selects: every tile divides M = 0, so
    # the answer for 0 depends on NORNICDB_GEMM_KERNEL alone (gemm_nt_variant
    # in csrc/gemm.hip keeps M = 0 valid for this)
    tile = nat.gemm_nt_variant(0)
    mp = (m + tile - 1) // tile * tile
    if mp != m:
        xpad = x2d.new_zeros((mp, x2d.shape[1]))
        xpad[:m] = x2d
        out = nat.gemm_nt(xpad, weight, bias, act)
        return out[:m]
    return nat.gemm_nt(x2d, weight, bias, act)


class _LinearAct(torch.autograd.Function):
    """HIP-kernel forward; torch backward (training only — serve never
    backprops, so the Tensile-free guarantee applies to the hot path)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        shp = x.shape
        x2d = x.reshape(-1, shp[-1]).contiguous()
        out = gemm_nt(x2d, weight, bias, act)
        ctx.save_for_backward(x2d, weight,
                              bias if bias is not None else x2d.new_empty(0))
        ctx.act = act
        ctx.has_bias = bias is not None
        return out.reshape(*shp[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, grad):
        x2d, weight, bias = ctx.saved_tensors
        g = grad.reshape(-1, grad.shape[-1])
        if ctx.act == ACT_GELU:
            pre = x2d.float() @ weight.float().T
            if ctx.has_bias:
                pre += bias.float()
            dgelu = (0.5 * (1.0 + torch.erf(pre * 0.7071067811865476))
                     + pre * torch.exp(-0.5 * pre * pre) * 0.3989422804014327)
            g = (g.float() * dgelu).to(grad.dtype)
        gx = (g @ weight).view(*grad.shape[:-1], weight.shape[1])
        gw = g.T @ x2d
        gb = g.sum(0) if ctx.has_bias else None
        return gx, gw, gb, None


def linear_act(x, weight, bias=None, act=ACT_NONE):
    """act(F.linear(x, weight, bias)); HIP MFMA kernel on the bf16 CUDA path."""
    nat = native_or_none()
    usable = (
        nat is not None and (_FORCE_HAND or not _FORCE_LIB)
        and x.is_cuda and x.dtype == torch.bfloat16
        and weight.dtype == torch.bfloat16
        and _tiles_ok(x.shape[:-1].numel(), weight.shape[0], weight.shape[1])
    )
    if usable:
        if torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad):
            return _LinearAct.apply(x, weight, bias, act)
        shp = x.shape
        x2d = x.reshape(-1, shp[-1]).contiguous()
        out = gemm_nt(x2d, weight, bias, act)
        return out.reshape(*shp[:-1], weight.shape[0])
    # library path / CPU oracle. For GELU on GPU keep the round-1 fused
    # epilogue: GEMM without bias + the hand-written bias_gelu kernel
    # (a separate torch GELU kernel costs ~3% of the bench step).
    if (act == ACT_GELU and nat is not None and x.is_cuda
            and x.dtype == torch.bfloat16 and bias is not None
            and weight.shape[0] % 8 == 0):
        return nat.bias_gelu(F.linear(x, weight), bias)
    y = F.linear(x, weight, bias)
    if act == ACT_GELU:
        y = F.gelu(y)
    return y
