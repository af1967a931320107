"""Tests aimed at the structure of the encoder flash-attention kernel.

The kernel keeps P in registers, with the K fragment's rows permuted so that
P comes out in the key order in which V is fetched transposed, walks K/V in
64-key tiles with 256 query rows
per workgroup, and keeps the exact running maximum. Each test below goes
after one of those: an exact selector (any mismatch of key order, tile offset
or query-row ownership picks a wrong V row), a maximum that arrives in the
last (or first) tile, random inputs at sizes that leave query blocks empty or
need more than one workgroup per head, and the memory next to the inputs.

Only the public entry points are used, so the file runs on any kernel behind
them.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

from nornicdb_amd.ops.attention import flash_attention_bshd, flash_attention_nc

D = 64


def _ref_bshd(q, k, v):
    """fp32 attention on [B,S,H,D] tensors, returned as [B,S,H,D]."""
    o = F.scaled_dot_product_attention(q.float().transpose(1, 2),
                                       k.float().transpose(1, 2),
                                       v.float().transpose(1, 2))
    return o.transpose(1, 2)


def _run_bshd_views(q, k, v):
    """Pack [B,S,H,D] q,k,v into one [B,S,3,H,D] tensor (the layout the qkv
    projection produces) and run the kernel on its unbind(2) views."""
    qkv = torch.stack([q, k, v], dim=2).contiguous()
    qv, kv, vv = qkv.unbind(2)
    assert not qv.is_contiguous()
    with torch.no_grad():
        return flash_attention_bshd(qv, kv, vv)


# ---------------------------------------------------------------------------
# selector: exact
# ---------------------------------------------------------------------------

SELECTOR_SHAPES = [(1, 1, 64), (2, 3, 192), (1, 2, 320), (1, 2, 448)]


@functools.lru_cache(maxsize=None)
def _selector_case(b, h, s):
    """CPU tensors [B,S,H,D]: K rows random +-2, Q row i = K row pi(i) with a
    permutation per (b,h), V[j][d] = ((7j + 3d) mod 509) - 254, and the
    expected output V[pi(i)]."""
    g = torch.Generator().manual_seed(1000 + s)
    k = (torch.randint(0, 2, (b, s, h, D), generator=g) * 4 - 2).float()
    perm = torch.stack([torch.stack([torch.randperm(s, generator=g)
                                     for _ in range(h)]) for _ in range(b)])
    idx = perm.permute(0, 2, 1)[..., None].expand(b, s, h, D)   # [B,S,H,D]
    q = torch.gather(k, 1, idx)
    j = torch.arange(s)[:, None]
    d = torch.arange(D)[None, :]
    v1 = (((7 * j + 3 * d) % 509) - 254).float()                # [S,D]
    v = v1[None, :, None, :].expand(b, s, h, D).contiguous()
    want = torch.gather(v, 1, idx)
    # the generators' own guarantees, on the CPU
    assert torch.unique(v1, dim=0).shape[0] == s
    logits = torch.einsum("bihd,bjhd->bhij", q, k) / 8.0
    top2 = logits.topk(2, dim=-1).values
    assert (top2[..., 0] - top2[..., 1]).min().item() >= 14.0
    assert torch.equal(logits.argmax(-1), perm)
    bf = torch.bfloat16
    assert torch.equal(v.to(bf).float(), v) and torch.equal(k.to(bf).float(), k)
    return q.to(bf), k.to(bf), v.to(bf), want


def _check_selector(out, want):
    err = (out.float().cpu() - want).abs().max().item()
    print(f"selector max |out - V[pi(i)]| = {err}")
    assert err <= 0.25, f"selector picked a wrong or mixed V row: {err}"


@pytest.mark.gpu
@pytest.mark.parametrize("b,h,s", SELECTOR_SHAPES)
def test_selector_reference(b, h, s):
    """The fp32 reference itself returns V[pi(i)] to within 4e-4."""
    q, k, v, want = _selector_case(b, h, s)
    ref = _ref_bshd(q.cuda(), k.cuda(), v.cuda()).cpu()
    assert (ref - want).abs().max().item() <= 4e-4


@pytest.mark.gpu
@pytest.mark.parametrize("b,h,s", SELECTOR_SHAPES)
def test_selector_nc(b, h, s):
    q, k, v, want = _selector_case(b, h, s)
    with torch.no_grad():
        out = flash_attention_nc(q.cuda().transpose(1, 2), k.cuda().transpose(1, 2),
                                 v.cuda().transpose(1, 2))
    _check_selector(out.transpose(1, 2), want)


@pytest.mark.gpu
@pytest.mark.parametrize("b,h,s", SELECTOR_SHAPES)
def test_selector_bshd_views(b, h, s):
    q, k, v, want = _selector_case(b, h, s)
    out = _run_bshd_views(q.cuda(), k.cuda(), v.cuda())
    assert out.is_contiguous() and out.shape == (b, s, h, D)
    _check_selector(out, want)


# ---------------------------------------------------------------------------
# the running maximum jumps after O has accumulated (or never moves again)
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pos", ["last", "first"])
def test_late_maximum(pos):
    b, h, s = 2, 4, 256
    g = torch.Generator().manual_seed(77)
    q = torch.randn(b, s, h, D, generator=g)
    k = torch.randn(b, s, h, D, generator=g)
    v = torch.randn(b, s, h, D, generator=g)
    u = torch.randn(b, 1, h, D, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    # even query rows and one key share a strong component along u: their
    # logit at that key is about 12*12/8 = 18, against a spread of about 2
    q[:, 0::2] += 12.0 * u
    kpos = s - 1 if pos == "last" else 0
    k[:, kpos:kpos + 1] += 12.0 * u
    q, k, v = (t.to(torch.bfloat16).cuda() for t in (q, k, v))
    ref = _ref_bshd(q, k, v)
    logits = torch.einsum("bihd,bjhd->bhij", q.float(), k.float()) / 8.0
    hit = (logits.argmax(-1) == kpos).float().mean().item()
    assert 0.45 <= hit <= 0.6, hit       # the spike wins on the even rows only
    out = _run_bshd_views(q, k, v)
    err = (out.float() - ref).abs().max().item()
    print(f"late maximum ({pos}): max err {err}")
    assert err < 0.05, f"max err {err}"
    with torch.no_grad():
        out2 = flash_attention_nc(q.transpose(1, 2), k.transpose(1, 2),
                                  v.transpose(1, 2)).transpose(1, 2)
    assert (out2.float() - ref).abs().max().item() < 0.05


# ---------------------------------------------------------------------------
# random inputs at the awkward sizes, production layout
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("b,h,s", [(3, 2, 64), (1, 5, 192), (2, 16, 256), (1, 2, 512)])
def test_random_bshd_views(b, h, s):
    g = torch.Generator().manual_seed(5 + s)
    q, k, v = (torch.randn(b, s, h, D, generator=g).to(torch.bfloat16).cuda()
               for _ in range(3))
    ref = _ref_bshd(q, k, v)
    out = _run_bshd_views(q, k, v)
    diff = (out.float() - ref).abs()
    print(f"random B{b} H{h} S{s}: max err {diff.max().item():.3e} "
          f"mean err {diff.mean().item():.3e}")
    assert diff.max().item() < 0.05


# ---------------------------------------------------------------------------
# memory next to the inputs
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("b,h,s", [(1, 2, 64), (2, 3, 320)])
def test_neighbouring_memory(b, h, s):
    """Inputs are views cut from one larger buffer with a sentinel-filled,
    output-sized guard before and after them; neither the guards nor the
    inputs may change."""
    n_out = b * s * h * D
    n_in = 3 * n_out
    sentinel = -12288.0   # exact in bf16
    g = torch.Generator().manual_seed(9 + s)
    buf = torch.full((n_out + n_in + n_out,), sentinel, dtype=torch.bfloat16)
    buf[n_out:n_out + n_in] = torch.randn(n_in, generator=g).to(torch.bfloat16)
    buf = buf.cuda()
    before = buf.clone()
    qkv = buf[n_out:n_out + n_in].view(b, s, 3, h, D)
    qv, kv, vv = qkv.unbind(2)
    with torch.no_grad():
        out = flash_attention_bshd(qv, kv, vv)
    torch.cuda.synchronize()
    assert torch.equal(buf, before), "inputs or guards were written"
    assert (buf[:n_out] == sentinel).all() and (buf[-n_out:] == sentinel).all()
    ref = _ref_bshd(qv, kv, vv)
    assert torch.isfinite(out.float()).all()
    assert (out.float() - ref).abs().max().item() < 0.05
