"""bge-m3 style embedding encoder (XLM-RoBERTa-large architecture), MI355X-native.

Replaces the reference's llama.cpp GGUF embedding path
(reference: pkg/localllm/llama.go:104-180 — tokenize -> llama_encode
non-causal -> mean pooling -> L2 norm) with a from-scratch PyTorch-ROCm
forward whose hot ops are hand-written HIP/CDNA4 kernels:

- GEMMs (QKV / attn-out / FFN): hipBLASLt via torch.matmul (bf16, fp32 accum)
- attention: non-causal flash-style HIP kernel (ops.attention) when native,
  torch scaled_dot_product_attention otherwise
- LayerNorm + residual, bias+GELU, masked mean-pool + L2 norm: fused HIP
  kernels (ops.encoder) when native

Architecture facts (XLM-R large / bge-m3): vocab 250002, hidden 1024,
24 layers, 16 heads, FFN 4096, GELU, post-LayerNorm, learned positions,
pad_id 1, position offset 2. Weights are random-init (no network access);
the benchmark metric is embed docs/sec at reference-identical shape.
"""

import math
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass
class BgeM3Config:
    vocab_size: int = 250002
    hidden_size: int = 1024
    num_layers: int = 24
    num_heads: int = 16
    intermediate_size: int = 4096
    max_position: int = 8194
    pad_token_id: int = 1
    layer_norm_eps: float = 1e-5
    pooling: str = "mean"  # "mean" (reference llama.go pooling) or "cls"

    @classmethod
    def tiny(cls, **kw):
        d = dict(vocab_size=1024, hidden_size=128, num_layers=2, num_heads=4,
                 intermediate_size=256, max_position=512)
        d.update(kw)
        return cls(**d)


def _gelu(x):
    return F.gelu(x)


def _fused_ok(x):
    """Fused HIP kernels are inference-only (no autograd graph)."""
    return (x.is_cuda and x.dtype == torch.bfloat16
            and not torch.is_grad_enabled())


class _EncoderLayer(nn.Module):
    def __init__(self, cfg: BgeM3Config):
        super().__init__()
        h = cfg.hidden_size
        self.qkv = nn.Linear(h, 3 * h)
        self.attn_out = nn.Linear(h, h)
        self.ln1 = nn.LayerNorm(h, eps=cfg.layer_norm_eps)
        self.ffn_in = nn.Linear(h, cfg.intermediate_size)
        self.ffn_out = nn.Linear(cfg.intermediate_size, h)
        self.ln2 = nn.LayerNorm(h, eps=cfg.layer_norm_eps)
        self.num_heads = cfg.num_heads
        self.head_dim = h // cfg.num_heads

    def forward(self, x, attn_bias):
        b, s, h = x.shape
        if _fused_ok(x):
            from nornicdb_amd.ops.gemm import linear_act
            qkv = linear_act(x, self.qkv.weight, self.qkv.bias)
        else:
            qkv = self.qkv(x)
        qkv = qkv.view(b, s, 3, self.num_heads, self.head_dim)
        q, k, v = qkv.unbind(dim=2)  # [b, s, nh, hd] strided views
        from nornicdb_amd.ops.attention import (flash_attention_bshd,
                                                flash_attention_nc)

        if attn_bias is None and _fused_ok(x):
            # zero-transpose path: stride-aware HIP flash attention
            a = flash_attention_bshd(q, k, v).reshape(b, s, h)
        else:
            a = flash_attention_nc(q.transpose(1, 2), k.transpose(1, 2),
                                   v.transpose(1, 2), attn_bias)
            a = a.transpose(1, 2).reshape(b, s, h)
        if _fused_ok(x):
            from nornicdb_amd.ops import encoder as eops
            from nornicdb_amd.ops.gemm import ACT_GELU, linear_act

            # all four GEMMs go through linear_act, whose default dispatch
            # (NORNICDB_GEMM=auto) routes them to hipBLASLt, with bias+GELU
            # as a fused HIP kernel behind ffn_in; NORNICDB_GEMM=hand
            # selects the hand-written MFMA kernels (bias and GELU in the
            # epilogue) instead.
            x = eops.add_layernorm(
                x, linear_act(a, self.attn_out.weight, self.attn_out.bias),
                self.ln1.weight, self.ln1.bias, self.ln1.eps)
            f = linear_act(
                linear_act(x, self.ffn_in.weight, self.ffn_in.bias, ACT_GELU),
                self.ffn_out.weight, self.ffn_out.bias)
            x = eops.add_layernorm(x, f, self.ln2.weight, self.ln2.bias,
                                   self.ln2.eps)
        else:
            x = self.ln1(x + self.attn_out(a))
            f = self.ffn_out(_gelu(self.ffn_in(x)))
            x = self.ln2(x + f)
        return x


class BgeM3Encoder(nn.Module):
    def __init__(self, cfg: BgeM3Config = None):
        super().__init__()
        self.cfg = cfg or BgeM3Config()
        c = self.cfg
        self.tok_emb = nn.Embedding(c.vocab_size, c.hidden_size, padding_idx=c.pad_token_id)
        self.pos_emb = nn.Embedding(c.max_position, c.hidden_size)
        self.emb_ln = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.layers = nn.ModuleList(_EncoderLayer(c) for _ in range(c.num_layers))

    @torch.no_grad()
    def init_small(self, std=0.02):
        for p in self.parameters():
            if p.dim() > 1:
                p.normal_(0, std)
            else:
                p.zero_()
        # LayerNorm gains must be 1, not 0
        for m in self.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.fill_(1.0)
        return self

    def forward(self, token_ids: torch.Tensor, attention_mask: torch.Tensor = None):
        """token_ids [B, S] int64 -> L2-normalized embeddings [B, H].

        attention_mask: [B, S] with 1 = real token, 0 = padding (optional).
        """
        b, s = token_ids.shape
        pos = torch.arange(2, s + 2, device=token_ids.device)  # XLM-R offset
        x = self.tok_emb(token_ids) + self.pos_emb(pos)[None]
        x = self.emb_ln(x)

        attn_bias = None
        if attention_mask is not None:
            attn_bias = torch.where(
                attention_mask[:, None, None, :].bool(),
                torch.zeros((), device=x.device, dtype=x.dtype),
                torch.full((), float("-inf"), device=x.device, dtype=x.dtype),
            )
        for layer in self.layers:
            x = layer(x, attn_bias)

        if self.cfg.pooling == "cls":
            pooled = x[:, 0].float()
        elif _fused_ok(x):
            from nornicdb_amd.ops import encoder as eops

            return eops.mean_pool_l2norm(x, attention_mask)
        else:
            if attention_mask is None:
                pooled = x.mean(dim=1)
            else:
                m = attention_mask[..., None].to(x.dtype)
                pooled = (x * m).sum(1) / m.sum(1).clamp_min(1)
            pooled = pooled.float()
        return pooled / torch.linalg.vector_norm(pooled, dim=-1, keepdim=True).clamp_min(1e-12)
