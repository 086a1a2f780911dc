"""Public op API: gfx950 HIP kernels on GPU, fp32 torch references on CPU.

Dispatch contract: on a GPU tensor the hand-written kernel MUST run — if the
in-tree extension is missing the call raises rather than silently falling back
(build contract: "make your ops fail loudly if their extension is missing on a
GPU box").  CPU tensors use the fp32 reference path so the whole model stack is
testable without hardware.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from . import reference as ref
from ._build import get_ext


def _ext_for(t: torch.Tensor, *grad_tensors, any_dtype: bool = False):
    """Dispatch: hand kernel on GPU for inference; differentiable torch
    composition when autograd needs to flow (training forward) — apart from
    attention, which has its own HIP backward (see `_attn_train_ext`), the
    custom kernels are forward-only, so grad-mode falls back to reference
    math on the SAME device (hipBLASLt/eager ROCm kernels), keeping
    LoRA/backward correct end-to-end.

    Most kernels are bf16-native (CDNA4 MFMA tiles); a non-bf16 GPU tensor
    (e.g. an fp32 research model) runs the reference composition on the same
    device rather than erroring.  Ops whose kernels take fp32 (sampling,
    softmax, AdamW) pass any_dtype=True.  A MISSING extension on a GPU box
    still fails loudly (get_ext(required=True))."""
    if torch.is_grad_enabled() and any(
            isinstance(g, torch.Tensor) and g.requires_grad
            for g in (t, *grad_tensors)):
        return None
    if t.is_cuda:
        if not any_dtype and t.dtype is not torch.bfloat16:
            get_ext(required=True)  # still verify the .so is present
            return None
        return _sync_wrapped(get_ext(required=True))
    return None


def _sync_wrapped(ext):
    from ..gpu.guard import SyncProxy, debug_sync_enabled

    return SyncProxy(ext) if debug_sync_enabled() else ext


def _attn_train_ext(q, k, v, causal: bool):
    """The extension, when a grad-mode attention call runs the HIP forward
    (saving the log-sum-exp) and the HIP backward: inputs on the GPU in bf16,
    head_dim 64 or 128, and not (causal with Sq > Sk).  None otherwise — CPU,
    fp32, other head dims, or MODAL_AMD_ATTN_BWD=ref (read at call time; the
    A/B switch back to the differentiable reference) keep the reference path.
    q/k/v are [B,H,S,D]-logical."""
    if not (torch.is_grad_enabled()
            and any(t.requires_grad for t in (q, k, v))):
        return None
    if os.environ.get("MODAL_AMD_ATTN_BWD", "") == "ref":
        return None
    if not all(t.is_cuda and t.dtype is torch.bfloat16 for t in (q, k, v)):
        return None
    if q.shape[-1] not in (64, 128) or (causal and q.shape[2] > k.shape[2]):
        return None
    return _sync_wrapped(get_ext(required=True))


def _d_contiguous(t):
    return t if t.stride(-1) == 1 else t.contiguous()


class _AttentionFn(torch.autograd.Function):
    """Differentiable flash attention on the gfx950 kernels.  q/k/v are
    [B,H,S,D]-logical with any strides (d contiguous); the forward saves o
    and one fp32 log-sum-exp per query row, the backward recomputes P from
    it (csrc/attention_bwd.hip) — O(S) extra memory, no score matrix.
    bshd=True returns o as [B,S,H,D] contiguous (attention_qkv)."""

    @staticmethod
    def forward(ctx, q, k, v, causal, scale, bshd, ext):
        q, k, v = _d_contiguous(q), _d_contiguous(k), _d_contiguous(v)
        if bshd:
            o, lse = ext.attention_fwd_lse_bshd(q, k, v, causal, scale)
        else:
            o, lse = ext.attention_fwd_lse(q, k, v, causal, scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal, ctx.scale, ctx.bshd, ctx.ext = causal, scale, bshd, ext
        return o

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, o, lse = ctx.saved_tensors
        if ctx.bshd:  # o and its gradient are [B,S,H,D]; the kernel wants BHSD
            o, dout = o.transpose(1, 2), dout.transpose(1, 2)
        dout = _d_contiguous(dout)

        def grad_like(t):  # sequence-major for sequence-major callers
            if ctx.bshd:
                B, H, S, D = t.shape
                return torch.empty(B, S, H, D, dtype=t.dtype,
                                   device=t.device).transpose(1, 2)
            return torch.empty(t.shape, dtype=t.dtype, device=t.device)

        dq, dk, dv = grad_like(q), grad_like(k), grad_like(v)
        ctx.ext.attention_bwd(q, k, v, o, lse, dout, dq, dk, dv, ctx.causal,
                              ctx.scale)
        return dq, dk, dv, None, None, None, None


def _attention(q, k, v, causal, scale, bshd: bool):
    """The dispatch of both attention entries.  q/k/v are [B,H,S,D]-logical
    with any strides; bshd=True returns o as [B,S,H,D] and hands the kernel
    the strided views as they are, bshd=False returns [B,H,S,D]."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    if k.shape[2] == 0:
        raise ValueError("attention: Sk must be at least 1, got Sk=0 (a query "
                         "with no key has no softmax)")
    ext = _attn_train_ext(q, k, v, causal)
    if ext is not None:
        return _AttentionFn.apply(q, k, v, causal, scale, bshd, ext)
    ext = _ext_for(q, k, v)
    if ext is None:
        o = ref.attention_ref(q, k, v, causal, scale)
        return o.transpose(1, 2) if bshd else o
    if bshd:
        return ext.attention_bshd(q, k, v, causal, scale)
    return ext.attention(q.contiguous(), k.contiguous(), v.contiguous(),
                         causal, scale)


def attention(q, k, v, causal: bool = False, scale: Optional[float] = None):
    """Flash attention (K1/K5/K7). q [B,Hq,Sq,D], k/v [B,Hkv,Sk,D] bf16.
    Differentiable on the GPU through the HIP backward.

    causal aligns the mask to the last key: row i sees keys <= i + Sk - Sq.
    With Sq > Sk the first Sq - Sk rows see no key and return exactly 0
    (their saved log-sum-exp is -inf, their gradients are 0; grad mode takes
    the reference path for this configuration).  No query at all (B, Hq or
    Sq zero) returns the empty tensor without a launch; Sk == 0 raises."""
    return _attention(q, k, v, causal, scale, False)


def attention_qkv(q, k, v, causal: bool = False, scale: Optional[float] = None):
    """Transpose-free attention for sequence-major models.

    q: [B, S, Hq, D] (any strides, d contiguous — e.g. a slice of a fused QKV
    projection); k/v: [B, Sk, Hkv, D].  Returns [B, S, Hq*D] contiguous,
    ready for the output projection.  On GPU the kernel reads the strided
    layouts directly and writes BSHD — no .contiguous() copies at all; in
    grad mode the backward reads the same views and the [B,S,Hq*D] output
    gradient in place.  Rows that see no key (causal, S > Sk), empty inputs
    and Sk == 0 behave as in `attention`.
    """
    B, S, Hq, D = q.shape
    o = _attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                   causal, scale, True)
    return o.reshape(B, S, Hq * D)


def paged_decode(q, k_cache, v_cache, block_table, seq_lens, block_size: int = 0,
                 scale: Optional[float] = None):
    """Decode attention over a (paged) KV cache (K6). q [B,Hq,D].
    Caches may be bf16 or float8_e4m3fn (fp8 halves KV bytes/token)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    ext = _ext_for(q)
    if ext is None:
        if k_cache.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            k_cache = k_cache.to(torch.float32)
            v_cache = v_cache.to(torch.float32)
        return ref.paged_decode_ref(q, k_cache, v_cache, block_table, seq_lens,
                                    block_size, scale)
    # .contiguous() also materializes expand()ed (stride-0) block tables —
    # the kernel indexes bt + row*stride and would read out of bounds.
    # block_table=None = contiguous (non-paged) cache mode.
    bt = block_table.contiguous() if block_table is not None else None
    return ext.paged_decode(q.contiguous(), k_cache, v_cache, bt,
                            seq_lens.int(), block_size, scale)


def paged_prefill(q, k_cache, v_cache, block_table, cu_q, seq_lens,
                  block_size: int, scale: Optional[float] = None,
                  max_q_len: Optional[int] = None):
    """Prefill attention over a paged KV cache (K6): causal attention of a
    ragged batch of NEW tokens against a cache that already holds their K/V
    — chunked prefill and the suffix after a prefix-cache hit.

    q [T,Hq,D]: rows cu_q[b]..cu_q[b+1] are sequence b's new tokens (cu_q
    int32 [B+1]); caches [blocks,Hkv,block_size,D], bf16 or float8_e4m3fn;
    block_table int32 [B,max_blocks]; seq_lens int32 [B], the cached length
    INCLUDING the new tokens, so query i of n_b sits at position
    seq_lens[b] - n_b + i.  max_q_len is a host-side bound on the longest
    run of new tokens (it sizes the grid, nothing is read back); None means
    T, which is always safe.  Returns [T,Hq,D]."""
    if block_table is None:
        raise ValueError("paged_prefill needs a block_table (there is no "
                         "contiguous-cache mode)")
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    ext = _ext_for(q)
    if ext is None:
        if k_cache.dtype not in (torch.float32, torch.float64, torch.bfloat16,
                                 torch.float16):
            k_cache = k_cache.to(torch.float32)
            v_cache = v_cache.to(torch.float32)
        return ref.paged_prefill_ref(q, k_cache, v_cache, block_table, cu_q,
                                     seq_lens, block_size, scale)
    # .contiguous() also materializes expand()ed (stride-0) block tables —
    # the kernel indexes bt + row*stride and would read out of bounds.
    return ext.paged_prefill(q.contiguous(), k_cache, v_cache,
                             block_table.contiguous(), cu_q.int().contiguous(),
                             seq_lens.int().contiguous(), block_size, scale,
                             q.shape[0] if max_q_len is None else max_q_len)


def groupnorm_silu(x, gamma, beta, groups: int = 32, eps: float = 1e-5,
                   do_silu: bool = True, out_nhwc: bool = False):
    """GroupNorm(+SiLU) of x [N,C,H,W].  out_nhwc=True returns the result as
    [N, H*W, C] — `groupnorm_silu(x).permute(0, 2, 3, 1).reshape(N, H*W, C)`
    — which the kernel writes directly (same statistics pass, an apply kernel
    that transposes its tile in LDS), so the sequence-major sections of the
    UNet/VAE take it without a transposing copy."""
    ext = _ext_for(x, gamma, beta)
    if ext is None:
        y = ref.groupnorm_silu_ref(x, gamma, beta, groups, eps, do_silu)
        if out_nhwc:
            N, C, H, W = x.shape
            y = y.permute(0, 2, 3, 1).reshape(N, H * W, C)
        return y
    fn = ext.groupnorm_silu_nhwc if out_nhwc else ext.groupnorm_silu
    return fn(x.contiguous(), gamma.float().contiguous(),
              beta.float().contiguous(), groups, eps, do_silu)


def layernorm(x, gamma, beta, eps: float = 1e-5):
    ext = _ext_for(x, gamma, beta)
    if ext is None:
        return ref.layernorm_ref(x, gamma, beta, eps)
    return ext.layernorm(x.contiguous(), gamma.float().contiguous(),
                         beta.float().contiguous(), eps)


def add_layernorm(x, y, gamma, beta, eps: float = 1e-5):
    """(x + y, layernorm(x + y)): a residual add and the norm of the next
    sub-layer from one read of x and y.  The sum is rounded to x's dtype and
    the norm works on the rounded sum, so both results equal `s = x + y`
    followed by `layernorm(s, ...)` bit for bit.  A last dimension that is
    no multiple of 8 runs exactly those two ops."""
    ext = _ext_for(x, y, gamma, beta)
    if ext is None or x.shape[-1] % 8 != 0 or x.shape != y.shape \
            or y.dtype is not x.dtype:
        s = x + y
        return s, layernorm(s, gamma, beta, eps)
    s, ln = ext.add_layernorm(x.contiguous(), y.contiguous(),
                              gamma.float().contiguous(),
                              beta.float().contiguous(), eps)
    return s, ln


def add_nhwc_to_nchw(res, h):
    """res [N,C,H,W] + h [N,H*W,C] -> [N,C,H,W], i.e.
    `res + h.reshape(N, H, W, C).permute(0, 3, 1, 2)` as one tiled-transpose
    kernel instead of a strided TensorIterator add."""
    N, C, H, W = res.shape
    ext = _ext_for(res, h)
    if ext is None or h.dtype is not res.dtype:
        return res + h.reshape(N, H, W, C).permute(0, 3, 1, 2)
    return ext.add_nhwc_to_nchw(res.contiguous(), h.contiguous())


def scaled_softmax(s, scale: float):
    """softmax((s * scale).float(), -1).to(s.dtype) for bf16 scores: one read
    and one write of the score matrix instead of the four-kernel chain.  The
    product is rounded to bf16 before the fp32 softmax, as in the chain.
    Rows must be contiguous with a multiple of 8 columns; anything else runs
    the torch expression."""
    ext = _ext_for(s)
    if ext is None or s.shape[-1] % 8 != 0 or s.shape[-1] == 0 \
            or not s.is_contiguous():
        return torch.softmax((s * scale).float(), dim=-1).to(s.dtype)
    return ext.scaled_softmax(s, scale)


def rmsnorm(x, gamma, eps: float = 1e-6):
    ext = _ext_for(x, gamma)
    if ext is None:
        return ref.rmsnorm_ref(x, gamma, eps)
    return ext.rmsnorm(x.contiguous(), gamma.float().contiguous(), eps)


def cfg_euler(x_t, eps_c, eps_u, guidance: float, dsigma: float):
    """Fused CFG combine + Euler update (K4)."""
    ext = _ext_for(x_t)
    if ext is None:
        return ref.cfg_euler_ref(x_t, eps_c, eps_u, guidance, dsigma)
    return ext.cfg_euler(x_t.contiguous(), eps_c.contiguous(),
                         eps_u.contiguous() if eps_u is not None else None,
                         guidance, dsigma)


def silu_mul(a, b):
    ext = _ext_for(a, b)
    if ext is None:
        return ref.silu_mul_ref(a, b)
    return ext.silu_mul(a.contiguous(), b.contiguous())


def geglu(a, b):
    ext = _ext_for(a, b)
    if ext is None:
        return ref.geglu_ref(a, b)
    return ext.geglu(a.contiguous(), b.contiguous())


def glu_fused(src, gelu: bool = False):
    """act(src[..., :I]) * src[..., I:] reading the fused projection output
    in place (no slice copies).  gelu=True -> GEGLU (SDXL FF), else SwiGLU
    (Llama gate_up)."""
    inner = src.shape[-1] // 2
    ext = _ext_for(src)
    if ext is None or inner % 8 != 0:
        a, b = src[..., :inner], src[..., inner:]
        return (ref.geglu_ref(a, b) if gelu else ref.silu_mul_ref(a, b))
    return ext.glu_fused(src.contiguous(), gelu)


def add_residual(a, b):
    ext = _ext_for(a, b)
    if ext is None:
        return (a.float() + b.float()).to(a.dtype)
    return ext.add_residual(a.contiguous(), b.contiguous())


def rope(x, cos, sin, positions=None, inplace: bool = False):
    """RoPE with host-precomputed tables. x [B,H,S,D] bf16.
    positions: None (0..S-1), [S] (shared across batch) or [B*S] (per-seq —
    the batched-decode case where every sequence sits at its own offset)."""
    ext = _ext_for(x)
    if ext is None:
        if positions is not None and positions.numel() == x.shape[0] * x.shape[2] \
                and x.shape[0] > 1:
            B, H, S, D = x.shape
            pos = positions.view(B, S).long()
            outs = [ref.rope_ref(x[b:b + 1], cos, sin, pos[b]) for b in range(B)]
            return torch.cat(outs, 0)
        return ref.rope_ref(x, cos, sin, positions.long() if positions is not None else None)
    # kernel is stride-aware (d contiguous required); inplace works on views
    # (e.g. q/k slices of a fused QKV projection — no copies at all)
    assert x.stride(-1) == 1, "rope needs contiguous head_dim"
    y = x if inplace else x.clone()
    pos = positions
    if pos is not None:
        pos = pos.int()
        if pos.numel() == x.shape[2] and x.shape[0] > 1:
            pos = pos.repeat(x.shape[0])
    ext.rope_(y, cos.float().contiguous(), sin.float().contiguous(), pos)
    return y


def rope_tables(max_seq: int, dim: int, base: float = 10000.0, device="cpu"):
    """Host-side cos/sin tables (guide App.B: no on-device trig)."""
    inv = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float64) / dim))
    t = torch.arange(max_seq, dtype=torch.float64)
    freqs = torch.outer(t, inv)
    return (freqs.cos().float().to(device), freqs.sin().float().to(device))


def repack_conv3x3_weight(weight: torch.Tensor) -> torch.Tensor:
    """[K,C,3,3] conv weight → the kernel's [9, Kpad, C16] layout (c
    contiguous per (tap, k) row so the MFMA A-fragment is one bf16x8 read;
    K padded to the 64-channel block, C to the 16-channel chunk)."""
    K, C = weight.shape[0], weight.shape[1]
    kpad = (K + 63) // 64 * 64
    c16 = (C + 15) // 16 * 16
    wr = torch.zeros(9, kpad, c16, dtype=torch.bfloat16, device=weight.device)
    w = weight.permute(2, 3, 0, 1).reshape(9, K, C)  # [tap, k, c]
    wr[:, :K, :C] = w.to(torch.bfloat16)
    return wr.contiguous()


def conv3x3(x, wr, bias, K: int, residual=None, raw_weight=None,
            upsample: bool = False, addend=None):
    """3x3 stride-1 pad-1 conv (K3). x [N,C,H,W] bf16; wr from
    repack_conv3x3_weight; bias fp32 [K]; optional fused residual add;
    upsample=True fuses a nearest-2x upsample of x into the conv read.
    addend [N,K] (x's dtype) is added per (image, output channel) to the
    rounded conv output — `conv3x3(x, ...) + addend[:, :, None, None]` in the
    kernel's epilogue; it cannot be combined with residual.
    raw_weight [K,C,3,3] drives the CPU/autograd reference path."""
    if addend is not None and residual is not None:
        raise ValueError("conv3x3: addend and residual cannot be combined")
    ext = _ext_for(x, raw_weight if raw_weight is not None else x, addend)
    if ext is not None and addend is not None:
        return ext.conv3x3(x.contiguous(), wr, bias, None, K, upsample,
                           addend.contiguous())
    if addend is not None:
        return conv3x3(x, wr, bias, K, raw_weight=raw_weight,
                       upsample=upsample) + addend[:, :, None, None]
    if ext is None:
        assert raw_weight is not None, "reference conv path needs raw_weight"
        xin = x
        if upsample:
            xin = torch.nn.functional.interpolate(x, scale_factor=2.0,
                                                  mode="nearest")
        y = torch.nn.functional.conv2d(
            xin.float(), raw_weight.float(), bias.float(), padding=1)
        if residual is not None:
            y = y + residual.float()
        return y.to(x.dtype)
    out = ext.conv3x3(x.contiguous(), wr, bias,
                      residual.contiguous() if residual is not None else None,
                      K, upsample)
    return out


def conv3x3_gn(x, wr, bias, K: int, gamma, beta, groups: int = 32,
               eps: float = 1e-5, residual=None, raw_weight=None,
               upsample: bool = False):
    """GroupNorm+SiLU fused into the K3 conv's staging read: one stats pass
    over x + the conv — the gn_norm write/read pass over the full tensor
    disappears."""
    ext = _ext_for(x, raw_weight if raw_weight is not None else x)
    if ext is None:
        assert raw_weight is not None
        h = torch.nn.functional.group_norm(x.float(), groups, gamma.float(),
                                           beta.float(), eps)
        h = torch.nn.functional.silu(h)
        if upsample:
            h = torch.nn.functional.interpolate(h, scale_factor=2.0,
                                                mode="nearest")
        y = torch.nn.functional.conv2d(h, raw_weight.float(), bias.float(),
                                       padding=1)
        if residual is not None:
            y = y + residual.float()
        return y.to(x.dtype)
    return ext.conv3x3_gn(x.contiguous(), wr, bias,
                          residual.contiguous() if residual is not None else None,
                          K, upsample, gamma.float().contiguous(),
                          beta.float().contiguous(), groups, eps)


def adamw_step(p, g, m, v, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, step=1):
    """Fused AdamW (K9); in-place on p/m/v."""
    ext = _ext_for(p, any_dtype=True)
    if ext is None:
        return ref.adamw_ref(p, g, m, v, lr, beta1, beta2, eps, wd, step)
    ext.adamw_(p, g.contiguous(), m, v, lr, beta1, beta2, eps, wd, step)
    return p


def sample(logits, temperature: float = 1.0, seed: int = 0):
    """Fused sampling (K8): gumbel-max over softmax(logits/T); T=0 → argmax."""
    ext = _ext_for(logits, any_dtype=True)
    if ext is None:
        if temperature <= 0:
            return logits.argmax(-1).int()
        g = torch.Generator(device="cpu").manual_seed(seed or 1)
        u = torch.rand(logits.shape, generator=g).clamp_min(1e-10)
        gumbel = -(-u.log()).log()
        return (logits.float() / temperature + gumbel).argmax(-1).int()
    return ext.sample_gumbel(logits.float().contiguous(), temperature, seed)


def wrap_int64(v: int) -> int:
    """Any Python int as the int64 with the same low 64 bits (seeds are
    64-bit patterns; an int64 tensor carries them to the kernel)."""
    v = int(v) & (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def _row_param(v, rows: int, dtype, device, name: str) -> torch.Tensor:
    """A per-row sampling parameter as a contiguous [rows] tensor on `device`:
    a Python scalar is broadcast by a device fill, a tensor must already have
    one value per row.  Nothing here reads a value back to the host."""
    if isinstance(v, torch.Tensor):
        if v.dim() == 0:
            v = v.expand(rows)
        if v.dim() != 1 or v.shape[0] != rows:
            raise ValueError(f"{name} must have one value per row ([{rows}]), "
                             f"got {tuple(v.shape)}")
        if v.device != device:
            raise ValueError(f"{name} is on {v.device}, logits on {device}")
        return v.to(dtype).contiguous()
    if dtype is torch.int64:
        v = wrap_int64(v)
    return torch.full((rows,), v, dtype=dtype, device=device)


def _check_logits_2d(logits):
    if logits.dim() != 2 or logits.shape[0] == 0 or logits.shape[1] == 0:
        raise ValueError(f"logits must be [rows, V], got {tuple(logits.shape)}")


def _filter_params(logits, temperature, top_k, top_p, min_p):
    rows, dev = logits.shape[0], logits.device
    return (_row_param(temperature, rows, torch.float32, dev, "temperature"),
            _row_param(0 if top_k is None else top_k, rows, torch.int32, dev,
                       "top_k"),
            _row_param(1.0 if top_p is None else top_p, rows, torch.float32,
                       dev, "top_p"),
            _row_param(0.0 if min_p is None else min_p, rows, torch.float32,
                       dev, "min_p"))


def sampling_cutoff(logits, temperature, top_k=None, top_p=None, min_p=None):
    """Per-row cutoff logit c_r of the top-k / top-p / min-p filters (K8):
    the filtered distribution of row r lives on {i : logits[r, i] >= c_r}.

    logits [B, V]; every parameter is a [B] tensor or a Python scalar that
    is broadcast; None is off (so are top_k 0 or >= V, top_p 1, min_p 0).
    top-p is applied to the survivors of top-k and renormalised over them;
    ties at a threshold are all kept.  Rows with every filter off, or with
    temperature <= 0, get -inf.  Returns float32 [B]."""
    _check_logits_2d(logits)
    t, k, p, q = _filter_params(logits, temperature, top_k, top_p, min_p)
    ext = _ext_for(logits, any_dtype=True)
    if ext is None:
        return ref.sampling_cutoff_ref(logits, t, k, p, q)
    return ext.sampling_cutoff(logits.float().contiguous(), t, k, p, q)


def sample_batch(logits, temperature, top_k=None, top_p=None, min_p=None,
                 seeds=None, counters=None):
    """Batched sampling with per-row parameters (K8): gumbel-max over the
    filtered softmax(logits/T), T <= 0 -> first arg-max.

    Each parameter is a [B] tensor or a Python scalar that is broadcast;
    None is off, seeds default to 0 and counters to the row index.  The draw
    of a row depends on its (seed, counter, logits) only — not on its index
    or on the rest of the batch.  `sample(x, T, seed=s)` is the special case
    `sample_batch(x, T, seeds=s, counters=arange(B))`.  Returns int32 [B]."""
    _check_logits_2d(logits)
    rows, dev = logits.shape[0], logits.device
    s = _row_param(0 if seeds is None else seeds, rows, torch.int64, dev,
                   "seeds")
    c = (torch.arange(rows, dtype=torch.int64, device=dev) if counters is None
         else _row_param(counters, rows, torch.int64, dev, "counters"))
    ext = _ext_for(logits, any_dtype=True)
    if ext is None:
        t, k, p, q = _filter_params(logits, temperature, top_k, top_p, min_p)
        return ref.sample_batch_ref(logits, t, k, p, q, s, c)
    lg = logits.float().contiguous()
    if top_k is None and top_p is None and min_p is None:
        # unfiltered calls launch no cutoff kernel at all
        t = _row_param(temperature, rows, torch.float32, dev, "temperature")
        return ext.sample_batch(lg, t, s, c, None)
    t, k, p, q = _filter_params(logits, temperature, top_k, top_p, min_p)
    return ext.sample_batch(lg, t, s, c, ext.sampling_cutoff(lg, t, k, p, q))


def softmax(x):
    ext = _ext_for(x, any_dtype=True)
    if ext is None:
        return torch.softmax(x.float(), dim=-1)
    return ext.softmax_fwd(x.float().contiguous())


# ---- mixture-of-experts FFN.  Supported shapes (csrc/moe.hip): E <= 128,
# 1 <= top_k <= min(E, 8), dim and ffn_dim multiples of 64, any N >= 1,
# contiguous operands.  The checks below run on every device, before the
# dispatch, so the reference path refuses exactly what the kernel refuses.

def _check_moe_route(logits, top_k):
    if logits.dim() != 2 or logits.shape[0] < 1:
        raise ValueError(f"logits must be [N, E] with N >= 1, got "
                         f"{tuple(logits.shape)}")
    E = logits.shape[1]
    if not 1 <= E <= 128:
        raise ValueError(f"logits has E={E} experts (supported: 1..128)")
    if not isinstance(top_k, int) or not 1 <= top_k <= min(E, 8):
        raise ValueError(f"top_k={top_k!r} (supported: 1..min(E, 8) = "
                         f"{min(E, 8)})")


def moe_route(logits, top_k: int):
    """Top-k expert routing.  logits [N, E] -> (weights [N, k] fp32, idx
    [N, k] int32): the k largest logits per row in descending order, ties to
    the lower expert index; weights = softmax over those k logits.  One
    kernel, nothing read back to the host."""
    _check_moe_route(logits, top_k)
    ext = _ext_for(logits, any_dtype=True)
    if ext is None:
        return ref.moe_route_ref(logits, top_k)
    return ext.moe_route(logits.float().contiguous(), top_k)


def _check_moe_ffn(x, gate_up, down, weights, idx):
    if x.dim() != 2 or x.shape[0] < 1:
        raise ValueError(f"x must be [N, dim] with N >= 1, got "
                         f"{tuple(x.shape)}")
    N, d = x.shape
    if d % 64 != 0:
        raise ValueError(f"x has dim={d} (must be a multiple of 64)")
    if gate_up.dim() != 3 or gate_up.shape[2] != d \
            or gate_up.shape[1] % 2 != 0:
        raise ValueError(f"gate_up must be [E, 2*ffn_dim, dim={d}], got "
                         f"{tuple(gate_up.shape)}")
    E, F = gate_up.shape[0], gate_up.shape[1] // 2
    if not 1 <= E <= 128:
        raise ValueError(f"gate_up has E={E} experts (supported: 1..128)")
    if F % 64 != 0 or F < 64:
        raise ValueError(f"gate_up has ffn_dim={F} (must be a multiple of "
                         f"64)")
    if tuple(down.shape) != (E, d, F):
        raise ValueError(f"down must be [E={E}, dim={d}, ffn_dim={F}], got "
                         f"{tuple(down.shape)}")
    if idx.dtype is not torch.int32:
        raise TypeError(f"idx must be int32, got {idx.dtype}")
    if idx.dim() != 2 or idx.shape[0] != N \
            or not 1 <= idx.shape[1] <= min(E, 8):
        raise ValueError(f"idx must be [N={N}, top_k] with top_k in "
                         f"1..min(E, 8) = {min(E, 8)}, got {tuple(idx.shape)}")
    if weights.shape != idx.shape:
        raise ValueError(f"weights must have idx's shape "
                         f"{tuple(idx.shape)}, got {tuple(weights.shape)}")
    for name, t in (("x", x), ("gate_up", gate_up), ("down", down)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.dtype is not x.dtype or t.device != x.device:
            raise ValueError(f"{name} must have x's dtype and device "
                             f"({x.dtype}, {x.device}), got {t.dtype}, "
                             f"{t.device}")


def moe_ffn(x, gate_up, down, weights, idx):
    """Routed SwiGLU FFN over E experts, fused (csrc/moe.hip):
    out[t] = sum_j weights[t, j] * FFN_{idx[t, j]}(x[t]).

    x [N, dim]; gate_up [E, 2*ffn_dim, dim] (gate rows, then up rows); down
    [E, dim, ffn_dim]; weights fp32 / idx int32 [N, k] as moe_route returns
    them.  Precondition: idx values in [0, E) and distinct per token —
    moe_route always satisfies it; the values are never read on the host.
    On the GPU nothing depends on the routing but the data, so the call
    captures into a graph; the result is bitwise reproducible.  Returns
    [N, dim] in x's dtype."""
    _check_moe_ffn(x, gate_up, down, weights, idx)
    ext = _ext_for(x, gate_up, down, weights)
    if ext is None:
        return ref.moe_ffn_ref(x, gate_up, down, weights, idx)
    return ext.moe_ffn(x, gate_up, down, weights.float().contiguous(),
                       idx.contiguous())


# ---- int4 weight-only linear.  Supported shapes (csrc/linear_w4.hip): K a
# multiple of 128 (the quantization group), N a multiple of 64, any number of
# rows >= 1, contiguous weights.  The checks below run on every device,
# before the dispatch, so the reference path refuses exactly what the kernel
# refuses.

def _check_w4_weight(weight):
    if weight.dim() != 2:
        raise ValueError(f"weight must be [N, K], got {tuple(weight.shape)}")
    if weight.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"weight must be bf16 or fp32, got {weight.dtype}")
    N, K = weight.shape
    if K < 128 or K % 128 != 0:
        raise ValueError(f"weight has K={K} (must be a multiple of 128)")
    if N < 64 or N % 64 != 0:
        raise ValueError(f"weight has N={N} (must be a multiple of 64)")
    if not weight.is_contiguous():
        raise ValueError("weight must be contiguous")


def _check_w4(qweight, scales):
    """Returns (N, K) of a packed weight."""
    if qweight.dtype not in (torch.int32, torch.uint8):
        raise TypeError(f"qweight must be int32 or uint8, got "
                        f"{qweight.dtype}")
    if scales.dtype is not torch.bfloat16:
        raise TypeError(f"scales must be bf16, got {scales.dtype}")
    if qweight.dim() != 2 or scales.dim() != 2:
        raise ValueError(f"qweight must be [N, K/8] and scales [N, K/128], "
                         f"got {tuple(qweight.shape)}, {tuple(scales.shape)}")
    N = qweight.shape[0]
    K = qweight.shape[1] * (8 if qweight.dtype is torch.int32 else 2)
    if K < 128 or K % 128 != 0:
        raise ValueError(f"qweight has K={K} (must be a multiple of 128)")
    if N < 64 or N % 64 != 0:
        raise ValueError(f"qweight has N={N} (must be a multiple of 64)")
    if tuple(scales.shape) != (N, K // 128):
        raise ValueError(f"scales must be [N={N}, K/128={K // 128}], got "
                         f"{tuple(scales.shape)}")
    if scales.device != qweight.device:
        raise ValueError(f"scales is on {scales.device}, qweight on "
                         f"{qweight.device}")
    for name, t in (("qweight", qweight), ("scales", scales)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    return N, K


def quantize_w4(weight):
    """weight [N, K] (bf16 or fp32) -> (qweight int32 [N, K/8], scales bf16
    [N, K/128]): symmetric 4-bit quantization in groups of 128 along K.

    scale = bf16(absmax(group) / 7), 1 for an all-zero group;
    q = clamp(round_half_even(w / scale), -8, 7); the dequantized weight is
    float(scale) * q exactly.  The packing (eight weights to a word) is the
    kernel's and is described at the top of csrc/linear_w4.hip;
    `dequantize_w4` inverts it."""
    _check_w4_weight(weight)
    return ref.quantize_w4_ref(weight)


def dequantize_w4(qweight, scales):
    """The dequantized weight w_hat, fp32 [N, K], exact."""
    _check_w4(qweight, scales)
    return ref.dequantize_w4_ref(qweight, scales)


def linear_w4(x, qweight, scales):
    """x [..., K] . w_hat^T with int4 weights (quantize_w4), K2.

    On the GPU in bf16 without grad this is the csrc/linear_w4.hip kernel:
    nibbles become MFMA operands in registers, the group scale multiplies
    each group's fp32 sum, so no dequantized weight is ever rounded; K is
    split deterministically, the result of a row is bitwise reproducible and
    independent of the other rows, and the call captures into a graph.
    Anywhere else it is `linear(x, dequantize_w4(...).to(x.dtype))` on the
    same device, which is differentiable in x.  Returns [..., N] in x's
    dtype."""
    N, K = _check_w4(qweight, scales)
    if not x.is_floating_point():
        raise TypeError(f"x must be floating point, got {x.dtype}")
    if x.dim() < 1 or x.shape[-1] != K:
        raise ValueError(f"x must be [..., K={K}], got {tuple(x.shape)}")
    if x.numel() == 0:
        raise ValueError(f"x has no rows: {tuple(x.shape)}")
    if x.device != qweight.device:
        raise ValueError(f"x is on {x.device}, qweight on {qweight.device}")
    ext = _ext_for(x)
    if ext is None:
        return ref.linear_w4_ref(x, qweight, scales)
    y = ext.linear_w4(x.reshape(-1, K).contiguous(), qweight, scales)
    return y.view(*x.shape[:-1], N)
