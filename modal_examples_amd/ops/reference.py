"""Plain PyTorch fp32 reference implementations of every HIP op.

These are the ground truth the GPU numerics tests compare the gfx950 kernels
against (per the build contract: "numerics tests for a HIP kernel compare it
against a plain PyTorch fp32 reference of the same op"), and the CPU execution
path for hermetic tests.
"""
from __future__ import annotations

import math
from typing import Optional

import torch


def attention_ref(q, k, v, causal: bool = False, scale: Optional[float] = None):
    """q [B,Hq,Sq,D], k/v [B,Hkv,Sk,D] → [B,Hq,Sq,D]; GQA by head repeat.

    The causal mask is aligned to the last key (offset Sk - Sq).  With
    Sq > Sk the first Sq - Sk query rows see no key: their output is zero,
    and so are their gradients."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    qf, kf, vf = _wide(q), _wide(k), _wide(v)
    if Hkv != Hq:
        rep = Hq // Hkv
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    hidden = None
    if causal:
        off = Sk - Sq
        mask = torch.ones(Sq, Sk, dtype=torch.bool, device=q.device).tril(off)
        s = s.masked_fill(~mask, float("-inf"))
        if off < 0:
            # rows that see nothing: finite scores through the softmax (an
            # all -inf row is NaN, forward and backward), then P = 0
            hidden = ~mask.any(-1, keepdim=True)
            s = s.masked_fill(hidden, 0.0)
    p = torch.softmax(s, dim=-1)
    if hidden is not None:
        p = p.masked_fill(hidden, 0.0)
    return torch.matmul(p, vf).to(q.dtype)


def _wide(t):
    """fp32 working precision; fp64 inputs stay fp64 (truth for tests)."""
    return t if t.dtype is torch.float64 else t.float()


def _masked_scores(q, k, causal, scale):
    """Scaled scores [B,Hkv,G,Sq,Sk] (GQA group as its own axis), -inf where
    the causal mask (offset Sk - Sq) hides a key."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    qg = _wide(q).reshape(B, Hkv, Hq // Hkv, Sq, D)
    s = torch.matmul(qg, _wide(k).unsqueeze(2).transpose(-1, -2)) * scale
    if causal:
        mask = torch.ones(Sq, Sk, dtype=torch.bool,
                          device=q.device).tril(Sk - Sq)
        s = s.masked_fill(~mask, float("-inf"))
    return s


def attention_lse_ref(q, k, causal: bool = False,
                      scale: Optional[float] = None):
    """Log-sum-exp of the scaled, masked scores per query row: [B,Hq,Sq] in
    the working precision — what the forward kernel saves for the backward.
    A row that sees no key (causal with Sq > Sk) has -inf."""
    B, Hq, Sq, D = q.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    s = _masked_scores(q, k, causal, scale)
    return torch.logsumexp(s, dim=-1).reshape(B, Hq, Sq)


def attention_fwd_ref(q, k, v, causal: bool = False,
                      scale: Optional[float] = None,
                      emulate_bf16: bool = False):
    """Attention forward as csrc/attention_fwd32.hip computes it, and its
    specification: P = exp(s - rowmax), o = (P.V) / rowsum(P), lse = rowmax +
    log(rowsum(P)).  q [B,Hq,Sq,D], k/v [B,Hkv,Sk,D]; returns (o [B,Hq,Sq,D],
    lse [B,Hq,Sq]) in the working precision (fp64 for fp64 inputs).  A row
    that sees no key (causal with Sq > Sk) has o = 0 and lse = -inf.

    emulate_bf16=True rounds exactly where the kernel rounds: P to bf16
    before P.V, normalised by the unrounded row sum, and the output to bf16
    (returned widened).  The caller passes bf16-representable q/k/v for a
    faithful yardstick."""
    B, Hq, Sq, D = q.shape
    Hkv = k.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    wd = torch.float64 if q.dtype is torch.float64 else torch.float32

    def rnd(t):
        return t.to(torch.bfloat16).to(wd) if emulate_bf16 else t

    s = _masked_scores(q, k, causal, scale)  # [B,Hkv,G,Sq,Sk]
    m = s.amax(-1, keepdim=True)
    live = m > float("-inf")
    m = torch.where(live, m, torch.zeros_like(m))
    p = torch.exp(s - m)  # masked -> 0
    l = p.sum(-1, keepdim=True)
    lse = (m + torch.log(l)).reshape(B, Hq, Sq)
    o = torch.matmul(rnd(p), _wide(v).unsqueeze(2))
    o = torch.where(live, o / torch.where(live, l, torch.ones_like(l)),
                    torch.zeros_like(o))
    return rnd(o).reshape(B, Hq, Sq, D), lse


def attention_bwd_ref(q, k, v, o, lse, dout, causal: bool = False,
                      scale: Optional[float] = None,
                      emulate_bf16: bool = False):
    """Attention backward by recompute-from-LSE — the algorithm of
    csrc/attention_bwd.hip in torch, and its specification.

    q/o/dout [B,Hq,Sq,D], k/v [B,Hkv,Sk,D], lse [B,Hq,Sq].  P = exp(s*scale
    - lse), delta = rowsum(dout*o), dS = P o (dP - delta); dV = P^T.dO,
    dK = scale * dS^T.Q (both summed over the GQA group), dQ = scale * dS.K.
    Returns (dq, dk, dv) in the working precision (fp64 for fp64 inputs).

    emulate_bf16=True rounds exactly where the kernel rounds: P and dS to
    bf16 before their products, the outputs to bf16 (returned widened).  The
    caller passes bf16-representable q/k/v/o/dout for a faithful yardstick."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    G = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    wd = torch.float64 if q.dtype is torch.float64 else torch.float32

    def rnd(t):
        return t.to(torch.bfloat16).to(wd) if emulate_bf16 else t

    qg = _wide(q).reshape(B, Hkv, G, Sq, D)
    og = o.to(wd).reshape(B, Hkv, G, Sq, D)
    dog = dout.to(wd).reshape(B, Hkv, G, Sq, D)
    kg = _wide(k).unsqueeze(2)  # [B,Hkv,1,Sk,D]
    vg = _wide(v).unsqueeze(2)
    s = _masked_scores(q, k, causal, scale)
    p = torch.exp(s - lse.to(wd).reshape(B, Hkv, G, Sq, 1))  # masked -> 0
    delta = (dog * og).sum(-1, keepdim=True)
    dp = torch.matmul(dog, vg.transpose(-1, -2))
    ds = rnd(p * (dp - delta))
    p = rnd(p)
    dv = torch.matmul(p.transpose(-1, -2), dog).sum(2)
    dk = torch.matmul(ds.transpose(-1, -2), qg).sum(2) * scale
    dq = (torch.matmul(ds, kg) * scale).reshape(B, Hq, Sq, D)
    return rnd(dq), rnd(dk), rnd(dv)


def attention_bwd_bound_ref(q, k, v, o, lse, dout, causal: bool = False,
                            scale: Optional[float] = None):
    """The magnitudes a per-element error bound of a bf16 attention backward
    is made of, in fp64 (inputs as for attention_bwd_ref, any dtype):

      P       [B,Hq,Sq,Sk]  exp(s*scale - lse), 0 where masked
      E_q     [B,Hq,Sq]     sum_d |dO|*|O|: what delta = sum_d dO*O is made of
      dS_abs  [B,Hq,Sq,Sk]  |dS| + P*E_q, dS = P o (dP - delta): the size of
                            dS plus what one relative rounding of o moves it
                            by through delta
      A_dv    [B,Hkv,Sk,D]  P^T.|dO| summed over the GQA group
      A_dk    [B,Hkv,Sk,D]  |scale| * dS_abs^T.|Q| summed over the group
      A_dq    [B,Hq,Sq,D]   |scale| * dS_abs.|K|
      M       float         max over visible pairs of |s*scale| + |lse|: the
                            size of the exponential's argument before the
                            subtraction

    A_* are the absolute-value propagations of P and dS through the output
    products: an implementation that rounds P (dV) or dS (dQ, dK) and the
    output to bf16 errs by at most 2^-8 * (A + |truth|) from those two
    roundings if every one of them errs fully and in the worst direction."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    G = Hq // Hkv
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    q, k, v, o, dout = (t.double() for t in (q, k, v, o, dout))
    lse = lse.double().reshape(B, Hkv, G, Sq, 1)
    qg = q.reshape(B, Hkv, G, Sq, D)
    og = o.reshape(B, Hkv, G, Sq, D)
    dog = dout.reshape(B, Hkv, G, Sq, D)
    kg, vg = k.unsqueeze(2), v.unsqueeze(2)
    s = _masked_scores(q, k, causal, scale)  # [B,Hkv,G,Sq,Sk]
    seen = s > float("-inf")
    p = torch.exp(s - lse)  # masked -> 0
    arg = torch.where(seen, s.abs() + lse.abs(), torch.zeros_like(s))
    e_q = (dog.abs() * og.abs()).sum(-1, keepdim=True)
    delta = (dog * og).sum(-1, keepdim=True)
    ds = p * (torch.matmul(dog, vg.transpose(-1, -2)) - delta)
    ds_abs = ds.abs() + p * e_q
    a_dv = torch.matmul(p.transpose(-1, -2), dog.abs()).sum(2)
    a_dk = torch.matmul(ds_abs.transpose(-1, -2), qg.abs()).sum(2) * abs(scale)
    a_dq = (torch.matmul(ds_abs, kg.abs()) * abs(scale)).reshape(B, Hq, Sq, D)
    return dict(P=p.reshape(B, Hq, Sq, Sk), E_q=e_q.reshape(B, Hq, Sq),
                dS_abs=ds_abs.reshape(B, Hq, Sq, Sk), A_dv=a_dv, A_dk=a_dk,
                A_dq=a_dq, M=float(arg.max()))


def paged_decode_ref(q, k_cache, v_cache, block_table, seq_lens, block_size,
                     scale: Optional[float] = None):
    """q [B,Hq,D]; paged cache [nblocks,Hkv,block_size,D] (+table) or
    contiguous [B,Hkv,S,D] when block_table is None."""
    B, Hq, D = q.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    out = torch.empty_like(q)
    for b in range(B):
        S = int(seq_lens[b])
        if block_table is None:
            kb = k_cache[b, :, :S]  # [Hkv,S,D]
            vb = v_cache[b, :, :S]
        else:
            nblk = (S + block_size - 1) // block_size
            ks, vs = [], []
            for i in range(nblk):
                blk = int(block_table[b, i])
                ks.append(k_cache[blk])  # [Hkv, block_size, D]
                vs.append(v_cache[blk])
            kb = torch.cat(ks, dim=1)[:, :S]
            vb = torch.cat(vs, dim=1)[:, :S]
        for h in range(Hq):
            hk = h // G
            s = (kb[hk].float() @ q[b, h].float()) * scale  # [S]
            p = torch.softmax(s, dim=-1)
            out[b, h] = (p @ vb[hk].float()).to(q.dtype)
    return out


def paged_prefill_ref(q, k_cache, v_cache, block_table, cu_q, seq_lens,
                      block_size, scale: Optional[float] = None):
    """Causal attention of a ragged batch of NEW tokens over a paged cache
    that already holds their K/V — the specification of
    csrc/attention_prefill_paged.hip.

    q [T,Hq,D]: rows cu_q[b]..cu_q[b+1] (n_b of them) are sequence b's new
    tokens.  Cache [nblocks,Hkv,block_size,D], block_table [B,max_blocks],
    seq_lens[b] = S_b the cached length INCLUDING the new tokens: query i of
    sequence b sits at position S_b - n_b + i and sees kv positions <= that.
    Rows at a negative position (S_b < n_b) see nothing and return zeros.
    Works in fp32, or fp64 for fp64 inputs; returns q's dtype."""
    T, Hq, D = q.shape
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    out = torch.zeros_like(q)
    for b in range(seq_lens.shape[0]):
        lo, hi, S = int(cu_q[b]), int(cu_q[b + 1]), int(seq_lens[b])
        n = hi - lo
        if n == 0 or S <= 0:
            continue
        blks = block_table[b, :(S + block_size - 1) // block_size].long()
        # [Hkv, S, D]: the sequence's rows gathered through its table
        kb = _wide(k_cache[blks]).transpose(0, 1).reshape(Hkv, -1, D)[:, :S]
        vb = _wide(v_cache[blks]).transpose(0, 1).reshape(Hkv, -1, D)[:, :S]
        qb = _wide(q[lo:hi]).transpose(0, 1).reshape(Hkv, G, n, D)
        s = torch.matmul(qb, kb.unsqueeze(1).transpose(-1, -2)) * scale
        pos = torch.arange(S - n, S, device=q.device)  # position of query i
        seen = torch.arange(S, device=q.device)[None, :] <= pos[:, None]
        p = torch.softmax(s.masked_fill(~seen, float("-inf")), dim=-1)
        p = p.masked_fill(~seen, 0.0)  # also clears the NaN of all-masked rows
        o = torch.matmul(p, vb.unsqueeze(1)).reshape(Hq, n, D)
        out[lo:hi] = o.transpose(0, 1).to(q.dtype)
    return out


def groupnorm_silu_ref(x, gamma, beta, groups, eps=1e-5, do_silu=True):
    y = torch.nn.functional.group_norm(
        x.float(), groups, gamma.float(), beta.float(), eps
    )
    if do_silu:
        y = torch.nn.functional.silu(y)
    return y.to(x.dtype)


def layernorm_ref(x, gamma, beta, eps=1e-5):
    return torch.nn.functional.layer_norm(
        x.float(), (x.shape[-1],), gamma.float(), beta.float(), eps
    ).to(x.dtype)


def rmsnorm_ref(x, gamma, eps=1e-6):
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * rstd * gamma.float()).to(x.dtype)


def cfg_euler_ref(x_t, eps_c, eps_u, guidance, dsigma):
    e = eps_c.float()
    if eps_u is not None:
        e = eps_u.float() + guidance * (eps_c.float() - eps_u.float())
    return (x_t.float() + dsigma * e).to(x_t.dtype)


def silu_mul_ref(a, b):
    return (torch.nn.functional.silu(a.float()) * b.float()).to(a.dtype)


def geglu_ref(a, b):
    return (torch.nn.functional.gelu(a.float(), approximate="tanh") * b.float()).to(a.dtype)


def rope_ref(x, cos, sin, positions=None):
    """x [B,H,S,D]; cos/sin [S_max, D/2] f32; rotate-half convention."""
    B, H, S, D = x.shape
    idx = positions if positions is not None else torch.arange(S, device=x.device)
    c = cos[idx].view(1, 1, S, D // 2).float()
    s = sin[idx].view(1, 1, S, D // 2).float()
    x1 = x[..., : D // 2].float()
    x2 = x[..., D // 2:].float()
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    return out.to(x.dtype)


def adamw_ref(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    pf, gf = p.float(), g.float()
    m.mul_(beta1).add_(gf, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gf, gf, value=1 - beta2)
    mhat = m / (1 - beta1**step)
    vhat = v / (1 - beta2**step)
    pf = pf - lr * (mhat / (vhat.sqrt() + eps) + wd * pf)
    p.copy_(pf.to(p.dtype))
    return p


# ------------------------------------------------ per-row filtered sampling
# float64 models of sampling_cutoff / sample_batch (csrc/sampling.hip).  The
# kept set of a row is {i : logit_i >= cutoff}; ties at a threshold are all
# kept.  The uniform draws use the kernel's own integer hash, so a CPU engine
# is deterministic and agrees with the GPU except at near-ties.

_M32 = 0xFFFFFFFF


def _hash3(a, b, c):
    """The kernel's hash3 on uint32 values held in int64 tensors (products
    wrap mod 2^64, which leaves their low 32 bits exact)."""
    h = (a * 0x9E3779B1 ^ b * 0x85EBCA77 ^ c * 0xC2B2AE3D) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x2C1B3C6D) & _M32
    h = h ^ (h >> 12)
    h = (h * 0x297A2D39) & _M32
    return h ^ (h >> 15)


def sampling_cutoff_ref(logits, temperature, top_k, top_p, min_p):
    """Cutoff logit per row, float32 [B].  Parameters are [B] tensors:
    temperature/top_p/min_p float32, top_k integer.  top_k 0 or >= V, top_p
    >= 1 and min_p <= 0 are off; a row with every filter off, or with
    temperature <= 0, gets -inf.  A -inf logit is never kept by a filter."""
    x = logits.detach().double()
    B, V = x.shape
    ninf = float("-inf")
    T = temperature.double()
    live = T > 0
    T = torch.where(live, T, torch.ones_like(T))
    k = top_k.long()
    p = top_p.double()
    q = min_p.double()
    xs = x.sort(-1, descending=True).values
    finite = xs > ninf
    nfin = finite.sum(-1)
    k_on, p_on, q_on = (k > 0) & (k < V), p < 1, q > 0
    # top-k: the k-th largest finite logit (pure ordering)
    kth = (torch.minimum(k, nfin) - 1).clamp_(min=0)
    c_k = torch.where(k_on, xs.gather(1, kth[:, None])[:, 0],
                      torch.full_like(T, ninf))
    in_k = finite & (xs >= c_k[:, None])
    # top-p over the survivors: keep i iff the mass strictly above it is
    # <= p * Z_K; equal logits share the mass above their group
    s = xs / T[:, None]
    e_all = torch.exp(s - s[:, :1])
    e_all = torch.where(finite, e_all, torch.zeros_like(e_all))
    e = torch.where(in_k, e_all, torch.zeros_like(e_all))
    before = e.cumsum(-1) - e
    pos = torch.arange(V).expand(B, V)
    start = torch.ones(B, V, dtype=torch.bool)
    start[:, 1:] = xs[:, 1:] != xs[:, :-1]
    gstart = torch.where(start, pos, torch.zeros_like(pos)).cummax(-1).values
    above = before.gather(1, gstart)
    keep_p = in_k & (above <= (p * e.sum(-1))[:, None])
    pinf = torch.full_like(xs, float("inf"))
    c_p = torch.where(keep_p, xs, pinf).min(-1).values
    # min-p: p_i >= q * p_max
    c_q = torch.where(finite & (e_all >= q[:, None]), xs, pinf).min(-1).values
    c = c_k
    c = torch.where(p_on, torch.maximum(c, c_p), c)
    c = torch.where(q_on, torch.maximum(c, c_q), c)
    c = torch.where(live & (k_on | p_on | q_on), c, torch.full_like(c, ninf))
    return c.float()


def gumbel_scores_ref(logits, temperature, seeds, counters):
    """float64 scores logit * f32(1/T) + G(seed, counter, i), [B, V]; the
    uniform behind G is formed in float32 exactly as the kernel forms it."""
    B, V = logits.shape
    seeds, counters = seeds.long(), counters.long()
    lo = (seeds & _M32)[:, None]
    hi = (((seeds >> 32) & _M32) ^ (counters & _M32))[:, None]
    u = _hash3(lo, hi, torch.arange(V, dtype=torch.long)[None, :])
    uf = (u >> 8).float() * (1.0 / 16777216.0) + 1e-10
    gumbel = -torch.log(-torch.log(uf.double()))
    inv_t = (1.0 / temperature.float()).double()
    return logits.detach().double() * inv_t[:, None] + gumbel


def sample_batch_ref(logits, temperature, top_k, top_p, min_p, seeds, counters):
    """Token per row, int32 [B]: arg-max of the gumbel scores over the kept
    set, first index on ties; temperature <= 0 is the plain arg-max."""
    lg = logits.detach().float()
    temperature = temperature.float()
    live = temperature > 0
    cut = sampling_cutoff_ref(lg, temperature, top_k, top_p, min_p)
    safe_t = torch.where(live, temperature, torch.ones_like(temperature))
    scores = gumbel_scores_ref(lg, safe_t, seeds, counters)
    scores = scores.masked_fill(~(lg >= cut[:, None]), float("-inf"))
    return torch.where(live, scores.argmax(-1), lg.argmax(-1)).int()


def moe_route_ref(logits, top_k: int):
    """Top-k routing: (weights [N,k], idx int32 [N,k]).  A STABLE descending
    sort defines the order — descending logit, ties to the lower expert
    index; weights are the softmax over the k selected logits, in the
    logits' working precision (gradients flow to them)."""
    vals, order = torch.sort(_wide(logits), dim=-1, descending=True,
                             stable=True)
    return (torch.softmax(vals[:, :top_k], dim=-1),
            order[:, :top_k].to(torch.int32))


def moe_ffn_ref(x, gate_up, down, weights, idx):
    """Routed SwiGLU FFN: out[t] = sum_j weights[t,j] * FFN_{idx[t,j]}(x[t])
    with FFN_e(v) = (silu(v @ gate_e^T) * (v @ up_e^T)) @ down_e^T, where
    gate_e / up_e are the two halves of gate_up[e] [2F, d] and down[e] is
    [d, F].  Working-precision math with no data-dependent control flow:
    every expert runs on every token and the routing enters as a dense
    [N, E] coefficient matrix, so it is differentiable in x, the weights
    and the routing weights, and costs E/k times the routed FLOPs.  Returns
    [N, d] in x's dtype."""
    E, F = gate_up.shape[0], down.shape[2]
    xw, ww = _wide(x), _wide(weights).to(_wide(x).dtype)
    coef = torch.zeros(x.shape[0], E, dtype=xw.dtype, device=x.device)
    coef = coef.scatter_add(1, idx.long(), ww)
    out = torch.zeros_like(xw)
    for e in range(E):
        gu = xw @ _wide(gate_up[e]).T
        h = torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]
        out = out + coef[:, e:e + 1] * (h @ _wide(down[e]).T)
    return out.to(x.dtype)


def moe_ffn_bound_ref(x, gate_up, down, weights, idx, bf16_points=False):
    """(want, tol) in fp64 for a bf16 implementation of moe_ffn_ref that
    rounds to bf16 exactly twice, at h = silu(gate) * up and at the output.

      want      moe_ffn_ref in fp64 on the inputs as given
      A[t, c]   sum_j w[t,j] * sum_f |h_e[t,f]| * |down_e[c,f]|, e = idx[t,j]:
                the absolute-value propagation of h through the down
                projection
      tol       2 * 2^-9 * (A + |want|)

    Rounding to bf16 (8 significant bits) moves a value by at most 2^-8 of
    itself and by 2^-9 or less for most of a binade.  2^-8 * A is therefore
    what rounding every h can move an output by if all of them err fully
    and in the worst direction, and 2^-8 * |want| what rounding the output
    can: tol is the worst case of the two roundings, which independent
    roundings over ffn_dim terms stay far below.  That slack is what covers
    fp32 accumulation (about K * 2^-24 of A) and a fast exponential.

    bf16_points=True rounds h and the output to bf16 inside the same fp64
    pipeline and returns that output in place of `want`: the yardstick that
    shows how much of tol a correct implementation uses."""
    E, F = gate_up.shape[0], down.shape[2]
    xw, ww = x.double(), weights.double()
    coef = torch.zeros(x.shape[0], E, dtype=torch.float64)
    coef = coef.scatter_add(1, idx.long(), ww)
    out, A = torch.zeros_like(xw), torch.zeros_like(xw)
    for e in range(E):
        gu = xw @ gate_up[e].double().T
        h = torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]
        if bf16_points:
            h = h.to(torch.bfloat16).double()
        de = down[e].double()
        out = out + coef[:, e:e + 1] * (h @ de.T)
        A = A + coef[:, e:e + 1].abs() * (h.abs() @ de.abs().T)
    tol = 2.0 * 2.0 ** -9 * (A + out.abs())
    if bf16_points:
        out = out.to(torch.bfloat16).double()
    return out, tol


# ---- int4 weight-only linear.  Format (csrc/linear_w4.hip): weights are
# quantized symmetrically in groups of 128 along K; qweight int32 [N, K/8]
# holds k = 8w..8w+7 in word w as unsigned nibbles u = q + 8, k offset j at
# nibble position j/2 (j even) or 4 + j/2 (j odd); scales bf16 [N, K/128].

W4_GROUP = 128


def _w4_shifts(device, dtype):
    """Bit offset of k offset j inside a packed word, [8]: nibble j/2 for
    even j, 4 + j/2 for odd j.  Built by device ops only (no host tensor),
    so unpacking can run inside a graph capture."""
    j = torch.arange(8, device=device, dtype=dtype)
    return ((j >> 1) + ((j & 1) << 2)) << 2


def w4_pack(q):
    """q integer [N, K] with values in [-8, 7] -> int32 [N, K/8]."""
    N, K = q.shape
    u = (q.to(torch.int64) + 8).view(N, K // 8, 8)
    shifts = _w4_shifts(q.device, torch.int64)
    word = (u << shifts).sum(-1)
    word = torch.where(word >= 1 << 31, word - (1 << 32), word)
    return word.to(torch.int32)


def w4_unpack(qweight):
    """int32 [N, K/8] (or its uint8 view [N, K/2]) -> q int32 [N, K] with
    values in [-8, 7]; the exact inverse of w4_pack."""
    if qweight.dtype is torch.uint8:
        qweight = qweight.view(torch.int32)
    shifts = _w4_shifts(qweight.device, torch.int32)
    u = (qweight.unsqueeze(-1) >> shifts) & 0xF
    return (u - 8).view(qweight.shape[0], -1)


def quantize_w4_ref(weight):
    """weight [N, K] -> (qweight int32 [N, K/8], scales bf16 [N, K/128]).
    scale = bf16(absmax(group) / 7), 1 where that is zero (an all-zero
    group); q = clamp(round_half_even(w / scale), -8, 7) with the quotient
    taken in fp64, so a tie is a tie of the real quotient."""
    N, K = weight.shape
    g = weight.detach().double().view(N, K // W4_GROUP, W4_GROUP)
    scales = (g.abs().amax(-1).float() / 7.0).to(torch.bfloat16)
    scales = torch.where(scales == 0, torch.ones_like(scales), scales)
    q = torch.round(g / scales.double().unsqueeze(-1)).clamp_(-8, 7)
    return w4_pack(q.view(N, K)), scales


def dequantize_w4_ref(qweight, scales):
    """w_hat fp32 [N, K] = float(scale[n, k // 128]) * q[n, k], exact: a
    bf16 times a 4-bit integer fits in fp32."""
    q = w4_unpack(qweight)
    N, K = q.shape
    w = q.view(N, K // W4_GROUP, W4_GROUP).float() \
        * scales.float().unsqueeze(-1)
    return w.view(N, K)


def linear_w4_ref(x, qweight, scales):
    """x [..., K] . w_hat^T with w_hat cast to x's dtype (exact for fp32 and
    wider; one rounding per weight for bf16).  Differentiable in x."""
    w = dequantize_w4_ref(qweight, scales).to(x.dtype)
    return torch.nn.functional.linear(x, w)


def linear_w4_bound_ref(x, qweight, scales, bf16_points=False):
    """(want, tol) in fp64 for an implementation of x [M, K] . w_hat^T that
    keeps w_hat exact, accumulates in fp32 and rounds the output to bf16.

      want   x . w_hat^T
      A      |x| . |w_hat|^T
      tol    2^-7 * |want| + 2^-10 * A

    Rounding the output to bf16 moves it by at most 2^-8 * |want|; the first
    term is twice that.  Worst-case fp32 accumulation is about K * 2^-24 * A,
    at most 2^-10 * A up to K = 16384; the second term is also half of what
    rounding every dequantized weight to bf16 in the worst direction could
    do (2^-9 * A).

    bf16_points=True returns the same fp64 product with the output rounded
    to bf16 in place of `want`: the yardstick that shows how much of tol a
    correct implementation uses."""
    xw = x.detach().double().cpu()
    w = dequantize_w4_ref(qweight.cpu(), scales.cpu()).double()
    want = xw @ w.T
    A = xw.abs() @ w.abs().T
    tol = 2.0 ** -7 * want.abs() + 2.0 ** -10 * A
    if bf16_points:
        want = want.to(torch.bfloat16).double()
    return want, tol
