"""GPU tier for the HIP attention backward (csrc/attention_bwd.hip).

Tolerance rule for every gradient check: with g64 the fp64 truth from
reference.attention_bwd_ref on the bf16-rounded inputs and e_y the max error
of the bf16-emulating yardstick (same function, emulate_bf16=True) against
g64, the kernel must satisfy

    max|kernel - g64| <= 2 * e_y + 2**-8 * max|g64|

(2 = margin for another summation order and __expf; the additive term is
one bf16 ulp at the top of the range), with no NaN or Inf.  Each check prints
its measured max|kernel - g64| / e_y (run with -s to see them).

With a single key (Sq=130, Sk=1) the true dq and dk are exactly zero and so
is the bound: the kernel meets it because its delta is summed by the same
MFMA chain as dP, so dS = P o (dP - delta) cancels exactly.
"""
import functools
import math

import pytest
import torch

import modal_examples_amd.ops.functional as F
import modal_examples_amd.ops.reference as ref

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

BF = torch.bfloat16


@functools.lru_cache(maxsize=None)
def _case(B, Hq, Hkv, Sq, Sk, D, causal, qmul=1.0, seed=0):
    """Fixed-seed bf16 inputs (on the CPU) with the fp64 truth and the
    yardstick's error, computed once per shape and never modified."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(B, Hq, Sq, D, generator=g) * qmul).to(BF)
    k = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    dout = torch.randn(B, Hq, Sq, D, generator=g).to(BF)  # independent of o
    scale = 1.0 / math.sqrt(D)
    q64, k64, v64, d64 = q.double(), k.double(), v.double(), dout.double()
    o64 = ref.attention_ref(q64, k64, v64, causal, scale)
    lse64 = ref.attention_lse_ref(q64, k64, causal, scale)
    g64 = ref.attention_bwd_ref(q64, k64, v64, o64, lse64, d64, causal, scale)
    yard = ref.attention_bwd_ref(q64, k64, v64, o64.to(BF).double(),
                                 lse64.float(), d64, causal, scale,
                                 emulate_bf16=True)
    e_y = tuple((y - t).abs().max().item() for y, t in zip(yard, g64))
    return dict(q=q, k=k, v=v, dout=dout, scale=scale, causal=causal,
                lse64=lse64, g64=g64, e_y=e_y)


def _check_grads(c, grads, label):
    for name, got, want, e_y in zip(("dq", "dk", "dv"), grads, c["g64"],
                                    c["e_y"]):
        got = got.detach().cpu().double()
        assert got.shape == want.shape, f"{label} {name}: shape {got.shape}"
        assert torch.isfinite(got).all(), f"{label} {name}: NaN/Inf"
        err = (got - want).abs().max().item()
        top = want.abs().max().item()
        ratio = err / e_y if e_y > 0 else (0.0 if err == 0 else math.inf)
        print(f"ATTN_BWD_RATIO {label} {name} err={err:.4e} e_y={e_y:.4e} "
              f"ratio={ratio:.3f} max|g64|={top:.4e}")
        assert err <= 2.0 * e_y + 2.0 ** -8 * top, (
            f"{label} {name}: max err {err:.4e} > 2*{e_y:.4e} + 2^-8*{top:.4e}")


def _run_attention(c):
    """fwd+bwd through F.attention on the GPU; returns (o, dq, dk, dv)."""
    q, k, v = (c[n].cuda().requires_grad_(True) for n in "qkv")
    o = F.attention(q, k, v, causal=c["causal"])
    assert type(o.grad_fn).__name__ == "_AttentionFnBackward"
    o.backward(c["dout"].cuda())
    return o.detach(), q.grad, k.grad, v.grad


GQA = (2, 8, 2, 160, 160, 128, True)


@requires_gpu
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_bwd_tiles_and_diagonal(D, causal):
    c = _case(2, 4, 4, 256, 256, D, causal)
    _check_grads(c, _run_attention(c)[1:], f"tiles D{D} causal={causal}")


@requires_gpu
@pytest.mark.parametrize("Sq,Sk,causal", [
    (200, 77, False), (77, 200, True), (129, 129, True), (1, 33, True),
    (130, 1, False)])
@pytest.mark.parametrize("D", [64, 128])
def test_bwd_tails(D, Sq, Sk, causal):
    c = _case(2, 2, 2, Sq, Sk, D, causal)
    _check_grads(c, _run_attention(c)[1:],
                 f"tails D{D} Sq{Sq} Sk{Sk} causal={causal}")


@requires_gpu
def test_bwd_gqa_sums_over_group():
    c = _case(*GQA)
    _check_grads(c, _run_attention(c)[1:], "gqa Hq8 Hkv2 D128 S160 causal")


@requires_gpu
def test_bwd_saturated_scores():
    c = _case(2, 4, 4, 256, 256, 64, True, qmul=8.0)
    _check_grads(c, _run_attention(c)[1:], "saturated D64 S256 causal q*8")


@requires_gpu
@pytest.mark.parametrize("D", [64, 128])
def test_bwd_fused_qkv_strides(D):
    B, S, H = 2, 150, 4
    c = _case(B, H, H, S, S, D, True, seed=5)
    fused = torch.stack([c[n].transpose(1, 2) for n in "qkv"], dim=2)
    fused = fused.contiguous().cuda().requires_grad_(True)  # [B,S,3,H,D] leaf
    assert fused.shape == (B, S, 3, H, D)
    qs, ks, vs = fused[:, :, 0], fused[:, :, 1], fused[:, :, 2]
    o = F.attention_qkv(qs, ks, vs, causal=True)
    assert o.shape == (B, S, H * D) and o.is_contiguous()
    with torch.no_grad():
        o_ng = F.attention_qkv(qs, ks, vs, causal=True)
    assert torch.equal(o.detach(), o_ng)
    # the gradient arrives as [B,S,H*D]; dout is [B,H,S,D]-logical
    o.backward(c["dout"].transpose(1, 2).reshape(B, S, H * D).cuda())
    grads = [fused.grad[:, :, i].transpose(1, 2) for i in range(3)]
    _check_grads(c, grads, f"fused-qkv D{D} S{S} causal")


@requires_gpu
@pytest.mark.parametrize("case", [
    (2, 4, 4, 256, 256, 64, True), (2, 2, 2, 200, 77, 128, False), GQA],
    ids=str)
def test_fwd_lse(case):
    from modal_examples_amd.ops._build import get_ext

    ext = get_ext(required=True)
    c = _case(*case)
    q, k, v = (c[n].cuda() for n in "qkv")
    o, lse = ext.attention_fwd_lse(q, k, v, c["causal"], c["scale"])
    assert lse.dtype is torch.float32 and lse.shape == c["lse64"].shape
    err = (lse.cpu().double() - c["lse64"]).abs().max().item()
    print(f"ATTN_LSE_ERR {case} {err:.3e}")
    assert err <= 1e-3
    assert torch.equal(o, ext.attention(q, k, v, c["causal"], c["scale"]))
    o2, lse2 = ext.attention_fwd_lse_bshd(q, k, v, c["causal"], c["scale"])
    assert torch.equal(o2.transpose(1, 2), o) and torch.equal(lse2, lse)


@requires_gpu
def test_bwd_bitwise_reproducible():
    c = _case(*GQA)
    a = _run_attention(c)
    b = _run_attention(c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@requires_gpu
@pytest.mark.parametrize("Sq,Sk,causal", [(200, 77, False), (129, 129, True)])
def test_bwd_no_stray_writes(Sq, Sk, causal):
    from modal_examples_amd.gpu.guard import GuardBand
    from modal_examples_amd.ops._build import get_ext

    ext = get_ext(required=True)
    c = _case(2, 2, 2, Sq, Sk, 64, causal)
    q, k, v, dout = (c[n].cuda() for n in ("q", "k", "v", "dout"))
    o, lse = ext.attention_fwd_lse(q, k, v, causal, c["scale"])
    bands = [GuardBand(t.shape, BF, "cuda") for t in (q, k, v)]
    ext.attention_bwd(q, k, v, o, lse, dout, *(b.tensor for b in bands),
                      causal, c["scale"])
    torch.cuda.synchronize()
    for b in bands:
        b.check()
    _check_grads(c, [b.tensor for b in bands],
                 f"guarded D64 Sq{Sq} Sk{Sk} causal={causal}")


def _fwd_bwd_peak_growth():
    B, H, S, D = 1, 8, 4096, 64
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, H, S, D, generator=g).to(BF).cuda()
               .requires_grad_(True) for _ in range(3))
    dout = torch.randn(B, H, S, D, generator=g).to(BF).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    F.attention(q, k, v).backward(dout)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v))
    return torch.cuda.max_memory_allocated() - base


@requires_gpu
def test_bwd_memory_is_linear_in_sequence(monkeypatch):
    """B1 H8 S4096 D64 fwd+bwd: o, lse, dO, dq, dk, dv and delta are about
    25 MB; the reference path's fp32 scores alone are 512 MB."""
    MB = 1 << 20
    monkeypatch.delenv("MODAL_AMD_ATTN_BWD", raising=False)
    grown = _fwd_bwd_peak_growth()
    print(f"ATTN_BWD_MEM kernel path {grown / MB:.1f} MB")
    assert grown < 128 * MB
    monkeypatch.setenv("MODAL_AMD_ATTN_BWD", "ref")
    grown_ref = _fwd_bwd_peak_growth()
    print(f"ATTN_BWD_MEM reference path {grown_ref / MB:.1f} MB")
    assert grown_ref > 512 * MB


@requires_gpu
@pytest.mark.parametrize("D,dtype,Sq,Sk,causal", [
    (32, BF, 40, 40, False), (64, torch.float32, 40, 40, True),
    (64, BF, 48, 40, True)])
def test_grad_mode_fallbacks_use_reference(D, dtype, Sq, Sk, causal):
    torch.manual_seed(1)
    q = torch.randn(1, 2, Sq, D, device="cuda", dtype=dtype, requires_grad=True)
    k = torch.randn(1, 2, Sk, D, device="cuda", dtype=dtype, requires_grad=True)
    v = torch.randn(1, 2, Sk, D, device="cuda", dtype=dtype, requires_grad=True)
    o = F.attention(q, k, v, causal=causal)
    assert type(o.grad_fn).__name__ != "_AttentionFnBackward"
    o.float().sum().backward()
    for t in (q, k, v):
        assert t.grad is not None and t.grad.shape == t.shape


@requires_gpu
def test_raw_bwd_rejects_bad_arguments():
    from modal_examples_amd.ops._build import get_ext

    ext = get_ext(required=True)
    c = _case(2, 2, 2, 129, 129, 64, True)
    q, k, v, dout = (c[n].cuda() for n in ("q", "k", "v", "dout"))
    o, lse = ext.attention_fwd_lse(q, k, v, True, c["scale"])
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    args = lambda **kw: [kw.get(n, x) for n, x in (
        ("q", q), ("k", k), ("v", v), ("o", o), ("lse", lse), ("dout", dout),
        ("dq", dq), ("dk", dk), ("dv", dv))] + [kw.get("causal", True),
                                                 c["scale"]]
    with pytest.raises(RuntimeError, match="lse"):
        ext.attention_bwd(*args(lse=lse[:, :, :-1].contiguous()))
    with pytest.raises(RuntimeError, match="bf16"):
        ext.attention_bwd(*args(dout=dout.to(torch.float16)))
    with pytest.raises(RuntimeError, match="Sk >= Sq"):
        ext.attention_bwd(*args(k=k[:, :, :100].contiguous(),
                                v=v[:, :, :100].contiguous(),
                                dk=dk[:, :, :100].contiguous(),
                                dv=dv[:, :, :100].contiguous()))
    with pytest.raises(RuntimeError, match="shape"):
        ext.attention_bwd(*args(dq=dq[:, :, :-1].contiguous()))
    torch.cuda.synchronize()
