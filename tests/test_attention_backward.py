"""CPU tier for the attention backward: the torch reference of the
recompute-from-LSE algorithm (the HIP kernel's specification and the
yardstick for its tolerance) against autograd, and the unchanged CPU
dispatch of F.attention in grad mode."""
import math

import pytest
import torch

from modal_examples_amd.ops import functional as F
from modal_examples_amd.ops import reference as ref

# (B, Hq, Hkv, Sq, Sk, D, causal)
CASES = [
    (2, 4, 4, 40, 40, 16, False),
    (2, 4, 4, 40, 40, 16, True),
    (1, 4, 2, 33, 33, 32, True),    # GQA
    (1, 4, 2, 17, 50, 16, False),   # Sq != Sk
    (1, 4, 2, 17, 50, 16, True),    # causal, Sk > Sq
    (1, 2, 1, 50, 9, 16, False),
]


def _inputs(B, Hq, Hkv, Sq, Sk, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).double()
    return mk(B, Hq, Sq, D), mk(B, Hkv, Sk, D), mk(B, Hkv, Sk, D), \
        mk(B, Hq, Sq, D)


def _autograd64(q, k, v, dout, causal, scale):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = ref.attention_ref(q, k, v, causal, scale)
    assert o.dtype is torch.float64
    o.backward(dout)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("case", CASES, ids=str)
def test_bwd_ref_fp64_matches_autograd(case):
    B, Hq, Hkv, Sq, Sk, D, causal = case
    q, k, v, dout = _inputs(B, Hq, Hkv, Sq, Sk, D)
    scale = 1.0 / math.sqrt(D)
    o, gq, gk, gv = _autograd64(q, k, v, dout, causal, scale)
    lse = ref.attention_lse_ref(q, k, causal, scale)
    assert lse.shape == (B, Hq, Sq) and lse.dtype is torch.float64

    # lse == logsumexp of the scaled masked scores, built independently here
    rep = Hq // Hkv
    s = torch.matmul(q, k.repeat_interleave(rep, 1).transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(~torch.ones(Sq, Sk, dtype=torch.bool).tril(Sk - Sq),
                          float("-inf"))
    assert (lse - torch.logsumexp(s, -1)).abs().max() <= 1e-9

    dq, dk, dv = ref.attention_bwd_ref(q, k, v, o, lse, dout, causal, scale)
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    for got, want in ((dq, gq), (dk, gk), (dv, gv)):
        assert got.dtype is torch.float64
        assert (got - want).abs().max() <= 1e-9


@pytest.mark.parametrize("case", CASES, ids=str)
def test_bwd_ref_bf16_emulation_is_a_sane_yardstick(case):
    B, Hq, Hkv, Sq, Sk, D, causal = case
    q, k, v, dout = _inputs(B, Hq, Hkv, Sq, Sk, D, seed=1)
    scale = 1.0 / math.sqrt(D)
    o = ref.attention_ref(q, k, v, causal, scale)
    lse = ref.attention_lse_ref(q, k, causal, scale)
    truth = ref.attention_bwd_ref(q, k, v, o, lse, dout, causal, scale)
    emu = ref.attention_bwd_ref(q, k, v, o.to(torch.bfloat16).double(),
                                lse.float(), dout, causal, scale,
                                emulate_bf16=True)
    for got, want in zip(emu, truth):
        assert torch.isfinite(got).all()
        err = (got - want).abs().max().item()
        assert 0.0 < err < 0.05 * want.abs().max().item()


def test_bwd_ref_default_scale_and_fp32():
    q, k, v, dout = (t.float() for t in _inputs(1, 2, 2, 12, 12, 16, seed=2))
    o = ref.attention_ref(q, k, v, True)
    lse = ref.attention_lse_ref(q, k, True)
    dq, dk, dv = ref.attention_bwd_ref(q, k, v, o, lse, dout, True)
    assert dq.dtype is torch.float32
    _, gq, gk, gv = _autograd64(q.double(), k.double(), v.double(),
                                dout.double(), True, 1.0 / math.sqrt(16))
    for got, want in ((dq, gq), (dk, gk), (dv, gv)):
        assert (got.double() - want).abs().max() <= 1e-4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_cpu_grad_mode_keeps_reference_path(dtype):
    torch.manual_seed(3)
    q = torch.randn(1, 4, 20, 64).to(dtype).requires_grad_(True)
    k = torch.randn(1, 2, 24, 64).to(dtype).requires_grad_(True)
    v = torch.randn(1, 2, 24, 64).to(dtype).requires_grad_(True)
    o = F.attention(q, k, v, causal=True)
    assert torch.equal(o, ref.attention_ref(q, k, v, True, 1.0 / 8.0))
    o.float().square().sum().backward()
    for t in (q, k, v):
        assert t.grad is not None and torch.isfinite(t.grad).all()
        assert float(t.grad.abs().sum()) > 0


def test_cpu_attention_qkv_grad_reaches_fused_leaf():
    torch.manual_seed(4)
    qkv = torch.randn(2, 10, 3, 2, 64).to(torch.bfloat16).requires_grad_(True)
    o = F.attention_qkv(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    assert o.shape == (2, 10, 128)
    o.float().sum().backward()
    assert qkv.grad.shape == qkv.shape
    assert all(float(qkv.grad[:, :, i].abs().sum()) > 0 for i in range(3))
