"""Numerics: every gfx950 HIP kernel vs its plain-PyTorch fp32 reference.

Run on a real MI355X via:  gpurun -- 'python -m pytest tests -m gpu -x -q'
Tolerances reflect bf16 I/O with f32 accumulation.

The test_attention_* functions here are the loose tier for the attention
forward.  The strict tier — bitwise selector cases, an fp64 truth with a
bf16-emulating yardstick on every element, masks, GQA mapping, stray writes,
hidden rows, empty inputs and the no-defer instantiations — is
test_attention_forward.py (CPU: builders, judge, mutants) and
test_attention_forward_gpu.py.
"""
import math

import pytest
import torch

import modal_examples_amd.ops.functional as F
import modal_examples_amd.ops.reference as ref

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def _close(a, b, atol=2e-2, rtol=2e-2, frac=0.999):
    """bf16 comparison: allow a tiny fraction of stragglers (rounding at tile
    boundaries) but require the bulk to match tightly."""
    a, b = a.float(), b.float()
    ok = (a - b).abs() <= (atol + rtol * b.abs())
    good = ok.float().mean().item()
    assert good >= frac, f"only {good:.5f} of elements within tol; max err {(a-b).abs().max().item():.4f}"


@requires_gpu
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_attention_self(D, causal):
    torch.manual_seed(0)
    B, H, S = 2, 4, 512
    q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    out = F.attention(q, k, v, causal=causal)
    exp = ref.attention_ref(q, k, v, causal=causal)
    _close(out, exp)


@requires_gpu
def test_attention_asymmetric_detects_transpose():
    """Asymmetric low-rank inputs catch silent output transposes (guide G9)."""
    torch.manual_seed(1)
    B, H, S, D = 1, 2, 256, 64
    q = torch.zeros(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    q[..., 0] = torch.linspace(-2, 2, S, device="cuda").to(torch.bfloat16)
    k = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    _close(F.attention(q, k, v), ref.attention_ref(q, k, v))


@requires_gpu
def test_attention_cross_short_kv():
    """SDXL cross-attention: Sk=77 text tokens (non multiple of 32)."""
    torch.manual_seed(2)
    q = torch.randn(2, 10, 1024, 64, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(2, 10, 77, 64, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(2, 10, 77, 64, device="cuda", dtype=torch.bfloat16)
    _close(F.attention(q, k, v), ref.attention_ref(q, k, v))


@requires_gpu
def test_attention_gqa_causal():
    """Llama-3 shape: 32 q heads, 8 kv heads, D=128."""
    torch.manual_seed(3)
    q = torch.randn(1, 32, 384, 128, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(1, 8, 384, 128, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(1, 8, 384, 128, device="cuda", dtype=torch.bfloat16)
    _close(F.attention(q, k, v, causal=True), ref.attention_ref(q, k, v, causal=True))


@requires_gpu
def test_attention_ragged_seq():
    torch.manual_seed(4)
    q = torch.randn(1, 2, 200, 64, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(1, 2, 200, 64, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(1, 2, 200, 64, device="cuda", dtype=torch.bfloat16)
    _close(F.attention(q, k, v, causal=True), ref.attention_ref(q, k, v, causal=True))


def _bf16(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


# (name, Hq, Hkv, Sq, Sk) — q blocks are 128 rows; kv blocks are 64 rows at
# D=64 and 32 at D=128.
#   self:  Sq=160 is a full q block + a ragged one; Sk=160 is 2.5 kv blocks
#          at D=64 (ragged tail) and exactly 5 at D=128 (exact edge)
#   cross: Sk=77 is no multiple of 32 (SDXL text tokens); non-causal only
#   gqa:   two q heads per kv head, and causal_off = Sk - Sq > 0 when causal
_QKV_CASES = [
    ("self", 3, 3, 160, 160),
    ("cross", 3, 3, 160, 77),
    ("gqa", 4, 2, 96, 224),
]


@requires_gpu
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("case,causal", [
    (c, causal) for c in _QKV_CASES for causal in (False, True)
    if not (c[0] == "cross" and causal)
], ids=lambda p: p[0] if isinstance(p, tuple) else f"causal{int(p)}")
def test_attention_qkv_strided(case, causal, D):
    """The stride-aware BSHD entry every model uses, fed real strided views:
    slices of fused projections, never .contiguous() copies."""
    name, Hq, Hkv, Sq, Sk = case
    B = 2
    torch.manual_seed(0)
    if name == "self":
        qkv = _bf16(B, Sq, 3, Hq, D)  # fused QKV projection
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    else:
        q = _bf16(B, Sq, Hq, D) if name == "cross" else _bf16(B, Sq, 2, Hq, D)[:, :, 1]
        kv = _bf16(B, Sk, 2, Hkv, D)  # fused KV projection
        k, v = kv[:, :, 0], kv[:, :, 1]
    assert not k.is_contiguous() and not v.is_contiguous()
    out = F.attention_qkv(q, k, v, causal=causal)
    assert out.shape == (B, Sq, Hq * D)
    exp = ref.attention_ref(q.transpose(1, 2), k.transpose(1, 2),
                            v.transpose(1, 2), causal=causal)
    _close(out, exp.transpose(1, 2).reshape(B, Sq, Hq * D))


@requires_gpu
def test_unsupported_attention_config_raises():
    """An unsupported head dim or GQA group raises from the binding, on the
    host and before any launch — it must not take the process down."""
    lens = torch.tensor([16], device="cuda", dtype=torch.int32)
    with pytest.raises(RuntimeError, match="supported: 64, 128"):
        F.attention(_bf16(1, 2, 16, 80), _bf16(1, 2, 16, 80), _bf16(1, 2, 16, 80))
    with pytest.raises(RuntimeError, match="supported: 64, 128"):
        F.attention_qkv(_bf16(1, 16, 2, 80), _bf16(1, 16, 2, 80),
                        _bf16(1, 16, 2, 80))
    with pytest.raises(RuntimeError, match="supported: 64, 128"):
        F.paged_decode(_bf16(1, 4, 80), _bf16(1, 2, 16, 80), _bf16(1, 2, 16, 80),
                       None, lens)
    with pytest.raises(RuntimeError, match=r"supported: 1\.\.8"):
        F.paged_decode(_bf16(1, 32, 64), _bf16(1, 2, 16, 64), _bf16(1, 2, 16, 64),
                       None, lens)
    # the process and the stream are intact: a valid call still computes
    torch.manual_seed(18)
    q, k, v = _bf16(1, 2, 64, 64), _bf16(1, 2, 64, 64), _bf16(1, 2, 64, 64)
    _close(F.attention(q, k, v), ref.attention_ref(q, k, v))


@requires_gpu
@pytest.mark.parametrize("D", [64, 128])
def test_paged_decode_contiguous(D):
    torch.manual_seed(5)
    B, Hq, Hkv, S = 3, 8, 2, 300
    q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16)
    kc = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    lens = torch.tensor([300, 127, 64], device="cuda", dtype=torch.int32)
    out = F.paged_decode(q, kc, vc, None, lens)
    exp = ref.paged_decode_ref(q, kc, vc, None, lens.cpu(), S)
    _close(out, exp)


@requires_gpu
def test_paged_decode_split_s():
    """Long contiguous cache at tiny batch engages flash-decoding splits."""
    torch.manual_seed(55)
    B, Hq, Hkv, S, D = 1, 8, 2, 4096, 128
    q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16)
    kc = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
    lens = torch.tensor([3777], device="cuda", dtype=torch.int32)  # ragged
    out = F.paged_decode(q, kc, vc, None, lens)
    exp = ref.paged_decode_ref(q, kc, vc, None, lens.cpu(), S)
    _close(out, exp)


@requires_gpu
def test_paged_decode_block_table():
    torch.manual_seed(6)
    B, Hq, Hkv, D, BS = 2, 32, 8, 128, 16
    nblocks, max_blocks = 64, 20
    q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16)
    kc = torch.randn(nblocks, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    vc = torch.randn(nblocks, Hkv, BS, D, device="cuda", dtype=torch.bfloat16)
    bt = torch.randperm(nblocks, device="cuda")[: B * max_blocks].view(B, max_blocks).int()
    lens = torch.tensor([310, 77], device="cuda", dtype=torch.int32)
    out = F.paged_decode(q, kc, vc, bt, lens, block_size=BS)
    exp = ref.paged_decode_ref(q, kc, vc, bt.cpu(), lens.cpu(), BS)
    _close(out, exp)


@requires_gpu
def test_groupnorm_silu():
    torch.manual_seed(7)
    x = torch.randn(2, 64, 32, 32, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(64, device="cuda")
    b = torch.randn(64, device="cuda")
    _close(F.groupnorm_silu(x, g, b, 32), ref.groupnorm_silu_ref(x, g, b, 32))
    _close(F.groupnorm_silu(x, g, b, 32, do_silu=False),
           ref.groupnorm_silu_ref(x, g, b, 32, do_silu=False))


@requires_gpu
def test_layernorm():
    torch.manual_seed(8)
    x = torch.randn(512, 1280, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(1280, device="cuda")
    b = torch.randn(1280, device="cuda")
    _close(F.layernorm(x, g, b), ref.layernorm_ref(x, g, b))


@requires_gpu
def test_rmsnorm():
    torch.manual_seed(9)
    x = torch.randn(1024, 4096, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(4096, device="cuda")
    _close(F.rmsnorm(x, g), ref.rmsnorm_ref(x, g))


@requires_gpu
def test_cfg_euler():
    torch.manual_seed(10)
    n = 2 * 4 * 128 * 128 + 5  # ragged tail
    x = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    ec = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    eu = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    _close(F.cfg_euler(x, ec, eu, 7.5, -0.3), ref.cfg_euler_ref(x, ec, eu, 7.5, -0.3))
    _close(F.cfg_euler(x, ec, None, 0.0, -0.3), ref.cfg_euler_ref(x, ec, None, 0.0, -0.3))


@requires_gpu
def test_silu_mul_geglu_add():
    torch.manual_seed(11)
    a = torch.randn(4097 * 8, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(4097 * 8, device="cuda", dtype=torch.bfloat16)
    _close(F.silu_mul(a, b), ref.silu_mul_ref(a, b))
    _close(F.geglu(a, b), ref.geglu_ref(a, b))
    _close(F.add_residual(a, b), (a.float() + b.float()).to(torch.bfloat16))


@requires_gpu
def test_rope():
    torch.manual_seed(12)
    B, H, S, D = 2, 8, 128, 128
    x = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    cos, sin = F.rope_tables(256, D, device="cuda")
    _close(F.rope(x, cos, sin), ref.rope_ref(x, cos, sin))
    pos = torch.arange(64, 64 + S, device="cuda").int()
    _close(F.rope(x, cos, sin, positions=pos), ref.rope_ref(x, cos, sin, pos.long()))


@requires_gpu
def test_adamw():
    torch.manual_seed(13)
    n = 10_001
    p = torch.randn(n, device="cuda")
    g = torch.randn(n, device="cuda")
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    for step in (1, 2, 3):
        F.adamw_step(p, g, m, v, lr=1e-2, step=step)
        ref.adamw_ref(p2, g, m2, v2, 1e-2, 0.9, 0.999, 1e-8, 0.01, step)
    assert torch.allclose(p, p2, atol=1e-5, rtol=1e-4), (p - p2).abs().max()


@requires_gpu
def test_adamw_bf16_params():
    torch.manual_seed(14)
    n = 4096
    p = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(n, device="cuda", dtype=torch.bfloat16)
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda")
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    F.adamw_step(p, g, m, v, lr=1e-2, step=1)
    ref.adamw_ref(p2, g, m2, v2, 1e-2, 0.9, 0.999, 1e-8, 0.01, 1)
    _close(p, p2, atol=1e-2)


@requires_gpu
def test_sample_greedy_and_distribution():
    torch.manual_seed(15)
    logits = torch.randn(4, 32000, device="cuda")
    greedy = F.sample(logits, temperature=0.0)
    assert torch.equal(greedy.long(), logits.argmax(-1))
    # distribution sanity: a strongly-peaked row should sample its peak mostly
    peaked = torch.zeros(1, 1000, device="cuda")
    peaked[0, 123] = 10.0
    hits = 0
    for s in range(50):
        tok = F.sample(peaked, temperature=1.0, seed=1000 + s)
        hits += int(tok.item() == 123)
    assert hits >= 45, f"peak sampled only {hits}/50"


@requires_gpu
def test_softmax_rows():
    torch.manual_seed(16)
    x = torch.randn(8, 128000, device="cuda")
    _close(F.softmax(x), torch.softmax(x, -1), atol=1e-6, rtol=1e-4, frac=1.0)


@requires_gpu
def test_snapshot_roundtrip():
    from modal_examples_amd.gpu.snapshot import WeightSnapshot

    torch.manual_seed(17)
    tensors = {
        "a": torch.randn(1024, 1024, device="cuda", dtype=torch.bfloat16),
        "b": torch.randn(333, device="cuda"),
    }
    snap = WeightSnapshot.capture(tensors)
    originals = {k: t.clone() for k, t in tensors.items()}
    for t in tensors.values():
        t.zero_()
    snap.restore(tensors)
    for k in tensors:
        assert torch.equal(tensors[k], originals[k]), k
    snap.close()


@pytest.mark.gpu
def test_guard_band_around_inplace_rope():
    """Guard-band canaries survive the in-place RoPE kernel (no OOB writes),
    and the sync-debug proxy path executes the same kernel correctly."""
    import os

    import torch

    from modal_examples_amd.gpu.guard import GuardBand
    from modal_examples_amd.ops import functional as OF

    B, H, S, D = 2, 4, 64, 128
    g = GuardBand((B, H, S, D), dtype=torch.bfloat16, device="cuda")
    torch.manual_seed(0)
    g.tensor.copy_(torch.randn(B, H, S, D, device="cuda").bfloat16())
    cos, sin = OF.rope_tables(S, D, device="cuda")
    ref = OF.rope(g.tensor.clone(), cos, sin)
    OF.rope(g.tensor, cos, sin, inplace=True)
    torch.cuda.synchronize()
    g.check()
    assert torch.equal(g.tensor, ref)

    os.environ["MODAL_AMD_DEBUG_SYNC"] = "1"
    try:
        y2 = OF.rope(ref.clone(), cos, sin)
        assert torch.equal(y2, OF.rope(ref.clone(), cos, sin))
    finally:
        os.environ.pop("MODAL_AMD_DEBUG_SYNC", None)


@requires_gpu
@pytest.mark.parametrize("shape", [
    (2, 64, 64, 32, 32),      # generic
    (1, 512, 512, 64, 64),    # VAE-class
    (2, 4, 320, 16, 32),      # conv_in: tiny C, padded chunk
    (1, 128, 3, 24, 32),      # conv_out: K < 32, masked stores
    (1, 96, 64, 19, 45),      # ragged H/W: edge masking both dims
])
def test_conv3x3_vs_fp32(shape):
    """K3 NCHW implicit-GEMM conv vs torch fp32 conv2d."""
    N, C, K, H, W = shape
    torch.manual_seed(0)
    x = torch.randn(N, C, H, W, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(K, C, 3, 3, device="cuda", dtype=torch.bfloat16) / math.sqrt(C * 9)
    b = torch.randn(K, device="cuda", dtype=torch.float32)
    wr = F.repack_conv3x3_weight(w)
    got = F.conv3x3(x, wr, b.contiguous(), K, raw_weight=w)
    want = torch.nn.functional.conv2d(x.float(), w.float(), b, padding=1)
    _close(got, want, atol=5e-2, rtol=5e-2)


@requires_gpu
def test_conv3x3_fused_residual():
    N, C, K, H, W = 2, 64, 64, 16, 32
    torch.manual_seed(1)
    x = torch.randn(N, C, H, W, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(K, C, 3, 3, device="cuda", dtype=torch.bfloat16) / math.sqrt(C * 9)
    b = torch.zeros(K, device="cuda", dtype=torch.float32)
    r = torch.randn(N, K, H, W, device="cuda", dtype=torch.bfloat16)
    wr = F.repack_conv3x3_weight(w)
    got = F.conv3x3(x, wr, b, K, residual=r, raw_weight=w)
    want = torch.nn.functional.conv2d(x.float(), w.float(), b, padding=1) + r.float()
    _close(got, want, atol=5e-2, rtol=5e-2)


@requires_gpu
def test_conv3x3_fused_upsample():
    """UP variant == interpolate(nearest,2x) + conv2d."""
    N, C, K, H, W = 2, 32, 48, 12, 16
    torch.manual_seed(2)
    x = torch.randn(N, C, H, W, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(K, C, 3, 3, device="cuda", dtype=torch.bfloat16) / math.sqrt(C * 9)
    b = torch.randn(K, device="cuda", dtype=torch.float32)
    wr = F.repack_conv3x3_weight(w)
    got = F.conv3x3(x, wr, b, K, raw_weight=w, upsample=True)
    up = torch.nn.functional.interpolate(x.float(), scale_factor=2.0, mode="nearest")
    want = torch.nn.functional.conv2d(up, w.float(), b, padding=1)
    assert got.shape == want.shape
    _close(got, want, atol=5e-2, rtol=5e-2)


@requires_gpu
@pytest.mark.parametrize("upsample", [False, True])
def test_conv3x3_gn_fused(upsample):
    """GN+SiLU-fused conv == group_norm+silu (+interp) + conv2d fp32."""
    N, C, K, H, W = 2, 64, 32, 16, 32
    torch.manual_seed(3)
    x = torch.randn(N, C, H, W, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(K, C, 3, 3, device="cuda", dtype=torch.bfloat16) / math.sqrt(C * 9)
    b = torch.randn(K, device="cuda", dtype=torch.float32)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda") * 0.1
    wr = F.repack_conv3x3_weight(w)
    got = F.conv3x3_gn(x, wr, b, K, gamma, beta, groups=8, raw_weight=w,
                       upsample=upsample)
    h = torch.nn.functional.group_norm(x.float(), 8, gamma, beta, 1e-5)
    h = torch.nn.functional.silu(h)
    if upsample:
        h = torch.nn.functional.interpolate(h, scale_factor=2.0, mode="nearest")
    want = torch.nn.functional.conv2d(h, w.float(), b, padding=1)
    _close(got, want, atol=5e-2, rtol=5e-2)


@requires_gpu
@pytest.mark.parametrize("D", [64, 128])
def test_paged_decode_fp8_kv(D):
    """fp8 (e4m3) KV-cache decode vs the fp32 reference over the same
    quantized values — the kernel's HW fp8 conversion must match torch's."""
    B, Hq, Hkv, S = 4, 8, 2, 256
    torch.manual_seed(0)
    q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16)
    k8 = (torch.randn(B, Hkv, S, D, device="cuda") * 0.5).to(torch.float8_e4m3fn)
    v8 = (torch.randn(B, Hkv, S, D, device="cuda") * 0.5).to(torch.float8_e4m3fn)
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    got = F.paged_decode(q, k8.contiguous(), v8.contiguous(), None, lens)
    want = ref.paged_decode_ref(q.float(), k8.float(), v8.float(), None,
                                lens, S, 1.0 / math.sqrt(D))
    _close(got, want, atol=3e-2, rtol=3e-2)


@requires_gpu
@pytest.mark.parametrize("gelu", [False, True])
def test_glu_fused_matches_sliced(gelu):
    src = torch.randn(4, 37, 256, device="cuda", dtype=torch.bfloat16)
    got = F.glu_fused(src, gelu=gelu)
    a, b = src[..., :128].contiguous(), src[..., 128:].contiguous()
    want = F.geglu(a, b) if gelu else F.silu_mul(a, b)
    _close(got, want, atol=1e-2, rtol=1e-2)
