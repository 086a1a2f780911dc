"""The fused glue kernels of the SDXL step: scaled_softmax, GroupNorm with an
NHWC result, the transposing residual add, the conv3x3 epilogue addend and
add_layernorm, each against the torch expression it replaces in the models,
then the four rewired modules against the op sequence they ran before.

Every kernel reproduces the arithmetic of the chain it replaces, so the
comparisons are torch.equal wherever the result is reproducible.  GroupNorm
sums with float atomics; its exact cases use integer inputs with slabs of at
most 2^17 elements in [-8, 8], for which both sums (at most 2^17 * 64 = 2^23)
are exact in fp32 in any order.  Only the softmax is compared within a bound:
its fp32 exponential and sum are not the library's, so a probability may land
on the neighbouring bf16 value (bound and cap: test_scaled_softmax).

GPU tests carry `pytest.mark.gpu` and the `requires_gpu` skip, one by one.
"""
import functools

import pytest
import torch

import modal_examples_amd.ops.functional as F
import modal_examples_amd.ops.reference as ref

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

GN_TOL = dict(atol=2e-2, rtol=2e-2, frac=0.999)  # tests/test_kernels_gpu.py


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, atol, rtol, frac):
    a, b = a.float(), b.float()
    ok = (a - b).abs() <= (atol + rtol * b.abs())
    good = ok.float().mean().item()
    assert good >= frac, (f"only {good:.5f} of elements within tol; max err "
                          f"{(a - b).abs().max().item():.4f}")


def _exact(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    diff = got != want  # true for NaN as well
    first = diff.nonzero()[0].tolist()
    raise AssertionError(
        f"{what}: {int(diff.sum())} of {diff.numel()} elements differ, first "
        f"at {first}: got {float(got[tuple(first)])}, want "
        f"{float(want[tuple(first)])}")


def _ext():
    from modal_examples_amd.ops._build import get_ext

    return get_ext(required=True)


# -------------------------------------------------------------- scaled_softmax

_SCALE = 512 ** -0.5


@functools.lru_cache(maxsize=None)
def _softmax_case(rows, cols):
    """rows of 3*randn, then the three special rows: all values equal, a
    single +60 outlier, magnitude 30."""
    g = _gen(rows * 100003 + cols)
    s = 3 * torch.randn(rows + 3, cols, generator=g)
    s[rows] = 1.5
    s[rows + 1, cols // 3] = 60.0
    s[rows + 2] = 30 * torch.randn(cols, generator=g)
    return s.to(torch.bfloat16)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("shape", ((5, 8), (3, 40), (5, 2048), (3, 2056),
                                   (2, 16384)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_scaled_softmax(shape):
    """Against the chain on the same device: no element more than one bf16
    step away, and at most 0.5 % of the elements different at all.  (The
    chain itself differs from a float64 softmax, and from an exp2
    evaluation, in at most 2.5e-4 of the elements at these shapes; a kernel
    that skips the bf16 rounding of the product differs in tens of percent.)
    Probabilities are non-negative, so one bf16 step is a difference of one
    in the bit pattern.  2056 columns take one register vector more than
    2048, 16384 is the longest register-resident row."""
    s = _softmax_case(*shape).cuda()
    want = torch.softmax((s * _SCALE).float(), -1).to(torch.bfloat16)
    got = F.scaled_softmax(s, _SCALE)
    assert got.shape == want.shape and got.dtype == torch.bfloat16
    assert torch.isfinite(got.float()).all()
    steps = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()
    differ = float((steps != 0).float().mean())
    print(f"scaled_softmax {shape}: max {int(steps.max())} bf16 steps, "
          f"{differ:.2e} of the elements differ")
    assert int(steps.max()) <= 1
    assert differ <= 0.005


@pytest.mark.gpu
@requires_gpu
def test_scaled_softmax_long_rows_and_batch_dims():
    """Past 16384 columns the kernel reads the row again instead of keeping
    it in registers; leading dimensions are flattened into rows."""
    g = _gen(77)
    s = (3 * torch.randn(2, 2, 16392, generator=g)).to(torch.bfloat16).cuda()
    want = torch.softmax((s * _SCALE).float(), -1).to(torch.bfloat16)
    got = F.scaled_softmax(s, _SCALE)
    steps = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()
    assert got.shape == want.shape
    assert int(steps.max()) <= 1
    assert float((steps != 0).float().mean()) <= 0.005


@pytest.mark.gpu
@requires_gpu
def test_scaled_softmax_other_inputs_take_the_torch_expression():
    g = _gen(78)
    s = torch.randn(4, 12, generator=g).to(torch.bfloat16).cuda()  # 12 % 8 != 0
    _exact(F.scaled_softmax(s, 0.25),
           torch.softmax((s * 0.25).float(), -1).to(torch.bfloat16), "12 cols")
    t = torch.randn(4, 32, generator=g).to(torch.bfloat16).cuda()[:, ::2]
    _exact(F.scaled_softmax(t, 0.25),
           torch.softmax((t * 0.25).float(), -1).to(torch.bfloat16), "strided")


# ------------------------------------------------- groupnorm_silu(out_nhwc=True)

_GN_SHAPES = ((2, 64, 32, 5, 7),     # HW % 8 != 0
              (1, 320, 32, 16, 16),  # 10 channels per group
              (1, 32, 32, 72, 72),   # the statistics pass splits each slab
              (3, 40, 8, 9, 33))     # C and HW off the tile


@functools.lru_cache(maxsize=None)
def _gn_case(N, C, G, H, W):
    assert (C // G) * H * W <= 2 ** 17
    g = _gen((((N * 31 + C) * 31 + G) * 31 + H) * 31 + W)
    x = torch.randint(-8, 9, (N, C, H, W), generator=g).to(torch.bfloat16)
    return x, torch.randn(C, generator=g), torch.randn(C, generator=g)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("silu", (True, False), ids=("silu", "plain"))
@pytest.mark.parametrize("shape", _GN_SHAPES,
                         ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_nhwc(shape, silu):
    N, C, G, H, W = shape
    x, gamma, beta = (t.cuda() for t in _gn_case(*shape))
    got = F.groupnorm_silu(x, gamma, beta, G, do_silu=silu, out_nhwc=True)
    nchw = F.groupnorm_silu(x, gamma, beta, G, do_silu=silu)
    _exact(got, nchw.permute(0, 2, 3, 1).reshape(N, H * W, C),
           f"{shape} silu={silu} against the NCHW kernel")
    want = ref.groupnorm_silu_ref(x, gamma, beta, G, do_silu=silu)
    _close(got, want.permute(0, 2, 3, 1).reshape(N, H * W, C), **GN_TOL)


# ------------------------------------------------------------ add_nhwc_to_nchw

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("shape", ((2, 40, 5, 7), (1, 640, 8, 8), (1, 8, 1, 1),
                                   (2, 72, 33, 9)),
                         ids=lambda s: "x".join(map(str, s)))
def test_add_nhwc_to_nchw(shape):
    N, C, H, W = shape
    g = _gen(((N * 31 + C) * 31 + H) * 31 + W)
    res = torch.randn(N, C, H, W, generator=g).to(torch.bfloat16).cuda()
    h = torch.randn(N, H * W, C, generator=g).to(torch.bfloat16).cuda()
    want = res + h.reshape(N, H, W, C).permute(0, 3, 1, 2)
    got = F.add_nhwc_to_nchw(res, h)
    assert got.is_contiguous()
    _exact(got, want.contiguous(), f"{shape}")


# ----------------------------------------------------------------- conv addend

@functools.lru_cache(maxsize=None)
def _conv_case(K, H, W):
    """The exact-integer operands of tests/test_conv3x3_pipeline_gpu.py (x and
    w in [-2, 2], bias in [-4, 4]) and an integer addend that differs per
    image: every sum stays an integer below 2^24."""
    N, C = 2, 20
    g = _gen((K * 211 + H) * 211 + W)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).to(torch.bfloat16)
    w = torch.randint(-2, 3, (K, C, 3, 3), generator=g).to(torch.bfloat16)
    bias = torch.randint(-4, 5, (K,), generator=g).float()
    t = torch.randint(-6, 7, (N, K), generator=g).to(torch.bfloat16)
    assert not torch.equal(t[0], t[1])
    return x, w, bias, t


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("HW", ((8, 32), (9, 33)), ids=("8x32", "9x33"))
@pytest.mark.parametrize("K", (3, 64, 65, 320))
def test_conv3x3_addend(K, HW):
    """8 x 32 with K a multiple of 64 is interior tiles alone, 9 x 33 and the
    other K have edge tiles."""
    x, w, bias, t = (v.cuda() for v in _conv_case(K, *HW))
    wr = F.repack_conv3x3_weight(w)
    want = F.conv3x3(x, wr, bias, K, raw_weight=w) + t[:, :, None, None]
    got = F.conv3x3(x, wr, bias, K, raw_weight=w, addend=t)
    _exact(got, want, f"K={K} {HW}")
    # and the chain itself is the exact integer result
    exact = torch.nn.functional.conv2d(x.double(), w.double(), bias.double(),
                                       padding=1).to(torch.bfloat16)
    _exact(want, (exact.float() + t.float()[:, :, None, None])
           .to(torch.bfloat16), f"K={K} {HW} chain against float64")


@pytest.mark.gpu
@requires_gpu
def test_conv3x3_addend_with_residual_raises():
    x, w, bias, t = (v.cuda() for v in _conv_case(64, 8, 32))
    wr = F.repack_conv3x3_weight(w)
    res = torch.zeros(2, 64, 8, 32, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        F.conv3x3(x, wr, bias, 64, residual=res, raw_weight=w, addend=t)
    with pytest.raises(RuntimeError, match="cannot be combined"):
        _ext().conv3x3(x, wr, bias, res, 64, False, t)


# --------------------------------------------------------------- add_layernorm

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("D", (40, 640, 1280))
@pytest.mark.parametrize("rows", (1, 5, 8))
def test_add_layernorm(rows, D):
    """D = 40 is the row tail: 5 vectors on 5 lanes of the wave, the other 59
    idle; 640 and 1280 keep 2 and 3 vectors per lane in registers.  5 rows
    leave a block with one wave, 8 fill two blocks."""
    g = _gen(rows * 10007 + D)
    x = torch.randn(rows, D, generator=g).to(torch.bfloat16).cuda()
    y = torch.randn(rows, D, generator=g).to(torch.bfloat16).cuda()
    gamma = torch.randn(D, generator=g).cuda()
    beta = torch.randn(D, generator=g).cuda()
    s_want = x + y
    ln_want = F.layernorm(s_want, gamma, beta)
    s, ln = F.add_layernorm(x, y, gamma, beta)
    _exact(s, s_want, f"sum {rows}x{D}")
    _exact(ln, ln_want, f"norm {rows}x{D}")


@pytest.mark.gpu
@requires_gpu
def test_add_layernorm_long_rows_and_batch_dims():
    """D = 2600 is past the 2048 columns a wave keeps in registers, so the
    rest of the row is read twice; leading dimensions flatten into rows."""
    D = 2600
    g = _gen(D)
    x = torch.randn(3, 2, D, generator=g).to(torch.bfloat16).cuda()
    y = torch.randn(3, 2, D, generator=g).to(torch.bfloat16).cuda()
    gamma = torch.randn(D, generator=g).cuda()
    beta = torch.randn(D, generator=g).cuda()
    s, ln = F.add_layernorm(x, y, gamma, beta)
    _exact(s, x + y, f"sum D={D}")
    _exact(ln, F.layernorm(x + y, gamma, beta), f"norm D={D}")


# ----------------------------------------------------------------- model level

def _module(ctor, seed):
    """An eval-mode bf16 module on the GPU whose norm parameters are not the
    identity."""
    torch.manual_seed(seed)
    m = ctor()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "norm" in name:
                p.copy_(torch.randn_like(p) * 0.5 + (1.0 if name.endswith(
                    "weight") else 0.0))
    return m.to(device="cuda", dtype=torch.bfloat16).eval()


def _rand(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed)).to(torch.bfloat16).cuda()


def _old_transformer_block(m, x, ctx):
    x = x + m.attn1(m.norm1(x))
    x = x + m.attn2(m.norm2(x), ctx)
    x = x + m.ff(m.norm3(x))
    return x


@pytest.mark.gpu
@requires_gpu
def test_transformer_block_matches_the_separate_ops():
    from modal_examples_amd.models.sdxl.layers import TransformerBlock
    from modal_examples_amd.models.sdxl.unet import UNetConfig

    cfg = UNetConfig.small()
    dim = cfg.channels[1]
    m = _module(lambda: TransformerBlock(dim, cfg.ctx_dim, cfg.head_dim), 1)
    x, ctx = _rand(2, 64, dim, seed=2), _rand(2, 77, cfg.ctx_dim, seed=3)
    with torch.no_grad():
        _exact(m(x, ctx), _old_transformer_block(m, x, ctx), "TransformerBlock")


@pytest.mark.gpu
@requires_gpu
def test_spatial_transformer_matches_the_separate_ops():
    from modal_examples_amd.models.sdxl.unet import SpatialTransformer, UNetConfig

    cfg = UNetConfig.small()
    C = cfg.channels[1]
    m = _module(lambda: SpatialTransformer(C, 1, cfg.ctx_dim, cfg.head_dim), 4)
    B, H, W = 2, 16, 16
    x, ctx = _rand(B, C, H, W, seed=5), _rand(B, 77, cfg.ctx_dim, seed=6)
    with torch.no_grad():
        h = m.norm(x).permute(0, 2, 3, 1).reshape(B, H * W, C)
        h = m.proj_in(h)
        for blk in m.blocks:
            h = _old_transformer_block(blk, h, ctx)
        h = m.proj_out(h)
        want = x + h.reshape(B, H, W, C).permute(0, 3, 1, 2)
        got = m(x, ctx)
    assert got.shape == want.shape and got.is_contiguous()
    _close(got, want, **GN_TOL)  # GroupNorm atomics at the entry


@pytest.mark.gpu
@requires_gpu
def test_resnet_block_matches_the_separate_ops():
    from modal_examples_amd.models.sdxl.unet import ResnetBlock, UNetConfig

    cfg = UNetConfig.small()
    c_in, c_out = cfg.channels[0], cfg.channels[1]
    m = _module(lambda: ResnetBlock(c_in, c_out, cfg.time_embed_dim), 7)
    x = _rand(2, c_in, 16, 16, seed=8)
    temb = _rand(2, cfg.time_embed_dim, seed=9)
    with torch.no_grad():
        h = m.conv1(m.norm1(x))
        h = h + m.temb_proj(torch.nn.functional.silu(temb))[:, :, None, None]
        want = m.conv2(m.norm2(h), residual=m.skip(x))
        got = m(x, temb)
    _close(got, want, **GN_TOL)  # GroupNorm atomics in norm1 and norm2


@pytest.mark.gpu
@requires_gpu
def test_vae_mid_attention_matches_the_separate_ops():
    from modal_examples_amd.models.sdxl.vae import VAEMidAttention

    C, B, H, W = 64, 2, 16, 16
    m = _module(lambda: VAEMidAttention(C, chunk=128), 10)
    x = _rand(B, C, H, W, seed=11)
    with torch.no_grad():
        h = m.norm(x).permute(0, 2, 3, 1).reshape(B, H * W, C)
        q, k, v = m.q(h), m.k(h), m.v(h)
        outs = []
        for i in range(0, q.shape[1], m.chunk):
            s = torch.matmul(q[:, i:i + m.chunk], k.transpose(1, 2)) * m.scale
            p = torch.softmax(s.float(), dim=-1).to(v.dtype)
            outs.append(torch.matmul(p, v))
        o = m.out(torch.cat(outs, dim=1))
        want = x + o.reshape(B, H, W, C).permute(0, 3, 1, 2)
        got = m(x)
    assert got.shape == want.shape and got.is_contiguous()
    _close(got, want, **GN_TOL)  # GroupNorm atomics at the entry


# ------------------------------------------------------------- argument checks

def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16, device="cuda")


def _f32(*shape):
    return torch.zeros(*shape, dtype=torch.float32, device="cuda")


@pytest.mark.gpu
@requires_gpu
def test_bindings_reject_bad_arguments():
    """float32 where bf16 is expected, a CPU tensor, a shape mismatch and a
    non-contiguous tensor each raise before anything is launched."""
    ext = _ext()
    calls = {
        "scaled_softmax": (
            lambda s: ext.scaled_softmax(s, 0.5),
            _bf(4, 16), (_bf(4, 12), _bf(4, 32)[:, ::2])),
        "groupnorm_silu_nhwc": (
            lambda x, g=None: ext.groupnorm_silu_nhwc(
                x, _f32(32) if g is None else g, _f32(32), 8, 1e-5, True),
            _bf(1, 32, 4, 4), (_bf(1, 36, 4, 4), _bf(32, 4, 4),
                               _bf(1, 32, 4, 8)[:, :, :, ::2])),
        "add_layernorm": (
            lambda x, y=None: ext.add_layernorm(
                x, _bf(4, 16) if y is None else y, _f32(16), _f32(16), 1e-5),
            _bf(4, 16), (_bf(4, 24), _bf(2, 16), _bf(4, 32)[:, ::2])),
        "add_nhwc_to_nchw": (
            lambda r, h=None: ext.add_nhwc_to_nchw(
                r, _bf(1, 16, 8) if h is None else h),
            _bf(1, 8, 4, 4), (_bf(1, 8, 4, 5), _bf(8, 4, 4),
                              _bf(1, 8, 4, 8)[:, :, :, ::2])),
    }
    for name, (call, good, bad_shapes) in calls.items():
        call(good)  # the well-formed call goes through
        with pytest.raises(RuntimeError):
            call(good.float())
        with pytest.raises(RuntimeError):
            call(good.cpu())
        for bad in bad_shapes:
            with pytest.raises(RuntimeError):
                call(bad)
    # the second operand of the two-tensor ops, and the fp32 parameters
    with pytest.raises(RuntimeError):
        calls["add_layernorm"][0](_bf(4, 16), _f32(4, 16))
    with pytest.raises(RuntimeError):
        calls["add_layernorm"][0](_bf(4, 16), _bf(4, 16).cpu())
    with pytest.raises(RuntimeError):
        calls["add_nhwc_to_nchw"][0](_bf(1, 8, 4, 4), _bf(1, 8, 16))
    with pytest.raises(RuntimeError):
        calls["add_nhwc_to_nchw"][0](_bf(1, 8, 4, 4), _f32(1, 16, 8))
    with pytest.raises(RuntimeError):
        calls["groupnorm_silu_nhwc"][0](_bf(1, 32, 4, 4), _f32(31))
    with pytest.raises(RuntimeError):
        calls["groupnorm_silu_nhwc"][0](_bf(1, 32, 4, 4), _bf(32))
    with pytest.raises(RuntimeError):  # groups must divide C
        ext.groupnorm_silu_nhwc(_bf(1, 32, 4, 4), _f32(32), _f32(32), 5, 1e-5,
                                True)


@pytest.mark.gpu
@requires_gpu
def test_conv3x3_addend_argument_checks():
    x, w, bias, t = (v.cuda() for v in _conv_case(64, 8, 32))
    wr = F.repack_conv3x3_weight(w)
    ext = _ext()
    ext.conv3x3(x, wr, bias, None, 64, False, t)
    for bad in (t.float(), t.cpu(), t[:, :63].contiguous(), t[:1],
                _bf(2, 128)[:, ::2]):
        with pytest.raises(RuntimeError):
            ext.conv3x3(x, wr, bias, None, 64, False, bad)
