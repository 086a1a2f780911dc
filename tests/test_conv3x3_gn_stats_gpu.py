"""conv3x3 with GroupNorm statistics from its epilogue, and their consumers.

`F.conv3x3(..., gn_groups=G)` returns the output and, per (image, group), the
sum and the sum of squares of the values it stored; `F.groupnorm_silu(...,
stats=)` and `F.conv3x3_gn(..., stats=)` then skip their statistics pass.
What can go wrong: a masked pixel or a channel past K that is counted, a quad
of channels credited to the wrong group (a group that straddles two 64-channel
tiles), a pixel tile left out or counted twice, a wrong lane after the
half-wave exchange, an output that changes because statistics were asked for.

Exact cases use integer operands: x in [-1, 1], sparse weights in [-1, 1], bias,
residual and addend in [-2, 2].  Every output is then an integer of magnitude
at most 256 (a bf16 value), every sum of values or squares over a group stays
below 2^24, so every f32 partial sum in any order is exact: the comparisons are
torch.equal.  `test_exact_cases_are_exact` checks those conditions on the CPU.

GPU tests carry `pytest.mark.gpu` and the `requires_gpu` skip, one by one.
"""
import functools
import os
from types import SimpleNamespace

import pytest
import torch

import modal_examples_amd.ops.functional as F

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

GN_TOL = dict(atol=2e-2, rtol=2e-2, frac=0.999)  # tests/test_sdxl_glue_gpu.py


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _up2(t):
    return torch.nn.functional.interpolate(t, scale_factor=2.0, mode="nearest")


# (N, C, K, G, H, W, variant); H, W are the source's
_EXACT = {
    "interior": (2, 16, 64, 16, 8, 32, "plain"),
    "two-k-tiles": (2, 32, 128, 32, 16, 64, "plain"),
    "two-k-tiles-residual": (2, 32, 128, 32, 16, 64, "residual"),
    "two-k-tiles-addend": (2, 32, 128, 32, 16, 64, "addend"),
    "group-straddles-tiles": (2, 16, 96, 8, 8, 32, "plain"),
    "edge-9x33": (2, 16, 64, 16, 9, 33, "plain"),
    "edge-7x31": (2, 16, 64, 16, 7, 31, "plain"),
    "upsample-5x17": (2, 16, 64, 16, 5, 17, "upsample"),
    "conv-in-class": (1, 4, 512, 32, 8, 32, "plain"),
}
_NO_STATS = (2, 16, 80, 8, 8, 32, "plain")  # cpg 10
_RPW4 = ("edge-9x33", "group-straddles-tiles")


@functools.lru_cache(maxsize=None)
def _case(N, C, K, G, H, W, variant):
    """Integer operands (CPU) and the float64 reference of the output."""
    g = _gen((((((N * 211 + C) * 211 + K) * 211 + G) * 211 + H) * 211 + W) * 4
             + ("plain", "residual", "addend", "upsample").index(variant))
    up = variant == "upsample"
    x = torch.randint(-1, 2, (N, C, H, W), generator=g).to(torch.bfloat16)
    keep = torch.rand(K, C, 3, 3, generator=g) < min(1.0, 6.0 / (9 * C))
    w = (torch.randint(-1, 2, (K, C, 3, 3), generator=g) * keep).to(
        torch.bfloat16)
    bias = torch.randint(-2, 3, (K,), generator=g).float()
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    res = (torch.randint(-2, 3, (N, K, Ho, Wo), generator=g).to(torch.bfloat16)
           if variant == "residual" else None)
    add = (torch.randint(-2, 3, (N, K), generator=g).to(torch.bfloat16)
           if variant == "addend" else None)
    xin = _up2(x.double()) if up else x.double()
    want = torch.nn.functional.conv2d(xin, w.double(), bias.double(), padding=1)
    if res is not None:
        want = want + res.double()
    if add is not None:
        want = want + add.double()[:, :, None, None]
    return SimpleNamespace(x=x, w=w, bias=bias, res=res, add=add, K=K, G=G,
                           upsample=up, want=want)


def _sums(y, G):
    """float64 (sum, sumsq) per (n, group) of a stored tensor: [N, G, 2]."""
    v = y.detach().float().double().cpu()
    v = v.reshape(v.shape[0], G, -1)
    return torch.stack((v.sum(-1), (v * v).sum(-1)), dim=-1)


def test_exact_cases_are_exact():
    """The conditions of the exact cases (no GPU): the reference is an
    integer of magnitude at most 256, hence a bf16 value and the stored
    output; the sums and sums of squares over every group, and so each of
    their partial sums, are integers below 2^24."""
    for name, spec in list(_EXACT.items()) + [("no-stats", _NO_STATS)]:
        c = _case(*spec)
        assert torch.equal(c.want, c.want.round()), name
        assert float(c.want.abs().max()) <= 256, name
        assert torch.equal(c.want.bfloat16().double(), c.want), name
        s = _sums(c.want, c.G)
        absum = c.want.abs().reshape(c.want.shape[0], c.G, -1).sum(-1)
        top = max(float(absum.max()), float(s[..., 1].max()))
        print(f"{name}: largest |y| {float(c.want.abs().max()):.0f}, largest "
              f"group sum of |y| or y^2 {top:.0f}")
        assert top < 2.0 ** 24, name
        assert float(s[..., 1].min()) > 0, name  # no all-zero group


def _run(c, gn_groups=None):
    wd = c.w.cuda()
    return F.conv3x3(c.x.cuda(), F.repack_conv3x3_weight(wd), c.bias.cuda(),
                     c.K, residual=None if c.res is None else c.res.cuda(),
                     raw_weight=wd, upsample=c.upsample,
                     addend=None if c.add is None else c.add.cuda(),
                     gn_groups=gn_groups)


def _check_exact(name):
    c = _case(*_EXACT[name])
    plain = _run(c)
    y, stats = _run(c, gn_groups=c.G)
    assert stats is not None and stats.dtype is torch.float32
    assert tuple(stats.shape) == (c.x.shape[0], c.G, 2)
    assert torch.equal(y, plain), f"{name}: output changed with statistics"
    assert torch.equal(y.double().cpu(), c.want), f"{name}: output"
    got, want = stats.double().cpu(), _sums(y, c.G)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()[0].tolist()
        raise AssertionError(
            f"{name}: {int((got != want).sum())} of {got.numel()} statistics "
            f"differ, first at (n, g, sum/sumsq) = {bad}: got "
            f"{float(got[tuple(bad)])}, want {float(want[tuple(bad)])}")


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("name", sorted(_EXACT))
def test_statistics_exact(name):
    _check_exact(name)


@pytest.mark.gpu
@requires_gpu
def test_no_statistics_when_groups_do_not_hold_quads():
    """cpg = 10: the op returns None and the consumer takes its own
    statistics pass; the sums are exact integers, so that path is
    deterministic and the two results are equal."""
    c = _case(*_NO_STATS)
    y, stats = _run(c, gn_groups=c.G)
    assert stats is None
    assert torch.equal(y, _run(c))
    gamma = (torch.rand(c.K, generator=_gen(1)) + 0.5).cuda()
    beta = torch.randn(c.K, generator=_gen(2)).cuda()
    for nhwc in (False, True):
        got = F.groupnorm_silu(y, gamma, beta, c.G, out_nhwc=nhwc, stats=stats)
        want = F.groupnorm_silu(y, gamma, beta, c.G, out_nhwc=nhwc)
        assert torch.equal(got, want)


def _rpw4_main():
    """The child of test_statistics_four_rows_per_wave."""
    torch.cuda.init()
    for name in _RPW4:
        _check_exact(name)
    torch.cuda.synchronize()
    print(f"{len(_RPW4)} cases with MODAL_AMD_CONV_RPW="
          f"{os.environ.get('MODAL_AMD_CONV_RPW')}")


@pytest.mark.gpu
@requires_gpu
def test_statistics_four_rows_per_wave():
    """MODAL_AMD_CONV_RPW=4 is read once per process: a fresh child runs an
    edge case (16-row tiles over 9 rows) and the straddling groups.  The
    limit is far above the few seconds the child takes with its start."""
    import subprocess
    import sys

    tests_dir = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MODAL_AMD_CONV_RPW="4")
    code = ("import sys; sys.path[:0] = [%r, %r]; "
            "import test_conv3x3_gn_stats_gpu as t; t._rpw4_main()"
            % (os.path.dirname(tests_dir), tests_dir))
    r = subprocess.run([sys.executable, "-c", code], env=env, timeout=120.0,
                       capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (f"child exited with {r.returncode}\n"
                               f"{r.stdout[-4000:]}\n{r.stderr[-8000:]}")
    assert "MODAL_AMD_CONV_RPW=4" in r.stdout


# ------------------------------------------------------- random inputs

@functools.lru_cache(maxsize=None)
def _rand_case(N, C, K, H, W):
    g = _gen(((N * 31 + C) * 31 + K) * 31 + H * W)
    x = torch.randn(N, C, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(K, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(
        torch.bfloat16)
    bias = torch.randn(K, generator=g)
    gamma = torch.rand(K, generator=g) + 0.5
    beta = torch.randn(K, generator=g)
    # groups of 4 channels, SDXL's smallest: 32 groups at K 128, 16 at K 64
    return SimpleNamespace(x=x, w=w, bias=bias, gamma=gamma, beta=beta, K=K,
                           G=K // 4)


_RAND = ((2, 64, 128, 24, 40), (2, 32, 64, 64, 64))


def _conv_rand(c, gn_groups=None):
    wd = c.w.cuda()
    return F.conv3x3(c.x.cuda(), F.repack_conv3x3_weight(wd), c.bias.cuda(),
                     c.K, raw_weight=wd, gn_groups=gn_groups)


def _gn_silu64(y, c):
    h = torch.nn.functional.group_norm(y.double().cpu(), c.G, c.gamma.double(),
                                       c.beta.double(), 1e-5)
    return torch.nn.functional.silu(h)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("shape", _RAND, ids=lambda s: "x".join(map(str, s)))
def test_deterministic(shape):
    c = _rand_case(*shape)
    y1, s1 = _conv_rand(c, c.G)
    y2, s2 = _conv_rand(c, c.G)
    assert torch.equal(y1, y2) and torch.equal(s1, s2)
    assert torch.equal(y1, _conv_rand(c))


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("nhwc", (False, True), ids=("nchw", "nhwc"))
@pytest.mark.parametrize("shape", _RAND, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_with_statistics_is_as_accurate(shape, nhwc):
    """Against float64 GroupNorm+SiLU of the stored conv output: the largest
    error with the epilogue's statistics is at most twice that of the
    statistics pass (the margin of tests/test_moe_fused_gpu.py for a
    reordered f32 sum)."""
    c = _rand_case(*shape)
    y, stats = _conv_rand(c, c.G)
    assert stats is not None
    want = _gn_silu64(y, c)
    if nhwc:
        want = want.permute(0, 2, 3, 1).reshape(y.shape[0], -1, c.K)
    gamma, beta = c.gamma.cuda(), c.beta.cuda()
    new = F.groupnorm_silu(y, gamma, beta, c.G, out_nhwc=nhwc, stats=stats)
    old = F.groupnorm_silu(y, gamma, beta, c.G, out_nhwc=nhwc)
    e_new = float((new.double().cpu() - want).abs().max())
    e_old = float((old.double().cpu() - want).abs().max())
    print(f"groupnorm_silu {shape} nhwc={nhwc}: max error {e_new:.3e} with "
          f"statistics, {e_old:.3e} without")
    assert e_new <= 2 * e_old


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("shape", _RAND, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_gn_with_statistics_is_as_accurate(shape):
    """conv3x3_gn over the first conv's output, with and without its
    statistics, against float64 GroupNorm+SiLU+conv of that stored output."""
    c = _rand_case(*shape)
    y, stats = _conv_rand(c, c.G)
    g = _gen(shape[1] + 7)
    K2 = 64
    w2 = (torch.randn(K2, c.K, 3, 3, generator=g) / (3 * c.K ** 0.5)).to(
        torch.bfloat16)
    b2 = torch.randn(K2, generator=g)
    want = torch.nn.functional.conv2d(_gn_silu64(y, c), w2.double(),
                                      b2.double(), padding=1)
    wd = w2.cuda()
    args = (y, F.repack_conv3x3_weight(wd), b2.cuda(), K2, c.gamma.cuda(),
            c.beta.cuda())
    new = F.conv3x3_gn(*args, groups=c.G, raw_weight=wd, stats=stats)
    old = F.conv3x3_gn(*args, groups=c.G, raw_weight=wd)
    e_new = float((new.double().cpu() - want).abs().max())
    e_old = float((old.double().cpu() - want).abs().max())
    print(f"conv3x3_gn {shape}: max error {e_new:.3e} with statistics, "
          f"{e_old:.3e} without")
    assert e_new <= 2 * e_old


@pytest.mark.gpu
@requires_gpu
def test_graph_replay_matches_eager():
    """conv -> groupnorm_silu(stats) captured once; each replay after the
    input buffer is overwritten equals the eager pair on the same input."""
    c = _rand_case(*_RAND[0])
    wd = c.w.cuda()
    wr, bias = F.repack_conv3x3_weight(wd), c.bias.cuda()
    gamma, beta = c.gamma.cuda(), c.beta.cuda()

    def pair(x):
        y, s = F.conv3x3(x, wr, bias, c.K, raw_weight=wd, gn_groups=c.G)
        return F.groupnorm_silu(y, gamma, beta, c.G, stats=s)

    buf = c.x.cuda().clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair(buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pair(buf)
    for i in range(3):
        x = torch.randn(c.x.shape, generator=_gen(100 + i)).to(
            torch.bfloat16).cuda()
        buf.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, pair(x)), f"replay {i}"


# ------------------------------------------------------------- wiring

def _module(ctor, seed):
    """An eval-mode bf16 module on the GPU whose norm parameters are not the
    identity (tests/test_sdxl_glue_gpu.py)."""
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


def _close(a, b, atol, rtol, frac):
    a, b = a.float(), b.float()
    ok = (a - b).abs() <= (atol + rtol * b.abs())
    good = ok.float().mean().item()
    assert good >= frac, (f"only {good:.5f} of elements within tol; max err "
                          f"{(a - b).abs().max().item():.4f}")


def _on_and_off(monkeypatch, fn):
    """fn() with statistics passed from conv to norm, and with every norm
    taking its own."""
    from modal_examples_amd.models.sdxl import layers

    with torch.no_grad():
        monkeypatch.setattr(layers, "GN_STATS_FROM_CONV", True)
        on = fn()
        monkeypatch.setattr(layers, "GN_STATS_FROM_CONV", False)
        off = fn()
    return on, off


@pytest.mark.gpu
@requires_gpu
def test_vae_resnet_wiring(monkeypatch):
    from modal_examples_amd.models.sdxl.layers import Conv3x3
    from modal_examples_amd.models.sdxl.vae import VAEResnet

    m = _module(lambda: VAEResnet(128, 256), 21)
    conv = _module(lambda: Conv3x3(32, 128), 22)
    z = _rand(2, 32, 16, 24, seed=23)

    def fn():
        x, s = conv(z, gn_groups=32)
        y, s2 = m(x, stats=s, gn_groups=32)
        return y, s, s2

    (on, s, s2), (off, t, t2) = _on_and_off(monkeypatch, fn)
    assert s is not None and s2 is not None and t is None and t2 is None
    assert tuple(s2.shape) == (2, 32, 2)
    _close(on, off, **GN_TOL)
    with torch.no_grad():
        _close(m(conv(z)), off, **GN_TOL)  # a tensor in, a tensor out


@pytest.mark.gpu
@requires_gpu
def test_unet_resnet_block_wiring(monkeypatch):
    from modal_examples_amd.models.sdxl.layers import Conv3x3
    from modal_examples_amd.models.sdxl.unet import ResnetBlock, UNetConfig

    cfg = UNetConfig.small()
    m = _module(lambda: ResnetBlock(128, 256, cfg.time_embed_dim), 24)
    conv = _module(lambda: Conv3x3(32, 128), 25)
    z = _rand(2, 32, 16, 16, seed=26)
    temb = _rand(2, cfg.time_embed_dim, seed=27)

    def fn():
        x, s = conv(z, gn_groups=32)
        return m(x, temb, stats=s, gn_groups=32)

    (on, s), (off, t) = _on_and_off(monkeypatch, fn)
    assert s is not None and t is None
    _close(on, off, **GN_TOL)


@pytest.mark.gpu
@requires_gpu
def test_spatial_transformer_wiring(monkeypatch):
    from modal_examples_amd.models.sdxl.layers import Conv3x3
    from modal_examples_amd.models.sdxl.unet import SpatialTransformer, UNetConfig

    cfg = UNetConfig.small()
    C = cfg.channels[1]  # 128: groups of 4
    m = _module(lambda: SpatialTransformer(C, 1, cfg.ctx_dim, cfg.head_dim), 28)
    conv = _module(lambda: Conv3x3(32, C), 29)
    z, ctx = _rand(2, 32, 16, 16, seed=30), _rand(2, 77, cfg.ctx_dim, seed=31)

    def fn():
        x, s = conv(z, gn_groups=32)
        return m(x, ctx, stats=s), s

    (on, s), (off, t) = _on_and_off(monkeypatch, fn)
    assert s is not None and t is None
    _close(on, off, **GN_TOL)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("which", ("small", "quads"))
def test_vae_decoder_wiring(monkeypatch, which):
    """VAEDecoderSmall has 1 and 2 channels per group, so every conv returns
    None and the plumbing alone is exercised; the 128-channel decoder passes
    statistics at every GroupNorm but mid_res2.norm1."""
    from modal_examples_amd.models.sdxl.vae import VAEDecoder, VAEDecoderSmall

    ctor = VAEDecoderSmall if which == "small" else (
        lambda: VAEDecoder(channels=(128, 128), resnets_per_level=1))
    m = _module(ctor, 32)
    z = _rand(1, 4, 8, 8, seed=33) * 0.13025
    on, off = _on_and_off(monkeypatch, lambda: m(z))
    assert torch.isfinite(on.float()).all()
    _close(on, off, **GN_TOL)


# ------------------------------------------------------- argument checks

@pytest.mark.gpu
@requires_gpu
def test_argument_checks():
    """Each bad call raises before any launch; a good call follows."""
    from modal_examples_amd.ops._build import get_ext

    ext = get_ext(required=True)
    c = _case(*_EXACT["interior"])  # K 64, G 16
    y, stats = _run(c, gn_groups=c.G)
    gamma, beta = torch.ones(c.K).cuda(), torch.zeros(c.K).cuda()
    wd = c.w.cuda()
    wr, bias = F.repack_conv3x3_weight(wd), c.bias.cuda()
    w2 = torch.zeros(64, c.K, 3, 3, dtype=torch.bfloat16, device="cuda")
    wr2 = F.repack_conv3x3_weight(w2)

    def consumers(x, groups, st):
        yield lambda: F.groupnorm_silu(x, gamma, beta, groups, stats=st)
        yield lambda: F.groupnorm_silu(x, gamma, beta, groups, out_nhwc=True,
                                       stats=st)
        yield lambda: F.conv3x3_gn(x, wr2, bias, 64, gamma, beta, groups=groups,
                                   raw_weight=w2, stats=st)

    bad = [
        (y, 8, stats),                           # taken for 16 groups
        (y, c.G, stats[:1].contiguous()),        # taken for one image
        (y, c.G, stats.reshape(-1)),             # not [N, G, 2]
        (y, c.G, stats.cpu()),                   # wrong device
        (y, c.G, stats.double()),                # wrong dtype
    ]
    for x, groups, st in bad:
        for call in consumers(x, groups, st):
            with pytest.raises(RuntimeError):
                call()
    # statistics together with groups of 10 channels
    n = _case(*_NO_STATS)
    yn = _run(n)
    g80, b80 = torch.ones(80).cuda(), torch.zeros(80).cuda()
    fake = torch.zeros(2, 8, 2, device="cuda")
    with pytest.raises(RuntimeError):
        F.groupnorm_silu(yn, g80, b80, 8, stats=fake)
    with pytest.raises(RuntimeError):
        F.groupnorm_silu(yn, g80, b80, 8, out_nhwc=True, stats=fake)
    # the producer: groups that do not divide K, or not into quads
    with pytest.raises(ValueError):
        _run(c, gn_groups=7)
    with pytest.raises(ValueError):
        _run(c, gn_groups=0)
    with pytest.raises(RuntimeError):
        ext.conv3x3_stats(c.x.cuda(), wr, bias, None, c.K, False, None, 32)
    with pytest.raises(RuntimeError):
        ext.conv3x3_stats(c.x.cuda(), wr, bias, None, c.K, False, None, 0)
    # statistics for a tensor that is not on the kernel path
    with pytest.raises(ValueError):
        F.groupnorm_silu(y.cpu(), gamma.cpu(), beta.cpu(), c.G, stats=stats)
    torch.cuda.synchronize()
    for call in consumers(y, c.G, stats):
        assert torch.isfinite(call().float()).all()
