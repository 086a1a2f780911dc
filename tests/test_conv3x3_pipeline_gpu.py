"""conv3x3: the software-pipelined staging and the batched epilogue.

The kernel loads every staged input element unconditionally from a clamped
address and zero-fills by a mask when it writes the LDS patch; its epilogue
loads the residual unconditionally (clamped on edge tiles) and masks only the
stores.  What can go wrong is therefore a clamped value that leaks (a border
pixel repeated into the padding, channel C-1 repeated into the channel tail,
a neighbouring pixel's residual), a chunk that is staged one iteration early
or late, and an edge tile taking the interior path or the reverse.

Every exact case uses integer operands: x, w and the residual in [-2, 2], the
bias in [-4, 4].  All products and all f32 partial sums are then integers
below 2^24 (asserted on the CPU), the order of the MFMA sums does not matter,
and the only rounding is the final one to bf16.  The reference is
F.conv2d in float64 on the CPU plus bias plus residual, rounded once to bf16;
the comparison is torch.equal.

GPU tests carry `pytest.mark.gpu` and the `requires_gpu` skip, one by one.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import modal_examples_amd.ops.functional as F

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

CONV_TOL = (5e-2, 5e-2)  # atol, rtol of the fused GroupNorm conv (bf16 MFMA)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _up2(t):
    return torch.nn.functional.interpolate(t, scale_factor=2.0, mode="nearest")


def _reference(x, w, bias, res, upsample):
    """float64 on the CPU, rounded once to bf16; |values| < 2^24 before."""
    xin = _up2(x.double()) if upsample else x.double()
    want = torch.nn.functional.conv2d(xin, w.double(), bias.double(), padding=1)
    if res is not None:
        want = want + res.double()
    assert float(want.abs().max()) < 2.0 ** 24, "partial sums must stay exact"
    assert torch.equal(want, want.round()), "integer operands, integer sums"
    return want.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _case(N, C, K, H, W, upsample=False, residual=False):
    """Integer operands (CPU) and their reference; H, W are the source's."""
    g = _gen(((((N * 211 + C) * 211 + K) * 211 + H) * 211 + W) * 4
             + 2 * upsample + residual)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).to(torch.bfloat16)
    w = torch.randint(-2, 3, (K, C, 3, 3), generator=g).to(torch.bfloat16)
    bias = torch.randint(-4, 5, (K,), generator=g).float()
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    res = (torch.randint(-2, 3, (N, K, Ho, Wo), generator=g).to(torch.bfloat16)
           if residual else None)
    return SimpleNamespace(x=x, w=w, bias=bias, res=res, K=K, upsample=upsample,
                           want=_reference(x, w, bias, res, upsample))


def _run(c, x=None, res=None, wr=None):
    wd = c.w.cuda()
    if res is None and c.res is not None:
        res = c.res.cuda()
    return F.conv3x3(c.x.cuda() if x is None else x,
                     F.repack_conv3x3_weight(wd) if wr is None else wr,
                     c.bias.cuda(), c.K, residual=res, raw_weight=wd,
                     upsample=c.upsample)


def _exact(got, want, what):
    g, w = got.detach().cpu(), want.detach().cpu()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if torch.equal(g, w):
        return
    diff = g != w  # true for NaN as well
    n, k, y, x = diff.nonzero()[0].tolist()
    raise AssertionError(
        f"{what}: {int(diff.sum())} of {diff.numel()} elements differ, first "
        f"at (n={n}, k={k}, y={y}, x={x}): got {float(g[n, k, y, x])}, want "
        f"{float(w[n, k, y, x])}")


# ------------------------------------------------------------ pipeline depth

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("C", (4, 16, 17, 40, 48))
def test_pipeline_depth(C):
    """1, 1, 2, 3, 3 chunks: no prefetch at all, a prefetch whose last chunk
    holds one channel, middle iterations, and channel tails of 4 (less than
    an octet), 1 and 8 in the last chunk.  One interior tile per image."""
    c = _case(2, C, 64, 8, 32)
    _exact(_run(c), c.want, f"C={C}")


# ------------------------------------- tile edges and the epilogue's two paths

_HW = ((8, 32), (9, 33), (7, 40), (16, 24), (1, 1), (8, 31))


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("residual", (False, True), ids=("plain", "residual"))
@pytest.mark.parametrize("K", (3, 64, 65))
@pytest.mark.parametrize("HW", _HW, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_tile_edges_and_epilogue_split(HW, K, residual):
    """(8, 32) with K = 64 is the interior path alone; every other
    combination has edge tiles in y, in x or in k, (9, 33) and K = 65 have
    both kinds side by side.  C = 20 adds a channel tail; two images show a
    wrong batch stride."""
    c = _case(2, 20, K, HW[0], HW[1], False, residual)
    _exact(_run(c), c.want, f"{HW} K={K} residual={residual}")


# ------------------------------------------------- clamped addresses must not leak

@functools.lru_cache(maxsize=None)
def _leak_case(H, W):
    """Border rows, border columns and the last channel hold 256, the interior
    [-2, 2]; every weight is 1 or 2, so nothing cancels: a border pixel
    repeated into the padding adds at least 256 to an output.  The residual's
    last row, last column and last channel hold 256 as well, against a
    clamped residual load that reaches a stored element."""
    N, C, K = 2, 20, 64
    g = _gen(977 * H + W)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).float()
    x[:, :, 0, :] = x[:, :, -1, :] = 256.0
    x[:, :, :, 0] = x[:, :, :, -1] = 256.0
    x[:, -1] = 256.0
    w = torch.randint(1, 3, (K, C, 3, 3), generator=g).to(torch.bfloat16)
    bias = torch.randint(-4, 5, (K,), generator=g).float()
    res = torch.randint(-2, 3, (N, K, H, W), generator=g).float()
    res[:, :, -1, :] = res[:, :, :, -1] = 256.0
    res[:, -1] = 256.0
    x, res = x.to(torch.bfloat16), res.to(torch.bfloat16)
    return SimpleNamespace(x=x, w=w, bias=bias, res=res, K=K, upsample=False,
                           C=C, want=_reference(x, w, bias, res, False))


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("HW", ((8, 32), (9, 33)), ids=("8x32", "9x33"))
def test_clamped_addresses_do_not_leak(HW):
    """The packed weights of the 12 padded channels are set to 1 here (the
    repack leaves them 0): channel C-1, which the clamped loads of the tail
    re-read, is 256 everywhere, so an unmasked tail changes every output."""
    c = _leak_case(*HW)
    wr = F.repack_conv3x3_weight(c.w.cuda())
    wr[:, :, c.C:] = 1.0
    _exact(_run(c, wr=wr), c.want, f"leak {HW}")


# ------------------------------------------------------------------ alignment

def _carve(t, offset):
    """A contiguous copy of t that starts `offset` elements into its storage:
    the data pointer is then only 2-byte aligned."""
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=t.device)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == offset
    return v


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("offset", (1, 3))
def test_two_byte_aligned_pointers(offset):
    c = _case(2, 20, 64, 8, 32, False, True)
    aligned = _run(c)
    got = _run(c, x=_carve(c.x.cuda(), offset), res=_carve(c.res.cuda(), offset))
    _exact(got, aligned, f"storage offset {offset} against the aligned call")
    _exact(got, c.want, f"storage offset {offset}")


# ------------------------------------------------------------------- upsample

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("src", ((5, 5), (8, 16)), ids=("5x5", "8x16"))
def test_upsample_with_residual(src):
    """10 x 10 (one edge tile, clamped rows and columns map to source row and
    column 4) and 16 x 32 (two interior tiles) outputs."""
    c = _case(2, 20, 64, src[0], src[1], True, True)
    _exact(_run(c), c.want, f"upsample from {src}")


# ------------------------------------------------------------------ conv3x3_gn

@functools.lru_cache(maxsize=None)
def _gn_case():
    """2 x 32 -> 64 at 9 x 33, 8 groups.  beta = 3 and weights of one sign:
    padding applied before the activation would put silu(3) = 2.86 on every
    out-of-image tap, which moves a corner output by 5/9 of that."""
    N, C, K, H, W, G = 2, 32, 64, 9, 33, 8
    g = _gen(4242)
    x = torch.randn(N, C, H, W, generator=g).to(torch.bfloat16)
    w = (torch.rand(K, C, 3, 3, generator=g) / C).to(torch.bfloat16)
    bias = torch.randn(K, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.full((C,), 3.0)
    # the op's own reference path (CPU tensors take it)
    want = F.conv3x3_gn(x, None, bias, K, gamma, beta, groups=G, raw_weight=w)
    # the wrong model: zero padding before GroupNorm+SiLU's shift
    h = torch.nn.functional.silu(torch.nn.functional.group_norm(
        x.float(), G, gamma, beta, 1e-5))
    hp = torch.nn.functional.pad(h, (1, 1, 1, 1), value=float(
        torch.nn.functional.silu(torch.tensor(3.0))))
    wrong = torch.nn.functional.conv2d(hp, w.float(), bias)
    return SimpleNamespace(x=x, w=w, bias=bias, gamma=gamma, beta=beta, K=K,
                           groups=G, want=want, wrong=wrong)


def _ratio(got, want, atol, rtol):
    got, want = got.double().cpu(), want.double().cpu()
    return (got - want).abs() / (atol + rtol * want.abs())


@pytest.mark.gpu
@requires_gpu
def test_conv3x3_gn_border_taps_contribute_zero():
    c = _gn_case()
    wd = c.w.cuda()
    got = F.conv3x3_gn(c.x.cuda(), F.repack_conv3x3_weight(wd), c.bias.cuda(),
                       c.K, c.gamma.cuda(), c.beta.cuda(), groups=c.groups,
                       raw_weight=wd)
    assert torch.isfinite(got.float()).all()
    worst = float(_ratio(got, c.want, *CONV_TOL).max())
    print(f"conv3x3_gn 9x33: worst error {worst:.4f} of the bound")
    assert worst <= 1.0
    # the case tells the two paddings apart: on the border the wrong model is
    # many bounds away from the reference, so the kernel cannot match both
    border = torch.ones(9, 33, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    sep = _ratio(c.wrong, c.want, *CONV_TOL)[:, :, border]
    assert float(sep.min()) > 2.0, float(sep.min())
