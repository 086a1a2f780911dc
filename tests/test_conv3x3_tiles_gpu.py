"""conv3x3 on both of its tiles (8 and 16 output rows per block), and the
per-call choice between them.

The kernel's main loop reads every input fragment once per chunk and feeds it
to each tap that uses it, and the launcher picks the tile per call
(`conv3x3_tile_rule` in csrc/conv3x3.hip, `ext.conv3x3_tile` from Python).
What can go wrong: a patch row paired with the wrong tap or output row, a tile
seam or a padding row counted, a channel or output-channel tail, and a
statistics workspace sized for another tile than the one that wrote it.

Every case here is so small that the rule picks the 8-row tile; the same
cases run on the 16-row tile in one child process with MODAL_AMD_CONV_RPW=4
(read once per process).  Both assert which tile ran.

Exact cases are the construction of tests/test_kernel_edges_gpu.py: x in
[-2, 2], w in {-1, 0, 1} (80/C of them non-zero past C = 80), bias, residual
and addend in [-8, 8].  Every product and partial sum is an integer far below
2^24 and every result an integer of magnitude at most 256, a bf16 value, so
the order of the f32 sums does not matter: torch.equal against float64.
tests/test_conv3x3_tile_rule.py checks those conditions without a GPU.
"""
import functools
import os
from types import SimpleNamespace

import pytest
import torch

import modal_examples_amd.ops.functional as F

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

GN_TOL = dict(atol=2e-2, rtol=2e-2, frac=0.999)  # tests/test_sdxl_glue_gpu.py

_VARIANTS = ("plain", "residual", "addend", "upsample")


def gpu_test(fn):
    return pytest.mark.gpu(requires_gpu(fn))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _up2(t):
    return torch.nn.functional.interpolate(t, scale_factor=2.0, mode="nearest")


@functools.lru_cache(maxsize=None)
def _case(N, C, K, H, W, variant="plain"):
    """Integer operands (CPU) and the float64 reference.  H, W are the
    source's; the output is twice that with upsample."""
    g = _gen(((((N * 401 + C) * 401 + K) * 401 + H) * 401 + W) * 4
             + _VARIANTS.index(variant))
    up = variant == "upsample"
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).to(torch.bfloat16)
    w = torch.randint(-1, 2, (K, C, 3, 3), generator=g).float()
    if C > 80:
        w *= torch.rand(K, C, 3, 3, generator=g) < 80.0 / C
    w = w.to(torch.bfloat16)
    bias = torch.randint(-8, 9, (K,), generator=g).float()
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    res = (torch.randint(-8, 9, (N, K, Ho, Wo), generator=g).to(torch.bfloat16)
           if variant == "residual" else None)
    add = (torch.randint(-8, 9, (N, K), generator=g).to(torch.bfloat16)
           if variant == "addend" else None)
    xin = _up2(x.double()) if up else x.double()
    want = torch.nn.functional.conv2d(xin, w.double(), bias.double(), padding=1)
    if res is not None:
        want = want + res.double()
    if add is not None:
        want = want + add.double()[:, :, None, None]
    return SimpleNamespace(x=x, w=w, bias=bias, res=res, add=add, K=K, C=C,
                           upsample=up, want=want)


# all padding but one row, one short of, at and one past either tile, two
# tiles of the 16-row one and one row more; W one short of, at and one past
# the tile's 32 columns
SPATIAL = [(1, 16, 8, H, W) for H in (1, 15, 16, 17, 32, 33)
           for W in (31, 32, 33)]
C_TAILS = [(2, C, 8, 9, 33) for C in (1, 17, 80)]  # one, two and five chunks
K_TAILS = [(1, 16, K, 9, 33) for K in (64, 65)]    # a full tile; one k more
FUSED = [(2, 24, 40, 5, 17, "upsample"),           # odd source
         (2, 17, 65, 9, 33, "residual"),
         (2, 17, 65, 9, 33, "addend")]
# statistics: a seam of both tiles in H, a second tile column of one pixel
STATS = (1, 16, 64, 17, 33)
STATS_G = 16
EXACT = SPATIAL + C_TAILS + K_TAILS + FUSED


def _ext():
    from modal_examples_amd.ops._build import get_ext

    return get_ext(required=True)


def _tile_of(case):
    c = _case(*case)
    N, _, Ho, Wo = c.want.shape
    return _ext().conv3x3_tile(N, c.C, Ho, Wo, c.K, c.upsample)[0]


def _run(case, gn_groups=None):
    c = _case(*case)
    wd = c.w.cuda()
    return F.conv3x3(c.x.cuda(), F.repack_conv3x3_weight(wd), c.bias.cuda(),
                     c.K, residual=None if c.res is None else c.res.cuda(),
                     raw_weight=wd, upsample=c.upsample,
                     addend=None if c.add is None else c.add.cuda(),
                     gn_groups=gn_groups)


def _exact(got, want64, what):
    g = got.detach().double().cpu()
    assert g.shape == want64.shape, (what, g.shape, want64.shape)
    if torch.equal(g, want64):
        return
    diff = g != want64  # true for NaN as well
    at = diff.nonzero()[0].tolist()
    raise AssertionError(
        f"{what}: {int(diff.sum())} of {diff.numel()} elements differ, first "
        f"at {at}: got {float(g[tuple(at)])}, want {float(want64[tuple(at)])}")


def _check(case, rpw):
    assert _tile_of(case) == rpw, (case, _tile_of(case))
    _exact(_run(case), _case(*case).want, f"conv3x3{case} at {rpw} rows/wave")


def _sums(y, G):
    """float64 (sum, sumsq) per (n, group) of a stored tensor: [N, G, 2]."""
    v = y.detach().float().double().cpu()
    v = v.reshape(v.shape[0], G, -1)
    return torch.stack((v.sum(-1), (v * v).sum(-1)), dim=-1)


def _check_stats(rpw):
    assert _tile_of(STATS) == rpw
    y, stats = _run(STATS, gn_groups=STATS_G)
    assert stats is not None and tuple(stats.shape) == (STATS[0], STATS_G, 2)
    _exact(y, _case(*STATS).want, f"conv3x3{STATS} with statistics")
    _exact(stats, _sums(y, STATS_G), f"statistics of conv3x3{STATS}")


@gpu_test
@pytest.mark.parametrize("case", SPATIAL, ids=str)
def test_spatial_edges(case):
    _check(case, 2)


@gpu_test
@pytest.mark.parametrize("case", C_TAILS, ids=str)
def test_channel_tails(case):
    _check(case, 2)


@gpu_test
@pytest.mark.parametrize("case", K_TAILS, ids=str)
def test_output_channel_tails(case):
    _check(case, 2)


@gpu_test
@pytest.mark.parametrize("case", FUSED, ids=str)
def test_fused_variants(case):
    _check(case, 2)


@gpu_test
def test_statistics():
    _check_stats(2)


def _forced_main():
    """The child of test_all_cases_on_the_other_tile."""
    rpw = int(os.environ["MODAL_AMD_CONV_RPW"])
    torch.cuda.init()
    for case in EXACT:
        _check(case, rpw)
    _check_stats(rpw)
    torch.cuda.synchronize()
    print(f"{len(EXACT) + 1} cases at MODAL_AMD_CONV_RPW={rpw}")


@gpu_test
def test_all_cases_on_the_other_tile():
    """The rule gives every case above the 8-row tile; one fresh child runs
    them all on the 16-row tile.  The limit is far above the few seconds the
    child takes with its start, so that only a hang reaches it."""
    import subprocess
    import sys

    tests_dir = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MODAL_AMD_CONV_RPW="4")
    code = ("import sys; sys.path[:0] = [%r, %r]; "
            "import test_conv3x3_tiles_gpu as t; t._forced_main()"
            % (os.path.dirname(tests_dir), tests_dir))
    r = subprocess.run([sys.executable, "-c", code], env=env, timeout=120.0,
                       capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (f"child exited with {r.returncode}\n"
                               f"{r.stdout[-4000:]}\n{r.stderr[-8000:]}")
    assert f"{len(EXACT) + 1} cases at MODAL_AMD_CONV_RPW=4" in r.stdout


# ---- dispatch: one shape on each side of the rule's block count.  The
# smallest that reaches it: 1024 blocks of 16 x 32 pixels x 64 channels.
# (N, C, K, H, W, rows per wave the rule gives)
DISPATCH = [(1, 128, 512, 64, 1024, 4),   # 32 * 4 * 8 = 1024 blocks
            (1, 128, 512, 32, 1024, 2)]   # 512


@gpu_test
@pytest.mark.parametrize("spec", DISPATCH, ids=str)
def test_tile_rule_and_statistics_workspace_agree(spec):
    """The partials the conv wrote have the dims that conv3x3_tile reports
    for the call's shape, the tile is the one the rule gives on that side,
    and GroupNorm+SiLU from those statistics is that of the statistics pass
    within the GroupNorm tolerance."""
    N, C, K, H, W, rpw = spec
    G = 32
    ext = _ext()
    g = torch.Generator(device="cuda").manual_seed(N * 7 + H)
    x = torch.randn(N, C, H, W, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(K, C, 3, 3, device="cuda", generator=g)
         / (3 * C ** 0.5)).to(torch.bfloat16)
    bias = torch.randn(K, device="cuda", generator=g)
    gamma = torch.rand(K, device="cuda", generator=g) + 0.5
    beta = torch.randn(K, device="cuda", generator=g)
    tile = ext.conv3x3_tile(N, C, H, W, K)
    assert tile[0] == rpw, tile
    assert tile == ext.conv3x3_tile(N, C, H, W, K, rule_only=True)
    wr = F.repack_conv3x3_weight(w)
    y, sums, part = ext.conv3x3_stats_partials(x, wr, bias, None, K, False,
                                               None, G)
    assert tuple(part.shape) == (N, tile[1], tile[2], 2), (part.shape, tile)
    assert tile[1] == (W // 32) * (H // (4 * rpw)) and tile[2] == K // 4
    y2, sums2 = F.conv3x3(x, wr, bias, K, raw_weight=w, gn_groups=G)
    assert torch.equal(y, y2) and torch.equal(sums, sums2)
    got = F.groupnorm_silu(y, gamma, beta, G, stats=sums).float()
    want = F.groupnorm_silu(y, gamma, beta, G).float()
    ok = (got - want).abs() <= GN_TOL["atol"] + GN_TOL["rtol"] * want.abs()
    frac = float(ok.float().mean())
    print(f"{spec}: tile {tile}, max |diff| "
          f"{float((got - want).abs().max()):.3e}, within bound {frac:.6f}")
    assert torch.isfinite(got).all()
    assert frac >= GN_TOL["frac"]
