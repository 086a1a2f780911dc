"""The conv3x3 tile rule (csrc/conv3x3.hip, conv3x3_tile_rule) without a GPU:
it is a pure function of the call's shape, it sizes the statistics workspace
for the tile it names, and it gives the shapes of PERF.md's table the tile
that was faster there.  Also the conditions under which the exact cases of
tests/test_conv3x3_tiles_gpu.py are exact."""
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_conv3x3_tiles_gpu as T  # noqa: E402


def _ext():
    from modal_examples_amd.ops._build import get_ext

    return get_ext(required=True)


def _rule(*shape, **kw):
    return _ext().conv3x3_tile(*shape, rule_only=True, **kw)


_GRID = list(itertools.product((1, 4, 32), (4, 127, 128, 1280),
                               (1, 17, 32, 120, 128, 1024), (33, 1024),
                               (3, 64, 512)))  # N, C, H, W, K


def test_rule_is_a_pure_function_of_the_shape():
    """Same arguments, same answer: whatever was asked before, in whatever
    order, and whatever tile the process is forced to for its launches."""
    first = {s: _rule(*s) for s in _GRID}
    for s in reversed(_GRID):
        assert _rule(*s) == first[s], s
    forced = os.environ.get("MODAL_AMD_CONV_RPW")
    for s in _GRID[::7]:
        _ext().conv3x3_tile(*s)  # the process's choice, override included
        assert _rule(*s) == first[s], (s, forced)
    for s, (rpw, npix, nquads) in first.items():
        N, C, H, W, K = s
        assert rpw in (2, 4), s
        rows = 4 * rpw
        assert npix == -(-W // 32) * -(-H // rows), s
        assert nquads == -(-K // 64) * 16, s
        assert _rule(*s, gn=True)[0] == 2, s
        assert _rule(*s, upsample=True) == first[s], s


def test_rule_on_the_measured_shapes():
    """PERF.md's per-shape table (B = 4): 16 rows where that was faster."""
    want = {(4, 128, 1024, 1024, 128): 4, (4, 256, 512, 512, 256): 4,
            (4, 512, 256, 256, 512): 4, (4, 512, 128, 128, 512): 4,
            (4, 512, 512, 512, 256): 4, (4, 320, 128, 128, 320): 2,
            (4, 640, 64, 64, 640): 2, (4, 1280, 32, 32, 1280): 2,
            (4, 4, 128, 128, 512): 2}
    for s, rpw in want.items():
        assert _rule(*s)[0] == rpw, s
    assert _rule(4, 256, 1024, 1024, 256, upsample=True)[0] == 4
    assert _rule(4, 512, 256, 256, 512, upsample=True)[0] == 4


def test_more_images_never_take_the_tile_back():
    for C, H, W, K in ((128, 32, 32, 64), (512, 64, 64, 512), (320, 17, 40, 64)):
        seen4 = False
        for N in (1, 2, 8, 64, 512, 4096):
            rpw = _rule(N, C, H, W, K)[0]
            assert not (seen4 and rpw == 2), (N, C, H, W, K)
            seen4 = seen4 or rpw == 4


def test_exact_cases_are_exact_in_bf16():
    """Every reference value of the GPU file's exact cases is an integer of
    magnitude at most 256, hence a bf16 value; the statistics case's sums of
    |y| and of y^2 per group, and so every partial sum, are below 2^24."""
    for case in T.EXACT + [T.STATS]:
        want = T._case(*case).want
        assert torch.equal(want, want.round()), case
        assert float(want.abs().max()) <= 256, case
    want = T._case(*T.STATS).want
    s = T._sums(want, T.STATS_G)
    absum = want.abs().reshape(want.shape[0], T.STATS_G, -1).sum(-1)
    top = max(float(absum.max()), float(s[..., 1].max()))
    print(f"statistics case: largest group sum of |y| or y^2 {top:.0f}")
    assert top < 2.0 ** 24
