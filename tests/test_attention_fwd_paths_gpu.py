"""The paths of the attention forward (csrc/attention_fwd32.hip) that the
shape tables of test_attention_forward.py do not reach: the wave-uniform
interior-tile decision, the read-ahead of K and V fragments across the
barrier pair, and scales of every kind (large, small, negative, zero: at
scale 0 the result is the plain average of the visible V rows).

Cases, judge and rules are those of test_attention_forward.py (bitwise where
the case is exact, otherwise max|o - o64| <= 2 * e_y + 2**-8 * max|o64| and
|lse - lse64| <= 1e-3 on every element and row); every forward entry must
agree bit for bit and so must a second call.

Scales -0.25 and 0.0 go through the same judge: its yardstick
(reference.attention_fwd_ref) multiplies the scores by whatever scale it is
given, and on the CPU `judge` accepts the rounded fp64 truth of those cases
with e_y > 0 (at scale 0 every P is exactly 1 and e_y is the rounding of the
output alone), so no other reference is needed.  test_attention_fwd_paths.py
holds that check, on the shapes and scales of this file.

count_case asserts Sk <= 256; the Sk = 448 shape takes the same construction
through `_count_wide` below (log(n + 1) - log(n) > 2e-3 up to n = 448, still
twice the 1e-3 LSE bound, so the count stays told apart from its neighbours).
For that it borrows `_finish` and `_gen`, private helpers of
test_attention_forward.py: a change to either there has to be followed here.
"""
import math

import pytest
import torch

import modal_examples_amd.ops.functional as F
from test_attention_forward import (
    B, BF, DS, _finish, _gen, bshd_views, count_case, judge, ramp_case,
    random_case, selector_case, shape_id, visible_counts)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# (Hq, Hkv, Sq, Sk, causal); tiles: q block 128 = 4 waves x 32 rows, KV block
# 64 at D=64 and 32 at D=128
PATH_SHAPES = [
    # causal_off = 47: a KV tile is full for the last rows of a wave and not
    # for its first, at both KV blocks (the wave-uniform decision)
    (2, 2, 100, 147, True),
    # 7 / 14 tiles of distinct data, two live waves: read-ahead across the
    # barrier pair
    (2, 1, 64, 448, False),
    # only the fast path, and the fast path plus a one-key edge tile
    (2, 2, 128, 64, False),
    (2, 2, 128, 65, False),
    # the diagonal inside the first wave, a second wave with one live row
    (2, 2, 33, 192, True),
]
SCALES = (None, 0.3, 2.0, -0.25, 0.0)


def _count_wide(Hq, Hkv, Sq, Sk, causal, D, seed=1):
    """count_case past its Sk <= 256: q = 0, lse = log(n_i), o the mean of
    the visible V rows."""
    assert Sk < 500
    g = _gen(seed)
    q = torch.zeros(B, Hq, Sq, D).to(BF)
    k = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    n = visible_counts(Sq, Sk, causal).double()
    c = _finish("count", q, k, v, causal, 1.0 / math.sqrt(D),
                lse_expect=torch.log(n).expand(B, Hq, Sq))
    assert (c["lse64"] - c["lse_expect"]).abs().max() < 1e-12
    return c


def _count(shape, D):
    return (count_case if shape[3] <= 256 else _count_wide)(*shape, D)


def _ext():
    from modal_examples_amd.ops._build import get_ext

    return get_ext(required=True)


def _check(c, shape, D, extra=""):
    """Case c through every forward entry, contiguous and strided, twice;
    all outputs bit-equal, then the judge."""
    label = f"{c['name']}{extra} {shape_id(shape)} D{D}"
    ext = _ext()
    causal, scale = c["causal"], c["scale"]
    q, k, v = (c[n].cuda() for n in "qkv")
    qs, ks, vs = bshd_views(c, "cuda")
    qt, kt, vt = (t.transpose(1, 2) for t in (qs, ks, vs))
    assert torch.equal(qt, q) and torch.equal(kt, k) and torch.equal(vt, v)
    o, lse = ext.attention_fwd_lse(q, k, v, causal, scale)
    assert o.dtype is BF and o.shape == q.shape
    assert lse.dtype is torch.float32 and lse.shape == q.shape[:3]
    o_qkv = F.attention_qkv(qs, ks, vs, causal=causal, scale=scale)
    same_o = {
        "attention": ext.attention(q, k, v, causal, scale),
        "attention_bshd": ext.attention_bshd(qt, kt, vt, causal,
                                             scale).transpose(1, 2),
        "F.attention": F.attention(q, k, v, causal=causal, scale=scale),
        "F.attention_qkv": o_qkv.reshape(B, shape[2], shape[0],
                                         D).transpose(1, 2),
    }
    for rerun in (ext.attention_fwd_lse(q, k, v, causal, scale),
                  ext.attention_fwd_lse_bshd(qt, kt, vt, causal, scale)):
        o2, lse2 = rerun
        if o2.shape != o.shape:
            o2 = o2.transpose(1, 2)
        same_o[f"fwd_lse call {len(same_o)}"] = o2
        assert torch.equal(lse2, lse), f"{label}: lse differs between calls"
    for name, other in same_o.items():
        assert torch.equal(other, o), f"{label}: {name} differs"
    judge(c, o, lse, label)


@requires_gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"scale{s}")
@pytest.mark.parametrize("shape", PATH_SHAPES, ids=shape_id)
def test_random_at_every_kind_of_scale(shape, scale, D):
    c = random_case(*shape, D, scale)
    assert c["e_y"] > 0
    _check(c, shape, D, f" scale={scale}")


@requires_gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("growth", (12.0, -12.0))
@pytest.mark.parametrize("shape", PATH_SHAPES, ids=shape_id)
def test_ramp_rescales_on_every_tile_or_never(shape, growth, D):
    _check(ramp_case(*shape, D, growth), shape, D)


@requires_gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", PATH_SHAPES, ids=shape_id)
def test_count_of_visible_keys(shape, D):
    _check(_count(shape, D), shape, D)


@requires_gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", PATH_SHAPES, ids=shape_id)
def test_selector_is_bitwise_the_gathered_rows(shape, D):
    _check(selector_case(*shape, D), shape, D)
