"""GPU tier of the strict attention-forward tests: csrc/attention_fwd32.hip
through every entry (ext.attention, attention_bshd, attention_fwd_lse[_bshd],
F.attention, F.attention_qkv) on the cases of test_attention_forward.py,
judged by its `judge` — bitwise where the case is exact, otherwise

    max|o - o64| <= 2 * e_y + 2**-8 * max|o64|,   |lse - lse64| <= 1e-3

on every element and row.  Run with -s for the ATTN_FWD_RATIO / ATTN_FWD_LSE
figures.  Measured on an MI355X, worst case per family:

    family              err / e_y   max err    LSE err
    selector            0 (bitwise) 0          1.2e-7
    count               1.000       7.8e-3     6.6e-7
    ramp +3             1.757       9.1e-3     5.0e-6
    ramp +12            1.597       1.2e-2     3.0e-5
    ramp -3 / -12       1.000       9.1e-3     4.2e-6
    random              1.499       7.6e-3     8.9e-7
    random, scale 0.3   2.404       1.9e-2     2.8e-6
    hidden rows         1.000       7.8e-3     7.7e-7

A ratio of 1.000 is the rounding of the output alone.  The ratios above it
come from P: the yardstick rounds exp(s - rowmax), whose largest term is
exactly 1, the kernel rounds exp(s - m_run) with m_run a deferred (stale)
max, so its largest term carries a rounding too.  At scale 0.3 one or two
keys carry a row and that term is the error; the case stays inside the rule
through the 2**-8 * max|o64| term (bound 2.8e-2).
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import modal_examples_amd.ops.functional as F
from test_attention_forward import (
    BF, DS, GROWTHS, HIDDEN_SHAPES, SHAPES, WIDE_SHAPES, bshd_views,
    count_case, judge, ramp_case, random_case, selector_case, shape_id)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

NODEFER = "MODAL_AMD_FA_NODEFER"
# Measured on an MI355X: this whole file, child included, takes 10 s from a
# cold process start (7 s of it inside pytest); the child alone, which runs
# 94 of its tests, 4 s.  The child gets three times the whole file's time.
CHILD_S = 10
FATAL_EXITS = (134, 139, 124, 137)


def _ext():
    from modal_examples_amd.ops._build import get_ext

    return get_ext(required=True)


def _forward_all(c, label):
    """Case c through every forward entry.  All of them must agree bit for
    bit, and so must a second call; returns (o [B,Hq,Sq,D], lse)."""
    ext = _ext()
    causal, scale = c["causal"], c["scale"]
    q, k, v = (c[n].cuda() for n in "qkv")
    o = ext.attention(q, k, v, causal, scale)
    o_l, lse = ext.attention_fwd_lse(q, k, v, causal, scale)
    assert o.dtype is BF and o.shape == q.shape and o.is_contiguous()
    assert lse.dtype is torch.float32 and lse.shape == q.shape[:3]
    assert torch.equal(o_l, o), f"{label}: attention_fwd_lse o != attention"
    # the same data as strided sequence-major views
    qs, ks, vs = bshd_views(c, "cuda")
    assert not (ks.is_contiguous() or vs.is_contiguous())
    qt, kt, vt = (t.transpose(1, 2) for t in (qs, ks, vs))
    assert torch.equal(qt, q) and torch.equal(kt, k) and torch.equal(vt, v)
    o_b = ext.attention_bshd(qt, kt, vt, causal, scale)
    o_bl, lse_b = ext.attention_fwd_lse_bshd(qt, kt, vt, causal, scale)
    assert o_b.shape == qs.shape and o_b.is_contiguous()
    assert torch.equal(o_b.transpose(1, 2), o), f"{label}: bshd o differs"
    assert torch.equal(o_bl, o_b), f"{label}: fwd_lse_bshd o differs"
    assert torch.equal(lse_b, lse), f"{label}: bshd lse differs"
    # the public API on top of them
    assert torch.equal(F.attention(q, k, v, causal=causal, scale=scale), o)
    o_qkv = F.attention_qkv(qs, ks, vs, causal=causal, scale=scale)
    assert torch.equal(o_qkv, o_b.reshape(o_qkv.shape)), (
        f"{label}: attention_qkv differs")
    # twice the same bits
    o2, lse2 = ext.attention_fwd_lse(q, k, v, causal, scale)
    assert torch.equal(o2, o) and torch.equal(lse2, lse), (
        f"{label}: two calls differ")
    return o, lse


def _run(c, shape, D, extra=""):
    label = f"{c['name']}{extra} {shape_id(shape)} D{D}"
    o, lse = _forward_all(c, label)
    judge(c, o, lse, label)


# -------------------------------------------------------- 1. selector, bitwise

@requires_gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_selector_is_bitwise_the_gathered_rows(shape, D):
    _run(selector_case(*shape, D), shape, D)


# -------------------------------------------------------------------- 2. count

@requires_gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_count_of_visible_keys(shape, D):
    _run(count_case(*shape, D), shape, D)


# ---------------------------------------------------------- 3. ramp and random

@requires_gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("growth", GROWTHS)
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=shape_id)
def test_ramp_through_the_rescale_schedules(shape, growth, D):
    _run(ramp_case(*shape, D, growth), shape, D)


@requires_gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", [(3, 3, 160, 77, False),
                                   (2, 2, 31, 65, False),
                                   (2, 2, 1, 33, True)], ids=shape_id)
def test_ramp_minus12_on_ragged_tails(shape, D):
    _run(ramp_case(*shape, D, -12.0), shape, D)


@requires_gpu
@pytest.mark.parametrize("scale", [None, 0.3])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=shape_id)
def test_random_under_the_yardstick(shape, D, scale):
    _run(random_case(*shape, D, scale), shape, D,
         "" if scale is None else f" scale={scale}")


# ------------------------------------------------------------ 5. stray writes

@requires_gpu
@pytest.mark.parametrize("bshd", [False, True], ids=["bhsd", "bshd"])
@pytest.mark.parametrize("Sq,Sk", [(1, 33), (129, 129)])
@pytest.mark.parametrize("D", DS)
def test_fwd_no_stray_writes(D, Sq, Sk, bshd):
    """o and lse in caller's buffers (out= / lse=): 8 sentinel rows after
    every (b, h) block of o — where rows Sq.. of the last q block would land —
    and guard bands around both buffers stay untouched."""
    from modal_examples_amd.gpu.guard import GuardBand

    ext = _ext()
    c = random_case(2, 2, Sq, Sk, True, D)
    Bn, H, PAD = 2, 2, 8
    if bshd:
        band = GuardBand((Bn, Sq + PAD, H, D), BF, "cuda", pad_bytes=1 << 16)
        out, spare = band.tensor[:, :Sq], band.tensor[:, Sq:]
        q, k, v = (t.transpose(1, 2) for t in bshd_views(c, "cuda"))
        fn = ext.attention_fwd_lse_bshd
    else:
        band = GuardBand((Bn, H, Sq + PAD, D), BF, "cuda", pad_bytes=1 << 16)
        out, spare = band.tensor[:, :, :Sq], band.tensor[:, :, Sq:]
        q, k, v = (c[n].cuda() for n in "qkv")
        fn = ext.attention_fwd_lse
    lband = GuardBand((Bn, H, Sq), torch.float32, "cuda", pad_bytes=4096)
    assert not out.is_contiguous() or Bn * H == 1
    o, lse = fn(q, k, v, True, c["scale"], out=out, lse=lband.tensor)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr() and o.stride() == out.stride()
    assert lse.data_ptr() == lband.tensor.data_ptr()
    band.check()
    lband.check()
    sentinel = spare.contiguous().view(torch.uint8)
    assert bool((sentinel == 0xAB).all()), (
        f"{int((sentinel != 0xAB).sum())} bytes written past row Sq")
    label = f"guarded {'bshd' if bshd else 'bhsd'} Sq{Sq} Sk{Sk} D{D}"
    judge(c, o.transpose(1, 2) if bshd else o, lse, label)
    o_ref, lse_ref = ext.attention_fwd_lse(*(c[n].cuda() for n in "qkv"),
                                           True, c["scale"])
    assert torch.equal(o.transpose(1, 2) if bshd else o, o_ref)
    assert torch.equal(lse, lse_ref)
    # a buffer of another shape or dtype is refused on the host
    with pytest.raises(RuntimeError, match="out must be"):
        fn(q, k, v, True, c["scale"], out=band.tensor)
    with pytest.raises(RuntimeError, match="lse must be"):
        fn(q, k, v, True, c["scale"], lse=lband.tensor.double())
    torch.cuda.synchronize()


# ------------------------------------------------------ 6. rows that see no key

@requires_gpu
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", HIDDEN_SHAPES, ids=shape_id)
def test_hidden_rows_are_zero_and_minus_inf(shape, D):
    for c in (random_case(*shape, D), count_case(*shape, D)):
        assert c["hidden"].sum() == shape[2] - shape[3]
        _run(c, shape, D)


# ------------------------------------------------ 7. empty and bad arguments

def _valid_small_call():
    shape = (2, 2, 1, 33, True)
    c = count_case(*shape, 64)
    q, k, v = (c[n].cuda() for n in "qkv")
    o, lse = _ext().attention_fwd_lse(q, k, v, True, c["scale"])
    torch.cuda.synchronize()
    judge(c, o, lse, "valid call after a refused or empty one")


@requires_gpu
@pytest.mark.parametrize("D", DS)
def test_empty_inputs_launch_nothing_and_no_key_raises(D):
    ext = _ext()
    mk = lambda *s: torch.zeros(*s, dtype=BF, device="cuda")
    for Bn, Sq in ((0, 8), (2, 0), (0, 0)):
        q, k, v = mk(Bn, 4, Sq, D), mk(Bn, 2, 16, D), mk(Bn, 2, 16, D)
        for o in (ext.attention(q, k, v, True, 0.125),
                  F.attention(q, k, v, causal=True)):
            assert o.shape == (Bn, 4, Sq, D) and o.dtype is BF and o.is_cuda
        o = ext.attention_bshd(q, k, v, False, 0.125)
        assert o.shape == (Bn, Sq, 4, D) and o.dtype is BF
        for fn, shp in ((ext.attention_fwd_lse, (Bn, 4, Sq, D)),
                        (ext.attention_fwd_lse_bshd, (Bn, Sq, 4, D))):
            o, lse = fn(q, k, v, True, 0.125)
            assert o.shape == shp and o.dtype is BF
            assert lse.shape == (Bn, 4, Sq) and lse.dtype is torch.float32
        qs = mk(Bn, Sq, 4, D)
        assert F.attention_qkv(qs, mk(Bn, 16, 2, D), mk(Bn, 16, 2, D)).shape \
            == (Bn, Sq, 4 * D)
        torch.cuda.synchronize()
        _valid_small_call()
    q, k, v = mk(2, 4, 8, D), mk(2, 2, 0, D), mk(2, 2, 0, D)
    for fn in (ext.attention, ext.attention_bshd, ext.attention_fwd_lse,
               ext.attention_fwd_lse_bshd):
        with pytest.raises(RuntimeError, match="Sk"):
            fn(q, k, v, False, 0.125)
    with pytest.raises(ValueError, match="Sk"):
        F.attention(q, k, v)
    with pytest.raises(ValueError, match="Sk"):
        F.attention_qkv(*(t.transpose(1, 2) for t in (q, k, v)))
    with pytest.raises(RuntimeError, match="Sk"):  # no key AND no query
        ext.attention(mk(0, 4, 8, D), mk(0, 2, 0, D), mk(0, 2, 0, D), False,
                      0.125)
    torch.cuda.synchronize()
    _valid_small_call()


# ------------------------------------------------- 8. the DEFER=false kernels

@requires_gpu
@pytest.mark.skipif(NODEFER in os.environ,
                    reason="already inside the no-defer child")
def test_nodefer_instantiations_pass_the_same_rules():
    """MODAL_AMD_FA_NODEFER is read once per process: one fresh child runs
    the bitwise and yardstick tests of this file on the DEFER=false
    instantiations."""
    env = dict(os.environ)
    env[NODEFER] = "1"
    cmd = [sys.executable, "-m", "pytest", str(Path(__file__).resolve()),
           "-q", "-p", "no:cacheprovider", "-k", "selector or ramp or count"]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True,
                           cwd=Path(__file__).resolve().parent.parent,
                           timeout=3 * CHILD_S)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if e.stdout else ""
        pytest.exit(f"no-defer child hung (> {3 * CHILD_S} s); nothing more "
                    f"runs on this GPU.\n{out[-3000:]}", returncode=1)
    tail = f"\n{r.stdout[-4000:]}\n{r.stderr[-1000:]}"
    if r.returncode < 0 or r.returncode in FATAL_EXITS:
        pytest.exit(f"no-defer child died with status {r.returncode}; "
                    f"nothing more runs on this GPU.{tail}", returncode=1)
    assert r.returncode == 0, tail
    last = r.stdout.strip().splitlines()[-1]
    assert " passed" in last and "skipped" not in last, tail
