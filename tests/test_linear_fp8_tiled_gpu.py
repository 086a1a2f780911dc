"""The workgroup-tiled fp8 GEMM for prefill (fp8_gemm_tiled_kernel in
csrc/linear_fp8.hip) on the GPU: exact cases bit for bit under both tiles and
the rule, random cases element by element against the fp64 bound,
reproducibility and row independence, composition, refused calls and
Fp8Linear's prefill lane.

A workgroup owns a BM x 128 tile over all of K: tile 1 is BM = 128, tile 2 is
BM = 256; the rule (tile 0) takes tile 1 for every shape and is run over
both tiles' row counts.  K is walked in
chunks of 128 through two LDS stages: a prologue stages chunk 0, every body
trip loads the next chunk over the current one's MFMAs, the tail runs the
last chunk's MFMAs.

  K      chunks   prologue   body trips   tail
  128    1        1          0            1
  256    2        1          1            1
  384    3        1          2            1     (stage 0 reused)
  512    4        1          3            1     (stage 1 reused)
  640    5        1          4            1

N = 64 is half a column tile (the dead half's waves skip their MFMAs and
stores), 128 one tile, 192 a tile and a live half.  M = 1, BM - 1, BM,
BM + 1, 2 * BM + 1 cover a partial tile, a full one and the step to the next
block.
"""
import functools

import pytest
import torch

from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from test_linear_fp8 import exact_case, exact_offsets, random_case

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda"
BM = {1: 128, 2: 256}
TILES = (0, 1, 2)
RANDOM_SHAPES = ((257, 192, 640), (129, 320, 4096), (513, 128, 1024))

exact = functools.lru_cache(maxsize=None)(exact_case)
rand = functools.lru_cache(maxsize=None)(random_case)


def _ext():
    from modal_examples_amd.ops._build import get_ext

    return get_ext(required=True)


def _gemm(c, tile):
    a = [c[k].to(DEV) for k in ("xq", "xscale", "qweight", "wscale")]
    if tile == 0:
        return OF.linear_fp8_q(*a, tiled=True).cpu()
    return _ext().linear_fp8_tiled(*a, tile).cpu()


def _rows(tile):
    bms = (128, 256) if tile == 0 else (BM[tile],)
    return sorted({m for b in bms for m in (1, b - 1, b, b + 1, 2 * b + 1)})


@requires_gpu
@pytest.mark.parametrize("K", (128, 256, 384, 512, 640))
@pytest.mark.parametrize("tile", TILES)
def test_exact_cases_bitwise(tile, K):
    for N in (64, 128, 192):
        for M in _rows(tile):
            for off in exact_offsets(M):
                c = exact(M, N, K, seed=K + M, off=off)
                got = _gemm(c, tile)
                assert got.dtype is torch.bfloat16 and got.shape == (M, N)
                assert torch.equal(got, c["want"]), (M, N, K, off)
            if K <= 256:
                c = exact(M, N, K, seed=K + M, dense=True)
                assert torch.equal(_gemm(c, tile), c["want"]), (M, N, K)


@requires_gpu
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_random_cases_within_the_bound(shape):
    c = rand(*shape, seed=sum(shape))
    want, tol = ref.linear_fp8_bound_ref(c["xq"], c["xscale"], c["qweight"],
                                         c["wscale"])
    for tile in TILES:
        got = _gemm(c, tile)
        assert got.shape == want.shape == tol.shape == shape[:2]
        ratio = (got.double() - want).abs() / tol
        # every element is compared: no mask, and tol is positive everywhere
        assert bool((tol > 0).all()) and ratio.numel() == want.numel()
        print(f"{shape} tile={tile}: worst ratio {float(ratio.max()):.3f}")
        assert bool((ratio <= 1).all()), (tile, float(ratio.max()))


@requires_gpu
def test_reproducible_and_independent_of_the_other_rows():
    c = rand(300, 192, 1024, seed=11)
    x, q, s = c["x"].to(DEV), c["qweight"].to(DEV), c["wscale"].to(DEV)
    a = OF.linear_fp8(x, q, s, tiled=True)
    assert torch.equal(a, OF.linear_fp8(x, q, s, tiled=True))
    for lo, hi in ((0, 1), (37, 170), (255, 300)):
        # another M, another tile, other rows of the tile
        assert torch.equal(OF.linear_fp8(x[lo:hi], q, s, tiled=True),
                           a[lo:hi]), (lo, hi)


@requires_gpu
def test_composition_and_refused_calls():
    ext = _ext()
    c = rand(33, 192, 640, seed=7)
    x = c["x"].to(DEV)
    xq, xs, q, s = (c[k].to(DEV) for k in ("xq", "xscale", "qweight",
                                           "wscale"))
    y = OF.linear_fp8(x, q, s, tiled=True)
    assert y.dtype is torch.bfloat16 and y.shape == (33, 192)
    assert torch.equal(
        y, OF.linear_fp8_q(*OF.quantize_rows_fp8(x), q, s, tiled=True))
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ext.linear_fp8_tiled(xq[:, :192].contiguous(), xs,
                             q[:, :192].contiguous(), s)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ext.linear_fp8_tiled(xq, xs, q[:96].contiguous(), s[:96].contiguous())
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        ext.linear_fp8_tiled(x, xs, q, s)
    with pytest.raises(RuntimeError, match="do not match"):
        ext.linear_fp8_tiled(xq[:, :128].contiguous(), xs, q, s)
    with pytest.raises(RuntimeError, match="out of range"):
        ext.linear_fp8_tiled(xq, xs, q, s, 3)


@requires_gpu
def test_module_prefill_lane(monkeypatch):
    from modal_examples_amd.models.llama.model import Fp8Linear

    c = rand(Fp8Linear.M_KERNEL + 1, 128, 256, seed=3)
    fl = Fp8Linear(256, 128)
    fl.qweight, fl.wscale = c["qweight"], c["wscale"]
    fl.to(DEV)
    x = c["x"].to(DEV)
    with torch.no_grad():
        monkeypatch.setattr(Fp8Linear, "PREFILL_LANE", "tiled")
        assert torch.equal(
            fl(x), OF.linear_fp8(x, fl.qweight, fl.wscale, tiled=True))
        monkeypatch.setattr(Fp8Linear, "PREFILL_LANE", "dequant")
        w = OF.dequantize_fp8(fl.qweight, fl.wscale).to(x.dtype)
        assert torch.equal(fl(x), torch.nn.functional.linear(x, w))
        # rows up to M_KERNEL do not look at the lane
        monkeypatch.setattr(Fp8Linear, "PREFILL_LANE", "tiled")
        assert torch.equal(fl(x[:-1]),
                           OF.linear_fp8(x[:-1], fl.qweight, fl.wscale))
