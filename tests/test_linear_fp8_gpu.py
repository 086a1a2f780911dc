"""FP8 W8A8 linear on the GPU (csrc/linear_fp8.hip): the row quantizer bit
for bit, exact GEMM cases bit for bit, random cases element by element
against the fp64 bound, composition, reproducibility and row independence,
graph capture, refused calls, and the engine's weight_dtype="fp8" lane.

The GEMM walks K in chunks of 128.  A wave owns one slice of K — `cps`
consecutive chunks — and runs them through linear_w4's two-register-set
pipeline: a body of two chunks while more than two remain, then a tail of
two chunks or of one.  With splits=1 K alone picks the path:

  K      chunks   body trips   tail
  128    1        0            1
  256    2        0            2
  384    3        1            1
  512    4        1            2
  640    5        2            1

The split rule is S = min(K/128, ceil(FP8_TARGET_WAVES / (N/64))), a
function of (N, K) only; at the widths used here (N = 64 .. 256) that is
S = K/128: K = 128 runs unsplit (scaled bf16 from the GEMM epilogue), every
larger K as one-chunk slices through the fp32 workspace and the reduce
kernel, which applies the scales.  FORCED_SPLITS adds uneven slices (640 / 2
is 3 + 2 chunks, 1024 / 3 is 3 + 3 + 2, 1024 / 5 normalises to 4 slices).

M = 1, 31, 32, 33 cover a partial and a full 32-row M-tile and the step to
two M-tiles per wave (above 32 rows); 64 and 65 fill that tile and start the
next, also with one and two M-tiles forced.  The row quantizer keeps a row in
registers up to K = 16384; K = 16512 is the smallest size on its other path.
"""
import pytest
import torch

from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from test_linear_fp8 import (EXACT_K, EXACT_M, EXACT_N, RANDOM_SHAPES,
                             exact_case, exact_offsets, quant_rows,
                             random_case)

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda"
FP8 = torch.float8_e4m3fn
TARGET_WAVES = 512

# (K, splits, S after normalisation)
FORCED_SPLITS = ((640, 2, 2), (1024, 2, 2), (1024, 3, 3), (1024, 4, 4),
                 (1024, 5, 4), (1024, 8, 8))


def _ext():
    from modal_examples_amd.ops._build import get_ext

    return get_ext(required=True)


def _gemm(c, splits=None, mtiles=0):
    """GPU -> CPU result: the public op, or the binding's test arguments."""
    a = [c[k].to(DEV) for k in ("xq", "xscale", "qweight", "wscale")]
    if splits is None and mtiles == 0:
        return OF.linear_fp8_q(*a).cpu()
    return _ext().linear_fp8(*a, splits or 0, mtiles).cpu()


@requires_gpu
@pytest.mark.parametrize("K", (128, 640, 16512))
@pytest.mark.parametrize("M", (1, 33))
def test_row_quantization_is_exact(M, K):
    x = quant_rows(K, seed=K)
    blocks = [x] if M == 33 else [x[r:r + 1] for r in range(5)]
    for xb in blocks:
        want_q, want_s = ref.quantize_rows_fp8_ref(xb)
        got_q, got_s = OF.quantize_rows_fp8(xb.to(DEV))
        assert got_q.dtype is FP8 and got_s.dtype is torch.float32
        assert torch.equal(got_s.cpu(), want_s)
        gq = got_q.cpu().float()
        assert not bool(torch.isnan(gq).any())
        assert torch.equal(gq, want_q.float())


@requires_gpu
@pytest.mark.parametrize("N", EXACT_N)
@pytest.mark.parametrize("K", EXACT_K)
def test_exact_cases_bitwise(N, K):
    ext = _ext()
    assert ext.linear_fp8_splits(1, N, K, 1) == 1
    rule = min(K // 128, -(-TARGET_WAVES // (N // 64)))
    assert ext.linear_fp8_splits(1, N, K) == rule == K // 128
    for M in EXACT_M:
        for off in exact_offsets(M):
            c = exact_case(M, N, K, seed=K + M, off=off)
            got = _gemm(c, splits=1)
            assert got.dtype is torch.bfloat16 and got.shape == (M, N)
            assert torch.equal(got, c["want"]), (M, N, K, off, "one slice")
            assert torch.equal(_gemm(c), c["want"]), (M, N, K, off, "rule")
        if M >= 64:
            for mt in (1, 2):
                assert torch.equal(_gemm(c, 1, mt), c["want"]), (M, N, K, mt)
                assert torch.equal(_gemm(c, 0, mt), c["want"]), (M, N, K, mt)
        if K <= 256:
            c = exact_case(M, N, K, seed=K + M, dense=True)
            assert torch.equal(_gemm(c, splits=1), c["want"]), (M, N, K)
            assert torch.equal(_gemm(c), c["want"]), (M, N, K, "rule")


@requires_gpu
@pytest.mark.parametrize("K,splits,S", FORCED_SPLITS)
def test_exact_cases_bitwise_forced_splits(K, splits, S):
    ext = _ext()
    for N in EXACT_N:
        assert ext.linear_fp8_splits(65, N, K, splits) == S
        for M in (1, 33, 65):
            c = exact_case(M, N, K, seed=K + M + splits)
            assert torch.equal(_gemm(c, splits), c["want"]), (M, N)


@requires_gpu
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_random_cases_within_the_bound(shape):
    c = random_case(*shape, seed=sum(shape))
    want, tol = ref.linear_fp8_bound_ref(c["xq"], c["xscale"], c["qweight"],
                                         c["wscale"])
    S = _ext().linear_fp8_splits(*shape)
    for splits in (None, 1):
        got = _gemm(c, splits)
        assert got.shape == want.shape == tol.shape == shape[:2]
        ratio = (got.double() - want).abs() / tol
        # every element is compared: no mask, and tol is positive everywhere
        assert bool((tol > 0).all()) and ratio.numel() == want.numel()
        print(f"{shape} S={S if splits is None else 1}: worst ratio "
              f"{float(ratio.max()):.3f}")
        assert bool((ratio <= 1).all()), float(ratio.max())


@requires_gpu
def test_public_op_is_quantize_then_gemm():
    c = random_case(33, 192, 640, seed=7)
    x, q, s = c["x"].to(DEV), c["qweight"].to(DEV), c["wscale"].to(DEV)
    y = OF.linear_fp8(x, q, s)
    assert y.dtype is torch.bfloat16 and y.shape == (33, 192)
    assert torch.equal(y, OF.linear_fp8_q(*OF.quantize_rows_fp8(x), q, s))


@requires_gpu
def test_reproducible_and_independent_of_the_other_rows():
    M, N, K = 65, 192, 1024
    c = random_case(M, N, K, seed=11)
    x, q, s = c["x"].to(DEV), c["qweight"].to(DEV), c["wscale"].to(DEV)
    ext = _ext()
    assert ext.linear_fp8_splits(M, N, K) > 1       # the split is engaged
    a, b = OF.linear_fp8(x, q, s), OF.linear_fp8(x, q, s)
    assert torch.equal(a, b)
    for r in (0, 31, 32, 64):
        # a row alone: its own scale, one M-tile per wave instead of two
        assert torch.equal(OF.linear_fp8(x[r:r + 1], q, s)[0], a[r]), r
    # M does not enter the split rule
    assert len({ext.linear_fp8_splits(m, N, K) for m in (1, 32, 65, 4096)}) == 1


@requires_gpu
def test_captures_into_a_graph():
    M, N, K = 7, 128, 1024
    c1, c2 = random_case(M, N, K, seed=21), random_case(M, N, K, seed=22)
    q, s = c1["qweight"].to(DEV), c1["wscale"].to(DEV)
    assert _ext().linear_fp8_splits(M, N, K) > 1     # workspace in the capture
    static_x = c1["x"].to(DEV).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        OF.linear_fp8(static_x, q, s)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_y = OF.linear_fp8(static_x, q, s)
    for c in (c1, c2, c1):
        static_x.copy_(c["x"].to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_y, OF.linear_fp8(c["x"].to(DEV), q, s))
    del g


@requires_gpu
def test_unsupported_calls_raise():
    """By the Python checks, the binding and the plan (0 = unsupported)."""
    ext = _ext()
    c = random_case(3, 64, 256, seed=5)
    x = c["x"].to(DEV)
    xq, xs, q, s = (c[k].to(DEV) for k in ("xq", "xscale", "qweight",
                                           "wscale"))
    assert ext.linear_fp8_splits(3, 64, 256, 3) == 0  # more slices than chunks
    assert ext.linear_fp8_splits(3, 96, 256) == 0
    assert ext.linear_fp8_splits(3, 64, 192) == 0
    with pytest.raises(RuntimeError, match="not supported"):
        ext.linear_fp8(xq, xs, q, s, 3)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ext.linear_fp8(xq[:, :192].contiguous(), xs, q[:, :192].contiguous(),
                       s)
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        ext.linear_fp8(x, xs, q, s)
    with pytest.raises(RuntimeError, match="do not match"):
        ext.linear_fp8(xq[:, :128].contiguous(), xs, q, s)
    with pytest.raises(ValueError, match="K=256"):
        OF.linear_fp8(x[:, :128].contiguous(), q, s)
    with pytest.raises(ValueError, match="N=96"):
        OF.linear_fp8(x, torch.cat([q, q[:32]]), torch.cat([s, s[:32]]))
    with pytest.raises(ValueError, match="is on"):
        OF.linear_fp8(x, q.cpu(), s.cpu())


def _engine_tokens(use_graph):
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    # max_batch = the number of requests: both lanes run the same shapes
    eng = LlamaEngine(LlamaConfig.small(), device="cuda",
                      dtype=torch.bfloat16, use_graph=use_graph,
                      kv_blocks=128, eos_id=-1, max_batch=3,
                      weight_dtype="fp8")
    rids = [eng.add_request([1, 17 + i, 99, 250, 31], max_new_tokens=16)
            for i in range(3)]
    eng.run_until_done()
    return eng, [eng.finished[r].out_tokens for r in rids]


@requires_gpu
def test_engine_fp8_graph_equals_eager():
    from modal_examples_amd.models.llama.model import (QUANT_PROJECTIONS,
                                                       Fp8Linear)

    eng, out_g = _engine_tokens(use_graph=True)
    assert eng.use_graph and eng._graph is not None
    for blk in eng.model.blocks:
        for name in QUANT_PROJECTIONS:
            m = getattr(blk, name)
            assert isinstance(m, Fp8Linear)
            assert m.qweight.dtype is FP8 and m.qweight.is_cuda
            assert m.wscale.dtype is torch.float32
    assert eng.model.lm_head.weight.dtype is torch.bfloat16
    assert all(len(t) == 16 and all(0 <= v < 1024 for v in t) for t in out_g)
    _, out_e = _engine_tokens(use_graph=False)
    assert out_g == out_e
    eng.close()
