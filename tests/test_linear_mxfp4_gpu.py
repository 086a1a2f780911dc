"""MXFP4 weight linear on the GPU (csrc/linear_mxfp4.hip): exact GEMM cases
bit for bit (every nibble, hashed block exponents, the E8M0 bias), random
cases element by element against the fp64 bound, reproducibility and row
independence, graph capture, refused calls, and the engine's
weight_dtype="mxfp4" lane.

The GEMM walks K in chunks of 128 through linear_fp8's pipeline, so the
table and the forced splits of tests/test_linear_fp8_gpu.py hold here."""
import pytest
import torch

from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from test_linear_fp8 import EXACT_K, EXACT_M, EXACT_N, RANDOM_SHAPES
from test_linear_fp8_gpu import FORCED_SPLITS
from test_linear_mxfp4 import exact_case, random_case

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda"
TARGET_WAVES = 512


def _ext():
    from modal_examples_amd.ops._build import get_ext

    return get_ext(required=True)


def _gemm(c, splits=None, mtiles=0):
    """GPU -> CPU result: the public op, or the binding's test arguments."""
    a = [c[k].to(DEV) for k in ("xq", "xscale", "qweight", "wscale")]
    if splits is None and mtiles == 0:
        return OF.linear_mxfp4_q(*a).cpu()
    return _ext().linear_mxfp4(*a, splits or 0, mtiles).cpu()


@requires_gpu
@pytest.mark.parametrize("N", EXACT_N)
@pytest.mark.parametrize("K", EXACT_K)
def test_exact_cases_bitwise(N, K):
    ext = _ext()
    assert ext.linear_mxfp4_splits(1, N, K, 1) == 1
    rule = min(K // 128, -(-TARGET_WAVES // (N // 64)))
    assert ext.linear_mxfp4_splits(1, N, K) == rule
    for M in EXACT_M:
        c = exact_case(M, N, K, seed=K + M)
        got = _gemm(c, splits=1)
        assert got.dtype is torch.bfloat16 and got.shape == (M, N)
        assert torch.equal(got, c["want"]), (M, N, K, "one slice")
        assert torch.equal(_gemm(c), c["want"]), (M, N, K, "rule")
        if M >= 64:
            for mt in (1, 2):
                assert torch.equal(_gemm(c, 1, mt), c["want"]), (M, N, K, mt)
                assert torch.equal(_gemm(c, 0, mt), c["want"]), (M, N, K, mt)


@requires_gpu
@pytest.mark.parametrize("K,splits,S", FORCED_SPLITS)
def test_exact_cases_bitwise_forced_splits(K, splits, S):
    ext = _ext()
    for N in EXACT_N:
        assert ext.linear_mxfp4_splits(65, N, K, splits) == S
        for M in (1, 33, 65):
            c = exact_case(M, N, K, seed=K + M + splits)
            assert torch.equal(_gemm(c, splits), c["want"]), (M, N)


@requires_gpu
@pytest.mark.parametrize("exponent", (-30, 30))
def test_scale_decode_has_bias_127_and_does_not_clip(exponent):
    for M, N, K in ((33, 64, 384), (65, 192, 640)):
        c = exact_case(M, N, K, seed=K + M, exponent=exponent)
        unit = exact_case(M, N, K, seed=K + M, exponent=0)
        assert int(c["wscale"][0, 0]) == 127 + exponent
        assert torch.equal(c["want"].double(),
                           unit["want"].double() * 2.0 ** exponent)
        assert torch.equal(_gemm(c, splits=1), c["want"]), (M, N, K)
        assert torch.equal(_gemm(c), c["want"]), (M, N, K, "rule")


@requires_gpu
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_random_cases_within_the_bound(shape):
    c = random_case(*shape, seed=sum(shape))
    want, tol = ref.linear_mxfp4_bound_ref(c["xq"], c["xscale"], c["qweight"],
                                           c["wscale"])
    S = _ext().linear_mxfp4_splits(*shape)
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
def test_reproducible_and_independent_of_the_other_rows():
    N, K = 192, 1024
    c = random_case(65, N, K, seed=11)
    x, q, s = c["x"].to(DEV), c["qweight"].to(DEV), c["wscale"].to(DEV)
    ext = _ext()
    assert ext.linear_mxfp4_splits(65, N, K) > 1      # the split is engaged
    a, b = OF.linear_mxfp4(x, q, s), OF.linear_mxfp4(x, q, s)
    assert torch.equal(a, b)
    assert torch.equal(a, OF.linear_mxfp4_q(*OF.quantize_rows_fp8(x), q, s))
    a33 = OF.linear_mxfp4(x[:33], q, s)
    assert torch.equal(a33, a[:33])
    for r in (0, 31, 32):
        # a row alone: one M-tile per wave instead of two, another tile row
        assert torch.equal(OF.linear_mxfp4(x[r:r + 1], q, s)[0], a[r]), r
    assert torch.equal(OF.linear_mxfp4(x[64:65], q, s)[0], a[64])
    # M does not enter the split rule
    assert len({ext.linear_mxfp4_splits(m, N, K)
                for m in (1, 32, 65, 4096)}) == 1


@requires_gpu
def test_captures_into_a_graph():
    M, N, K = 7, 128, 1024
    c1, c2 = random_case(M, N, K, seed=21), random_case(M, N, K, seed=22)
    q, s = c1["qweight"].to(DEV), c1["wscale"].to(DEV)
    assert _ext().linear_mxfp4_splits(M, N, K) > 1   # workspace in the capture
    static_x = c1["x"].to(DEV).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        OF.linear_mxfp4(static_x, q, s)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_y = OF.linear_mxfp4(static_x, q, s)
    for c in (c1, c2, c1):
        static_x.copy_(c["x"].to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_y, OF.linear_mxfp4(c["x"].to(DEV), q, s))
    del g


@requires_gpu
def test_unsupported_calls_raise():
    """By the Python checks, the binding and the plan (0 = unsupported)."""
    ext = _ext()
    c = random_case(3, 64, 256, seed=5)
    x = c["x"].to(DEV)
    xq, xs, q, s = (c[k].to(DEV) for k in ("xq", "xscale", "qweight",
                                           "wscale"))
    assert ext.linear_mxfp4_splits(3, 64, 256, 3) == 0  # more slices than chunks
    assert ext.linear_mxfp4_splits(3, 96, 256) == 0
    assert ext.linear_mxfp4_splits(3, 64, 192) == 0
    with pytest.raises(RuntimeError, match="not supported"):
        ext.linear_mxfp4(xq, xs, q, s, 3)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ext.linear_mxfp4(xq[:, :192].contiguous(), xs,
                         q[:, :96].contiguous(), s[:, :6].contiguous())
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        ext.linear_mxfp4(x, xs, q, s)
    with pytest.raises(RuntimeError, match="uint8"):
        ext.linear_mxfp4(xq, xs, q.int(), s)
    with pytest.raises(RuntimeError, match="do not match"):
        ext.linear_mxfp4(xq[:, :128].contiguous(), xs, q, s)
    with pytest.raises(ValueError, match="K=256"):
        OF.linear_mxfp4(x[:, :128].contiguous(), q, s)
    with pytest.raises(ValueError, match="N=96"):
        OF.linear_mxfp4(x, torch.cat([q, q[:32]]), torch.cat([s, s[:32]]))
    with pytest.raises(ValueError, match="is on"):
        OF.linear_mxfp4(x, q.cpu(), s.cpu())


def _engine_tokens(use_graph):
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    # max_batch = the number of requests: both lanes run the same shapes
    eng = LlamaEngine(LlamaConfig.small(), device="cuda",
                      dtype=torch.bfloat16, use_graph=use_graph,
                      kv_blocks=128, eos_id=-1, max_batch=3,
                      weight_dtype="mxfp4")
    rids = [eng.add_request([1, 17 + i, 99, 250, 31], max_new_tokens=16)
            for i in range(3)]
    eng.run_until_done()
    return eng, [eng.finished[r].out_tokens for r in rids]


@requires_gpu
def test_engine_mxfp4_graph_equals_eager():
    from modal_examples_amd.models.llama.model import (QUANT_PROJECTIONS,
                                                       Mxfp4Linear)

    eng, out_g = _engine_tokens(use_graph=True)
    assert eng.use_graph and eng._graph is not None
    for blk in eng.model.blocks:
        for name in QUANT_PROJECTIONS:
            m = getattr(blk, name)
            assert isinstance(m, Mxfp4Linear)
            assert m.qweight.dtype is torch.uint8 and m.qweight.is_cuda
            assert m.wscale.dtype is torch.uint8
    assert eng.model.lm_head.weight.dtype is torch.bfloat16
    assert all(len(t) == 16 and all(0 <= v < 1024 for v in t) for t in out_g)
    _, out_e = _engine_tokens(use_graph=False)
    assert out_g == out_e
    eng.close()
