"""Int4 weight-only linear on the GPU (csrc/linear_w4.hip): the exact cases
bit for bit, random cases element by element against the fp64 bound,
reproducibility and row independence, graph capture, and the engine's
weight_dtype="int4" lane under the decode graph.

The kernel walks K in chunks of one quantization group (128).  A wave owns
one slice of K — `cps` consecutive chunks — and runs them through a
two-register-set pipeline: a body of two chunks while more than two remain,
then a tail of two chunks or of one.  With splits=1 (one slice, set through
the binding's test-only argument) K alone picks the path:

  K      chunks   body trips   tail
  128    1        0            1
  256    2        0            2
  384    3        1            1
  512    4        1            2
  640    5        2            1

The split rule is S = min(K/128, ceil(512 / (N/64))), a function of (N, K)
only.  At the widths used here (N = 64 .. 256) that is always S = K/128: the
public op runs K = 128 unsplit (bf16 written by the GEMM epilogue) and every
larger K as one-chunk slices through the fp32 workspace and the reduce
kernel.  The forced splits below add uneven slices:

  K      splits   cps   S   chunks per slice
  640    2        3     2   3, 2
  1024   2        4     2   4, 4
  1024   3        3     3   3, 3, 2
  1024   4        2     4   2, 2, 2, 2
  1024   5        2     4   (normalised: no empty slice)
  1024   8        1     8   1 each

M = 1, 31, 32, 33, 65 cover a masked tail, an exactly full M-tile, and a
second and third M-tile; N = 192 puts three column tiles in the grid.
"""
import functools

import pytest
import torch

from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from test_linear_w4 import (EXACT_K, EXACT_M, EXACT_N, RANDOM_SHAPES,
                            assert_exact_case_sound, dense_case, exact_case,
                            exact_offsets, exact_want, random_case)

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda"

# (K, splits, S after normalisation)
FORCED_SPLITS = ((640, 2, 2), (1024, 2, 2), (1024, 3, 3), (1024, 4, 4),
                 (1024, 5, 4), (1024, 8, 8))


def _ext():
    from modal_examples_amd.ops._build import get_ext

    return get_ext(required=True)


def _kernel(c, splits=None):
    """The case on the GPU -> CPU result.  splits=None is the public op;
    a number goes through the binding's test-only argument."""
    x, q, s = c["x"].to(DEV), c["qweight"].to(DEV), c["scales"].to(DEV)
    if splits is None:
        return OF.linear_w4(x, q, s).cpu()
    return _ext().linear_w4(x, q, s, splits).cpu()


def _rule(N, K):
    return min(K // 128, -(-512 // (N // 64)))


# -------------------------------------------------------------- exact cases

@requires_gpu
@pytest.mark.parametrize("N", EXACT_N)
@pytest.mark.parametrize("K", EXACT_K)
def test_exact_cases_bitwise(N, K):
    """Every chunk count of the table, one slice and the public op's split,
    against the exact product."""
    ext = _ext()
    assert ext.linear_w4_splits(1, N, K, 1) == 1
    assert ext.linear_w4_splits(1, N, K) == _rule(N, K) == K // 128
    for M in EXACT_M:
        for off in exact_offsets(M):
            c = exact_case(M, N, K, seed=K + M, off=off)
            want = exact_want(c)
            got = _kernel(c, splits=1)
            assert got.dtype is torch.bfloat16 and got.shape == (M, N)
            assert torch.equal(got, want), (M, N, K, off, "one slice")
            assert torch.equal(_kernel(c), want), (M, N, K, off, "rule")


@requires_gpu
@pytest.mark.parametrize("K,splits,S", FORCED_SPLITS)
def test_exact_cases_bitwise_forced_splits(K, splits, S):
    ext = _ext()
    for N in EXACT_N:
        assert ext.linear_w4_splits(65, N, K, splits) == S
        for M in (1, 33, 65):
            c = exact_case(M, N, K, seed=K + M + splits)
            assert_exact_case_sound(c)
            assert torch.equal(_kernel(c, splits), exact_want(c)), (M, N)


@requires_gpu
@pytest.mark.parametrize("K", (128, 256))
def test_dense_case_bitwise(K):
    for M in (1, 33):
        c = dense_case(M, 64, K, seed=K + M)
        assert_exact_case_sound(c)
        want = exact_want(c)
        assert torch.equal(_kernel(c), want), (M, K, "rule")
        assert torch.equal(_kernel(c, 1), want), (M, K, "one slice")


# ------------------------------------------------------------- random cases

@functools.lru_cache(maxsize=None)
def _random(shape):
    c = random_case(*shape, seed=sum(shape))
    want, tol = ref.linear_w4_bound_ref(c["x"], c["qweight"], c["scales"])
    return c, want, tol


@requires_gpu
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_random_cases_within_the_bound(shape):
    c, want, tol = _random(shape)
    S = _ext().linear_w4_splits(*shape)
    for splits in (None, 1):
        got = _kernel(c, splits)
        assert got.shape == want.shape == tol.shape == shape[:2]
        assert bool(torch.isfinite(got).all())
        ratio = (got.double() - want).abs() / tol
        # every element is compared: no mask, and tol is positive everywhere
        assert bool((tol > 0).all()) and ratio.numel() == want.numel()
        print(f"{shape} S={S if splits is None else 1}: worst ratio "
              f"{float(ratio.max()):.3f}")
        assert bool((ratio <= 1).all()), float(ratio.max())


# ------------------------------------- reproducibility and row independence

@requires_gpu
def test_reproducible_and_independent_of_the_other_rows():
    M, N, K = 65, 192, 1024
    c = random_case(M, N, K, seed=11)
    assert _ext().linear_w4_splits(M, N, K) > 1     # the split is engaged
    for splits in (None, 1, 3):
        a, b = _kernel(c, splits), _kernel(c, splits)
        assert torch.equal(a, b), splits
        for r in (0, 31, 32, 64):
            one = dict(c, x=c["x"][r:r + 1].contiguous())
            assert torch.equal(_kernel(one, splits)[0], a[r]), (splits, r)
    # M does not enter the split rule
    ext = _ext()
    assert len({ext.linear_w4_splits(m, N, K) for m in (1, 32, 65, 4096)}) == 1


# ------------------------------------------------------------ graph capture

@requires_gpu
def test_captures_into_a_graph():
    M, N, K = 7, 128, 1024
    c1, c2 = random_case(M, N, K, seed=21), random_case(M, N, K, seed=22)
    q, s = c1["qweight"].to(DEV), c1["scales"].to(DEV)
    assert _ext().linear_w4_splits(M, N, K) > 1     # workspace in the capture
    static_x = c1["x"].to(DEV).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        OF.linear_w4(static_x, q, s)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_y = OF.linear_w4(static_x, q, s)
    for c in (c1, c2):
        static_x.copy_(c["x"].to(DEV))
        g.replay()
        torch.cuda.synchronize()
        eager = OF.linear_w4(c["x"].to(DEV), q, s)
        assert torch.equal(static_y, eager)
    del g


# ---------------------------------------------------------- refused shapes

@requires_gpu
def test_unsupported_calls_raise():
    """Refused before anything is launched: by the Python checks, by the
    binding, and by the launcher's plan (0 slices = unsupported)."""
    ext = _ext()
    c = random_case(3, 64, 256, seed=5)
    x, q, s = c["x"].to(DEV), c["qweight"].to(DEV), c["scales"].to(DEV)
    assert ext.linear_w4_splits(3, 64, 256, 3) == 0   # more slices than groups
    assert ext.linear_w4_splits(3, 96, 256) == 0
    assert ext.linear_w4_splits(3, 64, 192) == 0
    assert ext.linear_w4_splits(0, 64, 256) == 0
    with pytest.raises(RuntimeError, match="not supported"):
        ext.linear_w4(x, q, s, 3)
    with pytest.raises(RuntimeError, match="bf16"):
        ext.linear_w4(x.float(), q, s, 0)
    with pytest.raises(RuntimeError, match="do not match"):
        ext.linear_w4(x[:, :128].contiguous(), q, s, 0)
    with pytest.raises(ValueError, match="K=256"):
        OF.linear_w4(x[:, :128].contiguous(), q, s)
    with pytest.raises(ValueError, match="is on"):
        OF.linear_w4(x, q.cpu(), s.cpu())


# ------------------------------------------------------------------- engine

def _engine_tokens(use_graph):
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    # max_batch = the number of requests: the eager lane and the captured
    # lane then run the same kernels on the same shapes, so their tokens
    # are equal, not merely close
    eng = LlamaEngine(LlamaConfig.small(), device="cuda",
                      dtype=torch.bfloat16, use_graph=use_graph,
                      kv_blocks=128, eos_id=-1, max_batch=3,
                      weight_dtype="int4")
    rids = [eng.add_request([1, 17 + i, 99, 250, 31], max_new_tokens=16)
            for i in range(3)]
    eng.run_until_done()
    return eng, [eng.finished[r].out_tokens for r in rids]


@requires_gpu
def test_engine_int4_graph_equals_eager():
    from modal_examples_amd.models.llama.model import (QUANT_PROJECTIONS,
                                                       QuantLinear)

    eng, out_g = _engine_tokens(use_graph=True)
    assert eng.use_graph and eng._graph is not None
    for blk in eng.model.blocks:
        for name in QUANT_PROJECTIONS:
            m = getattr(blk, name)
            assert isinstance(m, QuantLinear)
            assert m.qweight.dtype is torch.int32 and m.qweight.is_cuda
            assert m.scales.dtype is torch.bfloat16
    assert eng.model.lm_head.weight.dtype is torch.bfloat16
    assert all(len(t) == 16 and all(0 <= v < 1024 for v in t) for t in out_g)
    _, out_e = _engine_tokens(use_graph=False)
    assert out_g == out_e
    eng.close()
