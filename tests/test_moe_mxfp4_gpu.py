"""MXFP4 experts on the GPU (csrc/moe_mxfp4.hip): the exact case bit for bit,
the random case element by element against ref.moe_ffn_mxfp4_bound_ref, and
the contract of the fused FFN (reproducible, batch-independent rows, forced
down slices, graph capture, engine).

Chunks of 128 k per GEMM in the exact shapes, (dim, ffn): (128, 128) 1,
(256, 384) 2 and 3, (384, 256) 3 and 2, (512, 640) 4 and 5, (640, 512) 5 and
4.  The up GEMM runs all of K in one slice: zero, one and two body trips and
both tails of the two-register-set loop.  So does the down GEMM, whose rule
is one slice; forced slices (3 and 2; 2, 2 and 1 chunks of ffn 640) have a
test of their own.  The random case adds 8 chunks (ffn 1024)."""
import pytest
import torch

from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops._build import get_ext
from test_moe_mxfp4 import (PACKED, W4_RANDOM_SHAPES, bound_and_yardstick,
                            mx_exact_case, random_mx_case)
from test_moe_w4_gpu import EXACT_SHAPES

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda"
SHIFTED = (37, 256, 384, 4, 2)


def _exact_gpu(shape, shift=None):
    c = mx_exact_case(shape, shift)
    w, idx = OF.moe_route(c["logits"].to(DEV), shape[4])
    assert torch.equal(idx.cpu(), c["idx"]) and torch.equal(w.cpu(), c["weights"])
    return c, (c["x"].to(DEV), *(c[n].to(DEV) for n in PACKED), w, idx)


@requires_gpu
@pytest.mark.parametrize("shape,shift", [(s, None) for s in EXACT_SHAPES] + [
    (SHIFTED, ("gate_up", 30)), (SHIFTED, ("gate_up", -30)),
    (SHIFTED, ("down", 30)), (SHIFTED, ("down", -30))], ids=str)
def test_exact_case_bitwise(shape, shift):
    c, args = _exact_gpu(shape, shift)
    got = OF.moe_ffn_mxfp4(*args).cpu()
    want = c["expect"].to(torch.bfloat16)
    bad = (got != want).any(-1).nonzero().flatten()
    assert got.dtype is torch.bfloat16 and torch.equal(got, want), \
        f"{shape} {shift}: {bad.numel()} rows differ, first {bad[:8].tolist()}"


def _random_gpu(shape):
    x, packed, logits = random_mx_case(shape)
    w, idx = OF.moe_route(logits.to(DEV), shape[4])
    return x.to(DEV), tuple(t.to(DEV) for t in packed), w, idx


@requires_gpu
@pytest.mark.parametrize("shape", W4_RANDOM_SHAPES, ids=str)
def test_random_case_within_the_bound(shape):
    """|out - want| <= tol on every element, no mask and no slack: want is
    fp64 on the quantized x and the exact w_hat with h unrounded, tol the sum
    of the worst cases of the roundings the semantics name (the reference's
    docstring derives each term); the yardstick uses under half of it
    (test_moe_mxfp4.py)."""
    x, packed, w, idx = _random_gpu(shape)
    want, tol, yard = bound_and_yardstick(shape, w.cpu(), idx.cpu())
    got = OF.moe_ffn_mxfp4(x, *packed, w, idx).cpu()
    err = (got.double() - want).abs()
    print(f"MOE_FFN_MXFP4_RATIO {shape}: worst err/tol={(err / tol).max():.3f} "
          f"yardstick {yard:.3f} over {err.numel()} elements")
    assert torch.isfinite(got).all()
    assert (err <= tol).all(), f"{int((err > tol).sum())} elements outside tol"


@requires_gpu
def test_rows_are_reproducible_and_batch_independent():
    x, packed, w, idx = _random_gpu((200, 384, 640, 8, 2))
    a = OF.moe_ffn_mxfp4(x, *packed, w, idx)
    assert torch.equal(a, OF.moe_ffn_mxfp4(x, *packed, w, idx))
    for t in (0, 77, 199):  # the same token alone: N = 1
        one = OF.moe_ffn_mxfp4(x[t:t + 1], *packed, w[t:t + 1].contiguous(),
                               idx[t:t + 1].contiguous())
        assert torch.equal(one[0], a[t]), t


@requires_gpu
@pytest.mark.parametrize("splits", [1, 2, 4])
def test_forced_down_slices_equal_the_rule(splits):
    """hscale is 1 and every partial sum an integer in the exact case, so any
    number of K slices gives the rule's bits (ffn 640: 5 chunks, slices of 5;
    3 and 2; 2, 2 and 1)."""
    ext = get_ext(required=True)
    assert ext.moe_ffn_mxfp4_splits(640) == 1      # the rule: one slice
    assert ext.moe_ffn_mxfp4_splits(640, 2) == 2
    assert ext.moe_ffn_mxfp4_splits(640, 4) == 3   # no empty slice
    assert ext.moe_ffn_mxfp4_splits(128) == 1 and ext.moe_ffn_mxfp4_splits(192) == 0
    c, args = _exact_gpu((37, 512, 640, 4, 2))
    got = ext.moe_ffn_mxfp4(*args, down_splits=splits)
    assert torch.equal(got, ext.moe_ffn_mxfp4(*args))
    assert torch.equal(got.cpu().double(), c["expect"])


@requires_gpu
def test_replays_under_a_graph():
    shape = (64, 512, 1024, 8, 4)
    x, packed, w, idx = _random_gpu(shape)
    g = torch.Generator().manual_seed(5)
    others = [(torch.randn(64, 512, generator=g).to(torch.bfloat16).to(DEV),
               tuple(t.roll(r, 0) for t in packed),
               *OF.moe_route(torch.randn(64, 8, generator=g).to(DEV), 4))
              for r in (1, 2, 3)]
    sx, sp, sw, si = x.clone(), [t.clone() for t in packed], w.clone(), idx.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            OF.moe_ffn_mxfp4(sx, *sp, sw, si)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sy = OF.moe_ffn_mxfp4(sx, *sp, sw, si)
    for x2, p2, w2, i2 in others:
        assert not torch.equal(i2, si)
        sx.copy_(x2), sw.copy_(w2), si.copy_(i2)
        for dst, src in zip(sp, p2):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sy, OF.moe_ffn_mxfp4(x2, *p2, w2, i2))


def _engine_tokens(use_graph):
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    torch.manual_seed(0)
    eng = LlamaEngine(LlamaConfig.moe_small(), device="cuda",
                      dtype=torch.bfloat16, moe_impl="fused",
                      expert_dtype="mxfp4", kv_blocks=128, eos_id=-1,
                      use_graph=use_graph)
    assert eng.model.blocks[0].moe.down_q.dtype is torch.uint8
    assert eng.model.blocks[0].moe.down_s.dtype is torch.uint8
    rid = eng.add_request([5, 6, 7, 8, 9], max_new_tokens=6, temperature=0.0)
    eng.run_until_done()
    return eng, eng.finished[rid].out_tokens


@requires_gpu
def test_engine_mxfp4_decodes_under_the_graph():
    eng, out_g = _engine_tokens(True)
    assert eng.use_graph and eng._graph is not None
    _, out_e = _engine_tokens(False)
    assert len(out_g) == 6 and out_g == out_e
