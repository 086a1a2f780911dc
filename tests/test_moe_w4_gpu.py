"""Int4 experts on the GPU (the int4 lane of csrc/moe.hip): the exact integer
case bit for bit, the random case element by element against the bound of
the fp64 reference on the dequantized weights, and the contract of the fused
FFN (reproducible, batch-independent rows, graph capture, errors, engine).

Groups of 128 k per GEMM in the exact shapes, (dim, ffn): (128, 128) 1,
(256, 384) 2 and 3, (384, 256) 3 and 2, (512, 640) 4 and 5, (640, 512) 5 and
4.  The up GEMM runs all of K in one slice: zero, one and two body trips and
both tails of the two-register-set loop.  The down GEMM cuts K into
min(2, groups) slices, both counts the rule can give, of ceil(groups / 2)
groups: slices of 1; 2 and 1; 1 and 1; 3 and 2; 2 and 2 groups, the tail of
one, the tail of two and one body trip.  The random case adds slices of 4
groups (ffn 1024): a body trip before the tail of two."""
import pytest
import torch

from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from test_moe_w4 import W4_RANDOM_SHAPES, pack_exact_case, random_w4_case

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda"
PACKED = ("gate_up_q", "gate_up_s", "down_q", "down_s")

EXACT_SHAPES = [(37, 128, 128, 4, 2), (37, 256, 384, 4, 2),
                (37, 384, 256, 4, 2), (37, 512, 640, 4, 2),
                (37, 640, 512, 4, 2),
                (260, 128, 128, 128, 2),  # sparse_idx: 31..103 rows, 120 empty
                (700, 128, 128, 8, 2)]    # second trip of align's loops


@requires_gpu
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=str)
def test_exact_case_bitwise(shape):
    c = pack_exact_case(shape)
    w, idx = OF.moe_route(c["logits"].to(DEV), shape[4])
    assert torch.equal(idx.cpu(), c["idx"]) and torch.equal(w.cpu(), c["weights"])
    got = OF.moe_ffn_w4(c["x"].to(DEV), *(c[n].to(DEV) for n in PACKED), w,
                        idx).cpu()
    want = c["expect"].to(torch.bfloat16)
    bad = (got != want).any(-1).nonzero().flatten()
    assert got.dtype is torch.bfloat16 and torch.equal(got, want), \
        f"{shape}: {bad.numel()} rows differ, first {bad[:8].tolist()}"


def _random_gpu(shape):
    x, packed, gate_up, down, logits = random_w4_case(shape)
    w, idx = OF.moe_route(logits.to(DEV), shape[4])
    return x.to(DEV), tuple(t.to(DEV) for t in packed), w, idx


@requires_gpu
@pytest.mark.parametrize("shape", W4_RANDOM_SHAPES, ids=str)
def test_random_case_within_the_bound(shape):
    """|out - want| <= tol on every element, want and tol from
    ref.moe_ffn_bound_ref on the dequantized experts: the kernels keep the
    weights exact and round at h and at the output, which is what the bound
    models.  No slack on tol; the bf16_points yardstick uses under half of
    it (test_moe_w4.py)."""
    x, packed, w, idx = _random_gpu(shape)
    _, _, gate_up, down, _ = random_w4_case(shape)
    args = (x.cpu(), gate_up, down, w.cpu(), idx.cpu())
    want, tol = ref.moe_ffn_bound_ref(*args)
    yard, _ = ref.moe_ffn_bound_ref(*args, bf16_points=True)
    got = OF.moe_ffn_w4(x, *packed, w, idx).cpu()
    err = (got.double() - want).abs()
    print(f"MOE_FFN_W4_RATIO {shape}: worst err/tol={(err / tol).max():.3f} "
          f"yardstick {((yard - want).abs() / tol).max():.3f} "
          f"over {err.numel()} elements")
    assert torch.isfinite(got).all()
    assert (err <= tol).all(), f"{int((err > tol).sum())} elements outside tol"


@requires_gpu
def test_rows_are_reproducible_and_batch_independent():
    x, packed, w, idx = _random_gpu((200, 384, 640, 8, 2))
    a = OF.moe_ffn_w4(x, *packed, w, idx)
    assert torch.equal(a, OF.moe_ffn_w4(x, *packed, w, idx))
    for t in (0, 77, 199):  # the same token alone: N = 1
        one = OF.moe_ffn_w4(x[t:t + 1], *packed, w[t:t + 1].contiguous(),
                            idx[t:t + 1].contiguous())
        assert torch.equal(one[0], a[t]), t


@requires_gpu
def test_replays_under_a_graph():
    shape = (64, 512, 1024, 8, 4)
    x, packed, w, idx = _random_gpu(shape)
    g = torch.Generator().manual_seed(5)
    others = [(torch.randn(64, 512, generator=g).to(torch.bfloat16).to(DEV),
               *OF.moe_route(torch.randn(64, 8, generator=g).to(DEV), 4))
              for _ in range(3)]
    sx, sw, si = x.clone(), w.clone(), idx.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            OF.moe_ffn_w4(sx, *packed, sw, si)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sy = OF.moe_ffn_w4(sx, *packed, sw, si)
    for x2, w2, i2 in others:
        assert not torch.equal(i2, si)
        sx.copy_(x2), sw.copy_(w2), si.copy_(i2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sy, OF.moe_ffn_w4(x2, *packed, w2, i2))


@requires_gpu
def test_unsupported_calls_raise():
    x, packed, w, idx = _random_gpu(W4_RANDOM_SHAPES[0])
    gq, gs, dq, ds = packed
    with pytest.raises(ValueError, match="x has dim=192"):
        OF.moe_ffn_w4(x[:, :192].contiguous(), *packed, w, idx)
    with pytest.raises(ValueError, match="down_s must be"):
        OF.moe_ffn_w4(x, gq, gs, dq, ds[:, :128].contiguous(), w, idx)
    with pytest.raises(TypeError, match="gate_up_s must be bf16"):
        OF.moe_ffn_w4(x, gq, gs.float(), dq, ds, w, idx)
    with pytest.raises(ValueError, match="gate_up_q must be contiguous"):
        OF.moe_ffn_w4(x, gq.transpose(0, 1).contiguous().transpose(0, 1), gs,
                      dq, ds, w, idx)
    with pytest.raises(ValueError, match="down_q is on cpu"):
        OF.moe_ffn_w4(x, gq, gs, dq.cpu(), ds.cpu(), w, idx)
    with pytest.raises(TypeError, match="idx must be int32"):
        OF.moe_ffn_w4(x, *packed, w, idx.long())


def _engine_tokens(use_graph):
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    torch.manual_seed(0)
    eng = LlamaEngine(LlamaConfig.moe_small(), device="cuda",
                      dtype=torch.bfloat16, moe_impl="fused",
                      expert_dtype="int4", kv_blocks=128, eos_id=-1,
                      use_graph=use_graph)
    assert eng.model.blocks[0].moe.down_q.dtype is torch.int32
    rid = eng.add_request([5, 6, 7, 8, 9], max_new_tokens=6, temperature=0.0)
    eng.run_until_done()
    return eng, eng.finished[rid].out_tokens


@requires_gpu
def test_engine_int4_decodes_under_the_graph():
    eng, out_g = _engine_tokens(True)
    assert eng.use_graph and eng._graph is not None
    _, out_e = _engine_tokens(False)
    assert len(out_g) == 6 and out_g == out_e
