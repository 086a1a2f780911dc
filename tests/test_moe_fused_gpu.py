"""Fused MoE FFN on the GPU (csrc/moe.hip): routing against the stable-sort
reference, the exact integer case bit for bit (tile edges included), the
random case against an fp64 reference with the host loop as the yardstick,
reproducibility, graph capture, and the engine's fused lane."""
import functools

import pytest
import torch

from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from test_moe_fused import EXACT_SHAPES, assert_exact_case_sound, exact_case

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tie_free(t):
    v = t.sort(-1).values
    return bool((v[:, 1:] != v[:, :-1]).all())


def _randn_tie_free(N, E, seed):
    """Seeded fp32 randn logits; a seed whose draw holds a tie inside a row
    (a few in a thousand at E = 128) is skipped for the next one."""
    while True:
        logits = torch.randn(N, E, generator=_gen(seed))
        if _tie_free(logits):
            return logits
        seed += 1


def _ffn_gpu(c, weights=None, idx=None):
    """ops.moe_ffn on the GPU for an exact_case dict -> CPU result."""
    w = c["weights"] if weights is None else weights
    i = c["idx"] if idx is None else idx
    return OF.moe_ffn(c["x"].to(DEV), c["gate_up"].to(DEV), c["down"].to(DEV),
                      w.to(DEV), i.to(DEV)).cpu()


# ---------------------------------------------------------------------- route

ROUTE_N = (1, 63, 64, 65, 257)
# top_k <= min(E, 8) is the supported range, so k = 8 pairs with E >= 8 only
ROUTE_EK = [(E, k) for E in (4, 8, 64, 128) for k in (1, 2, 8) if k <= E]


@requires_gpu
@pytest.mark.parametrize("E,k", ROUTE_EK)
def test_route_matches_reference(E, k):
    for N in ROUTE_N:
        logits = _randn_tie_free(N, E, 1000 * E + 10 * k + N)
        assert _tie_free(logits), "tie in input"
        w_ref, i_ref = ref.moe_route_ref(logits, k)
        w, i = OF.moe_route(logits.to(DEV), k)
        assert i.dtype is torch.int32 and w.dtype is torch.float32
        assert torch.equal(i.cpu(), i_ref), (N, E, k)
        torch.testing.assert_close(w.cpu(), w_ref, atol=1e-5, rtol=0)


@requires_gpu
def test_route_ties_take_the_lower_index():
    logits = _randn_tie_free(6, 16, 7)  # rows 4 and 5 stay tie-free
    logits[0] = 1.5                      # a whole row equal
    logits[1] = -0.25                    # another, negative
    logits[2, :] = 0.0
    logits[2, 9] = 2.0
    logits[2, [3, 12, 5]] = 1.0          # tie straddling the k-th place (k=3)
    logits[3, :] = -1.0
    logits[3, [15, 14]] = 4.0            # tie at the top, rest equal
    for k in (1, 3, 8):
        w_ref, i_ref = ref.moe_route_ref(logits, k)
        w, i = OF.moe_route(logits.to(DEV), k)
        assert torch.equal(i.cpu(), i_ref), k
        torch.testing.assert_close(w.cpu(), w_ref, atol=1e-5, rtol=0)
    assert ref.moe_route_ref(logits, 3)[1][2].tolist() == [9, 3, 5]


# ----------------------------------------------------------------- exact case

@functools.lru_cache(maxsize=None)
def _exact(shape):
    c = exact_case(*shape)
    assert_exact_case_sound(c)
    out = ref.moe_ffn_ref(c["x"], c["gate_up"], c["down"], c["weights"],
                          c["idx"])
    assert torch.equal(out.double(), c["expect"])
    return c, out


@requires_gpu
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=str)
def test_exact_case_bitwise(shape):
    c, want = _exact(shape)
    w, idx = OF.moe_route(c["logits"].to(DEV), shape[4])
    assert torch.equal(idx.cpu(), c["idx"])
    assert torch.equal(w.cpu(), c["weights"])
    got = _ffn_gpu(c, w, idx)
    assert got.dtype is torch.bfloat16 and torch.equal(got, want)


EDGE_COUNTS = [0, 1, 31, 32, 33, 64, 65, 129]  # rows per expert, E = 8


def _edge_case(idx):
    c = exact_case(idx.shape[0], 64, 64, 8, 1, idx=idx)
    assert_exact_case_sound(c)
    return c


@requires_gpu
def test_tile_edges_bitwise_and_order_independent():
    idx = torch.repeat_interleave(torch.arange(8),
                                  torch.tensor(EDGE_COUNTS))[:, None]
    c = _edge_case(idx)
    assert torch.bincount(c["idx"][:, 0].long(),
                          minlength=8).tolist() == EDGE_COUNTS
    want = c["expect"].to(torch.bfloat16)
    got = _ffn_gpu(c)
    assert torch.equal(got, want)

    # the same tokens in a shuffled order: same rows out, bit for bit
    perm = torch.randperm(idx.shape[0], generator=_gen(3))
    s = dict(c, x=c["x"][perm], idx=c["idx"][perm])
    got_s = _ffn_gpu(s)
    assert torch.equal(got_s, want[perm])
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    assert torch.equal(got_s[inv], got)


@requires_gpu
@pytest.mark.parametrize("N", [1, 130])
def test_all_rows_to_one_expert_bitwise(N):
    c = _edge_case(torch.full((N, 1), 5))
    assert torch.equal(_ffn_gpu(c), c["expect"].to(torch.bfloat16))


# ---------------------------------------------------------------- random case

def _loop_expression(flat, gate_up, down, w, idx):
    """The expert loop of MoEFFN.forward(impl="loop"), copied: the yardstick
    the fused path's error is measured against."""
    out = torch.zeros_like(flat)
    for e in idx.unique().tolist():
        hit = (idx == e)                                # [N, k]
        rows = hit.any(-1).nonzero(as_tuple=True)[0]
        contrib = (w * hit).sum(-1)[rows].unsqueeze(-1)  # routed weight
        h = OF.glu_fused(flat[rows] @ gate_up[e].T, gelu=False)
        out[rows] += contrib * (h @ down[e].T)
    return out


@requires_gpu
@pytest.mark.parametrize("shape", [(5, 256, 256, 4, 2), (200, 192, 320, 8, 2),
                                   (64, 512, 1024, 8, 4)], ids=str)
def test_random_case_no_worse_than_the_loop(shape):
    """err = max |out - ref|, ref = fp64 math on the bf16-rounded inputs with
    the same weights / idx.  The fused path rounds to bf16 at h and at the
    output only; the loop also rounds the gate_up product, each expert's
    output, the weighted product and every accumulate, so fused must land at
    or below the loop's error — 2x only covers the maximum over a few
    thousand elements falling on different rounding patterns."""
    N, dim, ffn, E, k = shape
    g = _gen(sum(shape))
    x = torch.randn(N, dim, generator=g).to(torch.bfloat16)
    gate_up = (torch.randn(E, 2 * ffn, dim, generator=g) * 0.02).to(torch.bfloat16)
    down = (torch.randn(E, dim, ffn, generator=g) * 0.02).to(torch.bfloat16)
    logits = _randn_tie_free(N, E, sum(shape))
    xd, gd, dd = x.to(DEV), gate_up.to(DEV), down.to(DEV)
    w, idx = OF.moe_route(logits.to(DEV), k)
    want = ref.moe_ffn_ref(x.double(), gate_up.double(), down.double(),
                           w.cpu().double(), idx.cpu())
    fused = OF.moe_ffn(xd, gd, dd, w, idx)
    loop = _loop_expression(xd, gd, dd, w.to(torch.bfloat16), idx)
    err_fused = (fused.cpu().double() - want).abs().max().item()
    err_loop = (loop.cpu().double() - want).abs().max().item()
    print(f"moe_ffn random {shape}: err_fused={err_fused:.3e} "
          f"err_loop={err_loop:.3e} max|ref|={want.abs().max().item():.3e}")
    assert err_loop > 0
    assert err_fused <= 2 * err_loop


@requires_gpu
def test_two_calls_are_bitwise_equal():
    g = _gen(11)
    x = torch.randn(200, 192, generator=g).to(torch.bfloat16).to(DEV)
    gate_up = (torch.randn(8, 640, 192, generator=g) * 0.02).to(torch.bfloat16).to(DEV)
    down = (torch.randn(8, 192, 320, generator=g) * 0.02).to(torch.bfloat16).to(DEV)
    w, idx = OF.moe_route(torch.randn(200, 8, generator=g).to(DEV), 2)
    a = OF.moe_ffn(x, gate_up, down, w, idx)
    b = OF.moe_ffn(x, gate_up, down, w, idx)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------- graph

@requires_gpu
def test_fused_moeffn_replays_under_a_graph():
    """The host loop cannot be captured (it reads the routing back); the
    fused lane can, and a replay follows the routing of whatever x the
    static input holds."""
    from modal_examples_amd.models.llama.model import MoEFFN

    torch.manual_seed(0)
    moe = MoEFFN(256, 256, 4, 2, impl="fused").to(DEV, torch.bfloat16).eval()
    xs = [torch.randn(1, 8, 256, generator=_gen(20 + i)).to(torch.bfloat16).to(DEV)
          for i in range(4)]
    static_x = xs[0].clone()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                moe(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = moe(static_x)
        routes = set()
        for x in xs[1:]:
            static_x.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, moe(x))
            routes.add(tuple(OF.moe_route(moe.router(x[0]).float(), 2)[1]
                             .flatten().tolist()))
    assert len(routes) == 3, "the replays did not see different routings"


# --------------------------------------------------------------------- engine

def _engine_tokens(**kw):
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    torch.manual_seed(0)
    eng = LlamaEngine(LlamaConfig.moe_small(), device="cuda",
                      dtype=torch.bfloat16, moe_impl="fused", kv_blocks=128,
                      eos_id=-1, **kw)
    rid = eng.add_request([5, 6, 7, 8, 9], max_new_tokens=6, temperature=0.0)
    eng.run_until_done()
    return eng, eng.finished[rid].out_tokens


@functools.lru_cache(maxsize=None)
def _eager_tokens():
    return tuple(_engine_tokens(use_graph=False)[1])


@requires_gpu
def test_engine_fused_decodes_under_the_graph():
    eng, out_g = _engine_tokens(use_graph=True)
    assert eng.use_graph and eng._graph is not None
    assert len(out_g) == 6 and all(0 <= t < 1024 for t in out_g)
    out_e = _eager_tokens()
    # the criterion of test_graph_decode_matches_eager, plus the first token
    agree = sum(a == b for a, b in zip(out_g, out_e))
    assert agree >= len(out_e) - 2 and out_g[0] == out_e[0], \
        f"{out_g} vs {out_e}"


@requires_gpu
def test_engine_loop_lane_turns_the_graph_off():
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    eng = LlamaEngine(LlamaConfig.moe_small(), device="cuda",
                      dtype=torch.bfloat16, use_graph=True, kv_blocks=128,
                      eos_id=-1)
    assert eng.cfg.moe_impl == "loop" and not eng.use_graph
    rid = eng.add_request([5, 6, 7, 8, 9], max_new_tokens=3, temperature=0.0)
    eng.run_until_done()
    assert len(eng.finished[rid].out_tokens) == 3


@requires_gpu
def test_engine_fused_with_speculation_and_prefix_cache():
    _, out = _engine_tokens(spec_tokens=3, prefix_cache=True, use_graph=False)
    assert tuple(out) == _eager_tokens()
