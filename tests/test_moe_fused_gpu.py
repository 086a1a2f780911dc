"""Fused MoE FFN on the GPU (csrc/moe.hip): routing against the stable-sort
reference (edge logits included), the exact integer cases bit for bit, the
random case element by element against a bound derived from the fp64
reference, SwiGLU tails, reproducibility, graph capture, and the engine's
fused lane.

What the bitwise cases with varied_gate=True reach, (N, dim, ffn, E, k):

  (700, 64, 64, 8, 2)      P = N*k = 1400: second trip of moe_align_kernel's
                           count and fill loops (p += 1024)
  (2200, 64, 64, 4, 1)     P = 2200: third trip
  (300, 64, 64, 128, 2)    E > 32: pad-slot loop (e += 32) trips 2..4, every
                           expert hit, tile_expert filled over 128 segments
  (260, 64, 64, 128, 2)    the same with 120 empty experts in the serial
                           prefix; 31..103 rows in the other 8
  (130, 64, 128, 64, 1)    E = 64: exactly two trips of the pad-slot loop
  (4100, 1024, 64, 4, 1)   N*dim/4 = 1 049 600 > 4096*256: the first 1024
                           threads of moe_combine_kernel take a second trip
  (4090, 1024, 64, 4, 1)   N*dim/4 = 1 047 040: grid capped at 4090, no trip

The K loop of moe_gemm_kernel (K = dim in the up GEMM, ffn in the down
GEMM) runs 64-wide chunks (NF=4) when K % 128 != 0 and 128-wide ones (NF=8)
otherwise: a body of two chunks while more than two remain, then a tail of
two chunks or of one.  test_chunk_counts_bitwise runs every (dim, ffn) of

  K      form   chunks   body trips   tail
  64     NF=4   1        0            1
  128    NF=8   1        0            1
  192    NF=4   3        1            1
  256    NF=8   2        0            2
  320    NF=4   5        2            1
  384    NF=8   3        1            1
  640    NF=8   5        2            1

on both GEMMs at once.  K % 128 != 0 means an odd number of 64-wide chunks,
so the two-chunk tail never runs in the NF=4 form; in the NF=8 form it runs
after a body trip at K = 512 and 1024, in the random case.
"""
import functools

import pytest
import torch

from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from test_moe_fused import (CHUNK_DIMS, EXACT_SHAPES, RANDOM_SHAPES,
                            SPARSE_COUNTS, VARIED_SHAPES,
                            assert_exact_case_sound, exact_case, random_case,
                            varied_case)
from test_moe_fused import _tie_free
from test_moe_fused import randn_tie_free as _randn_tie_free

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


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


EDGE_EK = [(E, k) for E in (16, 128) for k in (1, 3, 8)]


def _route_gpu(logits, k):
    w, i = OF.moe_route(logits.to(DEV), k)
    assert i.dtype is torch.int32 and w.dtype is torch.float32
    return w.cpu(), i.cpu()


def _assert_ids_valid(i, E):
    """In [0, E) and distinct within a row: what align and the GEMMs rely on
    when they index the weights with these ids."""
    assert ((i >= 0) & (i < E)).all()
    s = i.sort(-1).values
    assert (s[:, 1:] != s[:, :-1]).all()


@requires_gpu
@pytest.mark.parametrize("E,k", EDGE_EK)
def test_route_masked_experts(E, k):
    """Row t keeps m = t % (E + 1) finite logits (m = 0: none) and has -inf
    on the rest.  The stable sort puts the -inf experts behind the finite
    ones in index order, and so must the kernel: the first m ids are the
    finite experts, the rest the lowest masked ones, with weight exactly 0."""
    N = 2 * (E + 1) + 3
    logits = _randn_tie_free(N, E, 31 * E + k)
    m = torch.arange(N) % (E + 1)
    keep = torch.rand(N, E, generator=_gen(E + k)).argsort(-1) < m[:, None]
    logits[~keep] = float("-inf")
    w_ref, i_ref = ref.moe_route_ref(logits, k)
    w, i = _route_gpu(logits, k)
    _assert_ids_valid(i, E)
    assert torch.equal(i, i_ref)
    live = m >= 1
    assert (~live).sum() >= 2 and (live & (m < k)).sum() >= (2 if k > 1 else 0)
    torch.testing.assert_close(w[live], w_ref[live], atol=1e-5, rtol=0)
    assert w[~live].isnan().all() and w_ref[~live].isnan().all()
    assert torch.equal(i[~live], torch.arange(k, dtype=torch.int32)
                       .expand(int((~live).sum()), k))
    for t in (live & (m < k)).nonzero().flatten().tolist():
        assert keep[t, i[t, :m[t]].long()].all()
        assert (w[t, m[t]:] == 0).all(), t


@requires_gpu
@pytest.mark.parametrize("E,k", EDGE_EK)
def test_route_large_finite_logits(E, k):
    """+-1e4 and +-3e38 among ordinary logits: differences overflow to -inf
    and their weight is 0, equal values tie to the lower index."""
    N = 67
    g = _gen(7 * E + k)
    logits = torch.randn(N, E, generator=g)
    kind = torch.randint(0, 10, (N, E), generator=g)
    for code, v in ((0, 1e4), (1, -1e4), (2, 3e38), (3, -3e38)):
        logits[kind == code] = v
    logits[0] = 3e38
    logits[1] = -3e38
    w_ref, i_ref = ref.moe_route_ref(logits, k)
    w, i = _route_gpu(logits, k)
    assert torch.equal(i, i_ref)
    assert torch.isfinite(w).all() and (w >= 0).all()
    assert (w.double().sum(-1) - 1).abs().max() <= 1e-6
    torch.testing.assert_close(w, w_ref, atol=1e-5, rtol=0)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_route_half_precision_logits(dtype):
    """The model's router emits bf16: routing it is routing its fp32 value,
    ties (frequent at 8 bits) included."""
    for E, k in EDGE_EK:
        logits = torch.randn(130, E, generator=_gen(E + k)).to(dtype)
        assert E == 16 or not _tie_free(logits.float())
        w, i = _route_gpu(logits, k)
        w32, i32 = _route_gpu(logits.float(), k)
        assert torch.equal(i, i32) and torch.equal(w, w32)
        assert torch.equal(i, ref.moe_route_ref(logits.float(), k)[1])


@requires_gpu
@pytest.mark.parametrize("E,k", EDGE_EK)
def test_route_nan_and_inf_rows_keep_ids_valid(E, k):
    """NaN / +inf have no defined order here (torch.sort ranks NaN first,
    the kernel never prefers it), so the values are not compared: only that
    every id stays in range and distinct, and that clean rows of the same
    batch come out as they do without the bad rows."""
    N = 70
    clean = _randn_tie_free(N, E, 13 * E + k)
    logits = clean.clone()
    nan, inf = float("nan"), float("inf")
    logits[3, 0] = nan                    # NaN in the first place looked at
    logits[10, E - 1] = nan
    logits[17] = nan                      # a whole row
    logits[24, ::2] = nan
    logits[31, 1] = inf
    logits[38] = inf
    logits[45, [0, 5]] = inf
    logits[52, 2], logits[52, 7] = nan, inf
    logits[59, :] = float("-inf")
    logits[59, 4] = nan
    logits[69, 1:] = nan                  # the one live thread's neighbour
    bad = ~torch.isfinite(logits).all(-1)
    assert bad.sum() == 10
    w, i = _route_gpu(logits, k)
    _assert_ids_valid(i, E)
    w_c, i_c = _route_gpu(clean, k)
    assert torch.equal(i[~bad], i_c[~bad]) and torch.equal(w[~bad], w_c[~bad])
    assert torch.equal(i_c, ref.moe_route_ref(clean, k)[1])


@requires_gpu
def test_route_last_block_with_one_row():
    logits = _randn_tie_free(513, 16, 513)  # 3 blocks of 256, 1 live thread
    w_ref, i_ref = ref.moe_route_ref(logits, 3)
    w, i = _route_gpu(logits, 3)
    assert torch.equal(i, i_ref)
    torch.testing.assert_close(w, w_ref, atol=1e-5, rtol=0)


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


# ------------------------------------------------- exact case, varied gate

@functools.lru_cache(maxsize=None)
def _varied(shape):
    """(case, expected bf16 output); the CPU tier (test_moe_fused.py) shows
    that moe_ffn_ref reproduces `expect` for each of these shapes."""
    c = varied_case(shape)
    assert_exact_case_sound(c)
    return c, c["expect"].to(torch.bfloat16)


def _routed_bitwise(shape):
    c, want = _varied(shape)
    w, idx = OF.moe_route(c["logits"].to(DEV), shape[4])
    assert torch.equal(idx.cpu(), c["idx"])
    assert torch.equal(w.cpu(), c["weights"])
    got = _ffn_gpu(c, w, idx)
    assert got.dtype is torch.bfloat16
    bad = (got != want).any(-1).nonzero().flatten()
    assert torch.equal(got, want), \
        f"{shape}: {bad.numel()} rows differ, first {bad[:8].tolist()}"
    return c, want, got


def _assert_order_independent(c, want, got, seed):
    """The same tokens in a shuffled order: same rows out, bit for bit."""
    N = c["x"].shape[0]
    perm = torch.randperm(N, generator=_gen(seed))
    assert (perm != torch.arange(N)).float().mean() > 0.9
    got_s = _ffn_gpu(dict(c, x=c["x"][perm], idx=c["idx"][perm]))
    assert torch.equal(got_s, want[perm])
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N)
    assert torch.equal(got_s[inv], got)


@requires_gpu
@pytest.mark.parametrize("shape", VARIED_SHAPES, ids=str)
def test_varied_gate_case_bitwise(shape):
    N, dim, ffn, E, k = shape
    c, want, got = _routed_bitwise(shape)
    count = torch.bincount(c["idx"].flatten().long(), minlength=E)
    if shape == (260, 64, 64, 128, 2):
        assert {e: int(n) for e, n in enumerate(count) if n} == SPARSE_COUNTS
        assert int((count == 0).sum()) == 120
        assert count.max() > 64 and 0 < count[count > 0].min() < 32
    elif shape == (300, 64, 64, 128, 2):
        assert count.min() >= 1, "an expert is empty"
    if shape in ((700, 64, 64, 8, 2), (260, 64, 64, 128, 2)):
        _assert_order_independent(c, want, got, seed=N)


@requires_gpu
@pytest.mark.parametrize("dim", CHUNK_DIMS)
def test_chunk_counts_bitwise(dim):
    """Every chunk count of the module docstring's table in the up GEMM
    (K = dim) against every one in the down GEMM (K = ffn)."""
    for ffn in CHUNK_DIMS:
        _routed_bitwise((37, dim, ffn, 4, 2))


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
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=str)
def test_random_case_no_worse_than_the_loop(shape):
    """Two checks against ref = fp64 math on the bf16-rounded inputs with the
    same weights / idx.

    Element-wise: |out - ref| <= tol everywhere, tol from
    ref.moe_ffn_bound_ref (the worst case of the two bf16 roundings, the one
    at h propagated through the down projection).  A pipeline that
    rounds at those two points and is otherwise exact stays under 0.5 tol on
    these shapes (test_bound_leaves_the_yardstick_half), so no element is
    excused.  The worst err/tol is printed as MOE_FFN_RATIO.

    Against the loop: err = max |out - ref|.  The fused path rounds to bf16
    at h and at the output only; the loop also rounds the gate_up product,
    each expert's output, the weighted product and every accumulate, so
    fused must land at or below the loop's error — 2x only covers the
    maximum over a few thousand elements falling on different rounding
    patterns."""
    N, dim, ffn, E, k = shape
    x, gate_up, down, logits = random_case(shape)
    xd, gd, dd = x.to(DEV), gate_up.to(DEV), down.to(DEV)
    w, idx = OF.moe_route(logits.to(DEV), k)
    want, tol = ref.moe_ffn_bound_ref(x, gate_up, down, w.cpu(), idx.cpu())
    fused = OF.moe_ffn(xd, gd, dd, w, idx)
    loop = _loop_expression(xd, gd, dd, w.to(torch.bfloat16), idx)
    err = (fused.cpu().double() - want).abs()
    err_fused = err.max().item()
    err_loop = (loop.cpu().double() - want).abs().max().item()
    ratio = (err / tol).max().item()
    print(f"moe_ffn random {shape}: err_fused={err_fused:.3e} "
          f"err_loop={err_loop:.3e} max|ref|={want.abs().max().item():.3e}")
    print(f"MOE_FFN_RATIO {shape}: worst err/tol={ratio:.3f} "
          f"over {err.numel()} elements")
    assert torch.isfinite(fused).all()
    assert (err <= tol).all(), \
        f"{int((err > tol).sum())} elements outside tol, worst {ratio:.3f}"
    assert err_loop > 0
    assert err_fused <= 2 * err_loop


@requires_gpu
def test_swiglu_tails():
    """Gate pre-activations g of +-25 .. +-200 in every row: below -88,
    __expf(-g) is +inf and silu(g) * u has to come out as -0 * u = 0, not
    NaN; above +88 it is g * u.  down is dense, so each output element sums
    h over every f: one NaN in h would poison its whole row, and the
    elements stay within the bound of the random case (the exact
    contribution of an f with g < -88 is below 1e-30, far inside tol).

    Second call: every g = -200.  The exact h is 200 * e^-200 * |u| <
    1e-80, below the smallest fp32 subnormal, so every output is zero."""
    N, dim, ffn, E = 64, 64, 64, 4
    g = _gen(88)
    x = (torch.randn(N, dim, generator=g) * 0.5).to(torch.bfloat16)
    x[:, 0] = torch.tensor([1.0, -1.0, 2.0, -2.0]).repeat(N // 4)
    vals = torch.tensor([100.0, -100.0, 50.0, -50.0, 90.0, -90.0, 25.0, -25.0])
    gate = torch.zeros(E, ffn, dim)
    gate[:, :, 0] = vals[(torch.arange(E)[:, None] + torch.arange(ffn)) % 8]
    up = torch.randn(E, ffn, dim, generator=g) * 0.1
    gate_up = torch.cat([gate, up], 1).to(torch.bfloat16)
    down = (torch.randn(E, dim, ffn, generator=g) * 0.1).to(torch.bfloat16)
    idx = (torch.arange(N) // 4 % E).to(torch.int32)[:, None]
    w = torch.ones(N, 1)

    xe = x.double()
    pre = torch.einsum("td,tfd->tf", xe, gate_up[idx[:, 0].long(), :ffn].double())
    upv = torch.einsum("td,tfd->tf", xe, gate_up[idx[:, 0].long(), ffn:].double())
    low, high = pre < -88, pre > 88
    assert pre.min() == -200 and pre.max() == 200
    assert (low.sum(-1) >= 8).all() and (high.sum(-1) >= 8).all()
    h = torch.nn.functional.silu(pre) * upv
    assert h[low].abs().max() < 1e-30 and h[high].abs().max() > 100

    want, tol = ref.moe_ffn_bound_ref(x, gate_up, down, w, idx)
    assert (tol > 1e-3).all(), "an output element sees only the low tail"
    got = OF.moe_ffn(x.to(DEV), gate_up.to(DEV), down.to(DEV), w.to(DEV),
                     idx.to(DEV)).cpu()
    assert torch.isfinite(got).all()
    err = (got.double() - want).abs()
    print(f"MOE_FFN_RATIO swiglu tails: worst err/tol={(err / tol).max():.3f}")
    assert (err <= tol).all()

    x2 = x.clone()
    x2[:, 0] = 2.0
    gate_up2 = gate_up.clone()
    gate_up2[:, :ffn, 0] = -100.0
    assert (x2.double() @ gate_up2[0, :ffn].double().T == -200).all()
    got2 = OF.moe_ffn(x2.to(DEV), gate_up2.to(DEV), down.to(DEV), w.to(DEV),
                      idx.to(DEV)).cpu()
    assert not got2.isnan().any()
    assert (got2 == 0).all()


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
