"""Fused MoE FFN, the parts that need no GPU: the routing and FFN references,
the MoEFFN / LlamaEngine switch between the host loop and the fused lane,
the host-side argument checks, and the exact integer case that the GPU tests
(test_moe_fused_gpu.py) compare the kernels against bit for bit."""
import pytest
import torch

from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.models.llama.model import LlamaConfig, MoEFFN
from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref

# (N, dim, ffn, E, k) of the exact case; the GPU file runs the same three
EXACT_SHAPES = [(37, 64, 64, 4, 1), (37, 192, 320, 4, 2), (70, 64, 128, 8, 2)]

# exact cases with varied_gate=True; what each reaches in csrc/moe.hip is
# tabulated in test_moe_fused_gpu.py, which runs them on the kernels
VARIED_SHAPES = [
    (700, 64, 64, 8, 2),       # P = 1400: second trip of align's loops
    (2200, 64, 64, 4, 1),      # P = 2200: third trip
    (300, 64, 64, 128, 2),     # E > 32, every expert hit
    (260, 64, 64, 128, 2),     # E > 32, 8 experts hit (sparse_idx)
    (130, 64, 128, 64, 1),     # E = 64
    (4100, 1024, 64, 4, 1),    # N*dim/4 = 1 049 600 > 4096*256
    (4090, 1024, 64, 4, 1),    # N*dim/4 = 1 047 040 < 4096*256
]
# K of both GEMMs; 320 is there for five 64-wide chunks in the up GEMM
CHUNK_DIMS = (64, 128, 192, 256, 320, 384, 640)
CHUNK_SHAPES = [(37, d, f, 4, 2) for d in CHUNK_DIMS for f in CHUNK_DIMS]

# experts hit / rows per expert of the sparse E = 128 case: counts on both
# sides of the 32- and 64-row tile edges, the other 120 experts empty
SPARSE_COUNTS = {0: 31, 31: 33, 32: 64, 33: 65, 63: 95, 64: 97, 96: 32,
                 127: 103}

# (N, dim, ffn, E, k) of the random case, GPU and yardstick alike
RANDOM_SHAPES = [(5, 256, 256, 4, 2), (200, 192, 320, 8, 2),
                 (64, 512, 1024, 8, 4), (200, 384, 640, 8, 2),
                 (1100, 128, 192, 64, 8)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _signed_rows(rows, cols, nnz, g):
    """[rows, cols] with exactly nnz entries of +-1 in every row."""
    pos = torch.rand(rows, cols, generator=g).argsort(-1)[:, :nnz]
    sign = torch.randint(0, 2, (rows, nnz), generator=g) * 2 - 1
    return torch.zeros(rows, cols, dtype=torch.long).scatter_(1, pos, sign)


def _tie_free(t):
    v = t.sort(-1).values
    return bool((v[:, 1:] != v[:, :-1]).all())


def randn_tie_free(N, E, seed):
    """Seeded fp32 randn logits; a seed whose draw holds a tie inside a row
    (a few in a thousand at E = 128) is skipped for the next one."""
    while True:
        logits = torch.randn(N, E, generator=_gen(seed))
        if _tie_free(logits):
            return logits
        seed += 1


def random_case(shape):
    """bf16 x / gate_up / down and fp32 tie-free logits of a random shape."""
    N, dim, ffn, E, k = shape
    g = _gen(sum(shape))
    x = torch.randn(N, dim, generator=g).to(torch.bfloat16)
    gate_up = (torch.randn(E, 2 * ffn, dim, generator=g) * 0.02).to(torch.bfloat16)
    down = (torch.randn(E, dim, ffn, generator=g) * 0.02).to(torch.bfloat16)
    return x, gate_up, down, randn_tie_free(N, E, sum(shape))


def sparse_idx():
    """[260, 2] experts with SPARSE_COUNTS rows each, distinct per row: the
    520 pairs in expert order, row t taking pairs t and t + 260 (no expert
    has more than 260)."""
    flat = torch.repeat_interleave(torch.tensor(list(SPARSE_COUNTS)),
                                   torch.tensor(list(SPARSE_COUNTS.values())))
    idx = torch.stack([flat[:260], flat[260:]], 1)
    assert (idx[:, 0] != idx[:, 1]).all()
    return idx


def all_hit_idx(N, E, seed=0):
    """[N, 2] experts, every one of E hit: rows 0..E/2-1 take experts 2t and
    2t+1, the rest two random distinct ones."""
    idx = torch.rand(N, E, generator=_gen(seed)).argsort(-1)[:, :2]
    idx[:E // 2] = torch.arange(E).view(E // 2, 2)
    return idx


def varied_case(shape):
    """exact_case(varied_gate=True) of a VARIED_SHAPES / CHUNK_SHAPES entry,
    with the explicit idx the two E = 128 cases call for."""
    idx = None
    if shape == (260, 64, 64, 128, 2):
        idx = sparse_idx()
    elif shape == (300, 64, 64, 128, 2):
        idx = all_hit_idx(300, 128)
    return exact_case(*shape, idx=idx, varied_gate=True)


def exact_case(N, dim, ffn, E, k, idx=None, seed=0, varied_gate=False):
    """Inputs on which every intermediate of the routed FFN is a small
    integer, so any correct implementation is exact whatever its summation
    order or rounding points:

      x       integers in [-2, 2], x[:, 0] = 1
      gate    every gate row is 32 in column 0, zero elsewhere: each gate
              pre-activation is exactly 32, and silu(32) == 32 in fp32
      up      three entries of +-1 per row  -> |up . x| <= 6, |h| <= 192
      down    two entries of +-1 per row    -> |y| <= 384, multiples of 32
      logits  3.0 on the chosen k experts, -4.0 elsewhere -> weights 1/k

    varied_gate=True makes the gate visible to a bitwise comparison (above,
    every pre-activation is 32 whichever expert, N-tile or K-chunk of gate
    is read):

      x       also x[:, dim-1] = 1
      gate    row f of expert e has one non-zero: 32 or 64 by (e + f) % 2,
              in column 0 or column dim-1 by (e + f // 32) % 2.  Both
              columns meet a 1 of x, so the pre-activation is the value
              itself; silu(64) == 64 in fp32 as well.  The neighbouring
              expert's row f holds the other value, and a gate product that
              loses the first or the last K-chunk is 0 on every other
              32-row N-tile.
      bounds  |h| <= 384 in multiples of 32, |y| <= 768, out = sum(y) / k a
              multiple of 16: all bf16-representable integers.
      expect  computed in float64, not int64 (an int64 matmul takes seconds
              at dim 1024): every product and partial sum is an integer
              below 2^11, so float64 is exact whatever the summation order.

    idx: optional int [N, k] choice of experts (distinct per row); random
    otherwise.  Returns a dict with bf16 x / gate_up / down, fp32 logits
    and weights, int32 idx (sorted ascending per row: the order moe_route
    gives tied logits) and `expect`, the exact output in float64 computed in
    integer arithmetic."""
    assert k in (1, 2), "1/k must be exact"
    g = _gen(seed)
    x = torch.randint(-2, 3, (N, dim), generator=g)
    x[:, 0] = 1
    gate = torch.zeros(E, ffn, dim, dtype=torch.long)
    if varied_gate:
        x[:, dim - 1] = 1
        e_, f_ = torch.arange(E)[:, None], torch.arange(ffn)[None, :]
        col = ((e_ + f_ // 32) % 2) * (dim - 1)
        gate.scatter_(2, col[:, :, None], (32 + 32 * ((e_ + f_) % 2))[:, :, None])
    else:
        gate[:, :, 0] = 32
    up = torch.stack([_signed_rows(ffn, dim, 3, g) for _ in range(E)])
    down = torch.stack([_signed_rows(dim, ffn, 2, g) for _ in range(E)])
    if idx is None:
        idx = torch.rand(N, E, generator=g).argsort(-1)[:, :k]
    idx = idx.long().sort(-1).values
    logits = torch.full((N, E), -4.0).scatter_(1, idx, 3.0)

    total = torch.zeros(N, dim, dtype=torch.long)
    hmax = ymax = 0
    for e in range(E):
        hit = (idx == e).any(-1)
        if varied_gate:
            if not hit.any():
                continue
            xe = x[hit].double()
            h = (xe @ gate[e].double().T) * (xe @ up[e].double().T)
            y = (h @ down[e].double().T).long()
            hmax = max(hmax, int(h.abs().max()))
            ymax = max(ymax, int(y.abs().max()))
            total[hit] += y
            continue
        h = 32 * (x @ up[e].T)
        y = h @ down[e].T
        if hit.any():
            hmax = max(hmax, int(h[hit].abs().max()))
            ymax = max(ymax, int(y[hit].abs().max()))
        total += hit[:, None] * y
    return {
        "varied_gate": varied_gate,
        "x": x.to(torch.bfloat16),
        "gate_up": torch.cat([gate, up], 1).to(torch.bfloat16),
        "down": down.to(torch.bfloat16),
        "logits": logits,
        "weights": torch.full((N, k), 1.0 / k),
        "idx": idx.to(torch.int32),
        "expect": total.double() / k,
        "hmax": hmax, "ymax": ymax,
    }


def assert_exact_case_sound(c):
    """The properties that make a bitwise comparison on `c` meaningful."""
    e = c["expect"]
    assert torch.equal(e.to(torch.bfloat16).double(), e), \
        "expected output not representable in bf16"
    if c["varied_gate"]:
        assert c["hmax"] <= 384 and c["ymax"] <= 768
        assert (e % 16 == 0).all()
        F = c["down"].shape[2]
        g = c["gate_up"][:, :F].long()
        assert ((g != 0).sum(-1) == 1).all()
        assert sorted(g.sum(-1).unique().tolist()) == [32, 64]
    else:
        assert c["hmax"] <= 192 and c["ymax"] <= 384
    assert (e != 0).double().mean() > 0.5, "case is mostly zeros"
    for name in ("x", "gate_up", "down"):
        assert c[name].dtype is torch.bfloat16
    assert torch.nn.functional.silu(torch.tensor(32.0)).item() == 32.0
    assert torch.nn.functional.silu(torch.tensor(64.0)).item() == 64.0


# ------------------------------------------------------------ route reference

def test_route_ref_matches_topk_softmax():
    logits = torch.randn(50, 16, generator=_gen(1))
    assert all(r.unique().numel() == 16 for r in logits), "tie in the input"
    w, idx = ref.moe_route_ref(logits, 4)
    tv, ti = logits.topk(4, dim=-1)
    assert idx.dtype is torch.int32 and torch.equal(idx.long(), ti)
    torch.testing.assert_close(w, torch.softmax(tv, -1))
    w2, idx2 = OF.moe_route(logits, 4)  # CPU dispatch = the reference
    assert torch.equal(idx2, idx) and torch.equal(w2, w)


def test_route_ref_tie_takes_lower_index():
    logits = torch.tensor([[1.0, 1.0, 1.0, 1.0],     # whole row equal
                           [0.0, 2.0, 1.0, 1.0],     # tie across the k-th place
                           [1.0, 0.0, 1.0, 3.0]])
    _, idx = ref.moe_route_ref(logits, 2)
    assert idx.tolist() == [[0, 1], [1, 2], [3, 0]]


# -------------------------------------------------------------- FFN reference

def _moe(impl, dim=64, ffn=128, E=4, k=2, seed=0):
    torch.manual_seed(seed)
    return MoEFFN(dim, ffn, E, k, impl=impl)


def test_ffn_ref_matches_loop_fp32():
    m = _moe("loop")
    x = torch.randn(2, 9, 64, generator=_gen(2))
    with torch.no_grad():
        want = m(x)
        w, idx = ref.moe_route_ref(m.router(x.reshape(-1, 64)), 2)
        got = ref.moe_ffn_ref(x.reshape(-1, 64), m.gate_up, m.down, w, idx)
    torch.testing.assert_close(got.view_as(want), want)


def test_ffn_ref_gradients_flow():
    m = _moe("loop")
    x = torch.randn(11, 64, generator=_gen(3), requires_grad=True)
    w, idx = OF.moe_route(m.router(x), 2)
    OF.moe_ffn(x, m.gate_up, m.down, w, idx).square().sum().backward()
    for t in (x, m.gate_up, m.down, m.router.weight):
        assert t.grad is not None and torch.isfinite(t.grad).all()
        assert t.grad.abs().max() > 0


# --------------------------------------------------------------- model switch

def test_moeffn_fused_matches_loop_fp32():
    loop, fused = _moe("loop"), _moe("fused")
    fused.load_state_dict(loop.state_dict())
    x = torch.randn(3, 7, 64, generator=_gen(4))
    with torch.no_grad():
        torch.testing.assert_close(fused(x), loop(x))


def _greedy(moe_impl):
    torch.manual_seed(0)
    eng = LlamaEngine(LlamaConfig.moe_small(), device="cpu",
                      dtype=torch.float32, kv_blocks=64, eos_id=-1,
                      moe_impl=moe_impl)
    rid = eng.add_request([5, 6, 7, 8, 9], max_new_tokens=6, temperature=0.0)
    eng.run_until_done()
    return eng, eng.finished[rid].out_tokens


def test_engine_fused_emits_loop_tokens_fp32():
    eng_l, loop = _greedy("loop")
    eng_f, fused = _greedy("fused")
    assert eng_l.model.blocks[0].moe.impl == "loop"
    assert eng_f.model.blocks[0].moe.impl == "fused"
    assert len(loop) == 6 and fused == loop


def test_engine_moe_impl_default_and_bad_value():
    eng, _ = _greedy(None)  # None keeps the config's lane
    assert eng.cfg.moe_impl == "loop"
    assert eng.model.blocks[0].moe.impl == "loop"
    with pytest.raises(ValueError, match="moe_impl"):
        LlamaEngine(LlamaConfig.moe_small(), device="cpu",
                    dtype=torch.float32, kv_blocks=64, moe_impl="grouped")
    with pytest.raises(ValueError, match="impl"):
        MoEFFN(64, 64, 4, 2, impl="grouped")


# ------------------------------------------------------------ argument checks

def _ffn_args(dim=64, ffn=64, E=4, k=2, N=5):
    return dict(x=torch.zeros(N, dim), gate_up=torch.zeros(E, 2 * ffn, dim),
                down=torch.zeros(E, dim, ffn), weights=torch.zeros(N, k),
                idx=torch.arange(k, dtype=torch.int32).repeat(N, 1))


def test_route_argument_checks_name_the_argument():
    with pytest.raises(ValueError, match="top_k"):
        OF.moe_route(torch.zeros(3, 16), 9)
    with pytest.raises(ValueError, match="top_k"):
        OF.moe_route(torch.zeros(3, 4), 5)
    with pytest.raises(ValueError, match="logits.*E=129"):
        OF.moe_route(torch.zeros(3, 129), 2)
    with pytest.raises(ValueError, match="logits"):
        OF.moe_route(torch.zeros(3, 4, 2), 2)


def test_ffn_argument_checks_name_the_argument():
    OF.moe_ffn(**_ffn_args())  # the base arguments are accepted
    with pytest.raises(ValueError, match="x has dim=96"):
        OF.moe_ffn(**_ffn_args(dim=96))
    with pytest.raises(ValueError, match="ffn_dim=32"):
        OF.moe_ffn(**_ffn_args(ffn=32))
    with pytest.raises(ValueError, match="gate_up has E=129"):
        OF.moe_ffn(**_ffn_args(E=129))
    with pytest.raises(ValueError, match="idx.*top_k"):
        OF.moe_ffn(**_ffn_args(E=16, k=9))
    a = _ffn_args()
    a["idx"] = a["idx"].long()
    with pytest.raises(TypeError, match="idx must be int32"):
        OF.moe_ffn(**a)
    a = _ffn_args()
    a["gate_up"] = torch.zeros(4, 64, 128).transpose(1, 2)
    with pytest.raises(ValueError, match="gate_up must be contiguous"):
        OF.moe_ffn(**a)
    a = _ffn_args()
    a["down"] = torch.zeros(4, 64, 128)[:, :, ::2]
    with pytest.raises(ValueError, match="down must be contiguous"):
        OF.moe_ffn(**a)
    a = _ffn_args()
    a["weights"] = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="weights"):
        OF.moe_ffn(**a)


# ------------------------------------------------------------ exact int case

@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=str)
def test_exact_case_is_exact_on_the_reference(shape):
    c = exact_case(*shape)
    assert_exact_case_sound(c)
    w, idx = ref.moe_route_ref(c["logits"], shape[4])
    assert torch.equal(idx, c["idx"]) and torch.equal(w, c["weights"])
    out = ref.moe_ffn_ref(c["x"], c["gate_up"], c["down"], w, idx)
    assert out.dtype is torch.bfloat16
    assert torch.equal(out.double(), c["expect"])


@pytest.mark.parametrize("shape", VARIED_SHAPES + CHUNK_SHAPES, ids=str)
def test_varied_gate_case_is_exact_on_the_reference(shape):
    N, dim, ffn, E, k = shape
    c = varied_case(shape)
    assert_exact_case_sound(c)
    assert (c["x"][:, 0] == 1).all() and (c["x"][:, dim - 1] == 1).all()
    w, idx = ref.moe_route_ref(c["logits"], k)
    assert torch.equal(idx, c["idx"]) and torch.equal(w, c["weights"])
    out = ref.moe_ffn_ref(c["x"], c["gate_up"], c["down"], w, idx)
    assert out.dtype is torch.bfloat16
    assert torch.equal(out.double(), c["expect"])


def test_varied_gate_pattern():
    """Row f of expert e: value by (e + f) % 2, column by (e + f//32) % 2."""
    c = exact_case(37, 192, 128, 4, 2, varied_gate=True)
    gate = c["gate_up"][:, :128].long()
    for e, f, col, val in [(0, 0, 0, 32), (0, 1, 0, 64), (0, 32, 191, 32),
                           (0, 33, 191, 64), (1, 0, 191, 64), (1, 31, 191, 32),
                           (1, 32, 0, 64), (2, 64, 0, 32), (3, 127, 0, 32)]:
        assert gate[e, f, col] == val and gate[e, f].sum() == val, (e, f)
    # the default case is untouched by the option
    a, b = exact_case(37, 192, 128, 4, 2), exact_case(37, 192, 128, 4, 2,
                                                      varied_gate=False)
    assert all(torch.equal(a[n], b[n]) for n in ("x", "gate_up", "down",
                                                 "logits", "idx", "expect"))
    assert (a["gate_up"][:, :128, 0] == 32).all()
    assert a["gate_up"][:, :128, 1:].abs().sum() == 0


def test_varied_gate_case_sees_what_the_uniform_gate_hides():
    """Three wrong gate products, made by editing the reference's inputs:
    the neighbouring expert's gate rows, and a gate that loses its first or
    its last K-chunk.  Each moves the varied case's output; the first leaves
    the uniform case's output bit for bit the same, which is the gap the
    variant closes."""
    shape = (37, 192, 128, 4, 2)
    N, dim, ffn, E, k = shape

    def run(c, gate_up):
        return ref.moe_ffn_ref(c["x"], gate_up, c["down"], c["weights"],
                               c["idx"]).double()

    def swapped(c):
        gu = c["gate_up"].clone()
        gu[:, :ffn] = c["gate_up"][torch.arange(E) ^ 1, :ffn]
        return gu

    def chunk_lost(c, lo):
        gu = c["gate_up"].clone()
        gu[:, :ffn, lo:lo + 64] = 0
        return gu

    u = exact_case(*shape)
    assert torch.equal(run(u, swapped(u)), u["expect"])
    v = exact_case(*shape, varied_gate=True)
    assert torch.equal(run(v, v["gate_up"]), v["expect"])
    for wrong in (swapped(v), chunk_lost(v, 0), chunk_lost(v, dim - 64)):
        got = run(v, wrong)
        assert (got != v["expect"]).any(-1).double().mean() > 0.9


def test_sparse_and_all_hit_idx():
    idx = sparse_idx()
    count = torch.bincount(idx.flatten(), minlength=128)
    assert {e: int(n) for e, n in enumerate(count) if n} == SPARSE_COUNTS
    assert int((count == 0).sum()) == 120
    rows = sorted(SPARSE_COUNTS.values())
    assert rows[0] < 32 and 32 in rows and 32 < rows[2] < 64
    assert 64 in rows and rows[-1] > 64
    idx = all_hit_idx(300, 128)
    assert (idx[:, 0] != idx[:, 1]).all()
    assert torch.bincount(idx.flatten(), minlength=128).min() >= 1


# -------------------------------------------------- bound of the random case

@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=str)
def test_bound_leaves_the_yardstick_half(shape):
    """ref.moe_ffn_bound_ref's tol against a yardstick that does what a
    correct bf16 kernel must: the same fp64 pipeline with h and the output
    rounded to bf16.  It has to stay within half of tol on every element
    (it uses 0.13 to 0.28), so a kernel outside tol is wrong, not unlucky."""
    x, gate_up, down, logits = random_case(shape)
    w, idx = ref.moe_route_ref(logits, shape[4])
    want, tol = ref.moe_ffn_bound_ref(x, gate_up, down, w, idx)
    assert want.dtype is torch.float64 and tol.dtype is torch.float64
    plain = ref.moe_ffn_ref(x.double(), gate_up.double(), down.double(),
                            w.double(), idx)
    torch.testing.assert_close(want, plain, rtol=1e-12, atol=1e-15)
    assert (tol > 0).all() and (tol >= 2 * 2.0 ** -9 * want.abs()).all()
    yard, _ = ref.moe_ffn_bound_ref(x, gate_up, down, w, idx,
                                    bf16_points=True)
    assert torch.equal(yard.to(torch.bfloat16).double(), yard)
    ratio = ((yard - want).abs() / tol).max().item()
    print(f"MOE_FFN_YARD {shape}: worst err/tol={ratio:.3f}")
    assert 0 < ratio <= 0.5
