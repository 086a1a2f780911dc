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


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _signed_rows(rows, cols, nnz, g):
    """[rows, cols] with exactly nnz entries of +-1 in every row."""
    pos = torch.rand(rows, cols, generator=g).argsort(-1)[:, :nnz]
    sign = torch.randint(0, 2, (rows, nnz), generator=g) * 2 - 1
    return torch.zeros(rows, cols, dtype=torch.long).scatter_(1, pos, sign)


def exact_case(N, dim, ffn, E, k, idx=None, seed=0):
    """Inputs on which every intermediate of the routed FFN is a small
    integer, so any correct implementation is exact whatever its summation
    order or rounding points:

      x       integers in [-2, 2], x[:, 0] = 1
      gate    every gate row is 32 in column 0, zero elsewhere: each gate
              pre-activation is exactly 32, and silu(32) == 32 in fp32
      up      three entries of +-1 per row  -> |up . x| <= 6, |h| <= 192
      down    two entries of +-1 per row    -> |y| <= 384, multiples of 32
      logits  3.0 on the chosen k experts, -4.0 elsewhere -> weights 1/k

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
        h = 32 * (x @ up[e].T)
        y = h @ down[e].T
        hit = (idx == e).any(-1)
        if hit.any():
            hmax = max(hmax, int(h[hit].abs().max()))
            ymax = max(ymax, int(y[hit].abs().max()))
        total += hit[:, None] * y
    return {
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
    assert c["hmax"] <= 192 and c["ymax"] <= 384
    assert (e != 0).double().mean() > 0.5, "case is mostly zeros"
    for name in ("x", "gate_up", "down"):
        assert c[name].dtype is torch.bfloat16
    assert torch.nn.functional.silu(torch.tensor(32.0)).item() == 32.0


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
