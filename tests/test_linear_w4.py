"""Int4 weight-only linear on the CPU: the quantizer and its packing against
an independent fp64 computation, the bound of the GPU tests and its
yardstick, the exact cases with their soundness proof, and the engine's
weight_dtype="int4" lane in fp32.  The case builders here are shared with
tests/test_linear_w4_gpu.py."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.models.llama.model import (QUANT_PROJECTIONS,
                                                   LlamaBlock, LlamaConfig,
                                                   QuantLinear)
from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref

G = 128

# ------------------------------------------------------------ case builders

EXACT_M = (1, 31, 32, 33, 65)
EXACT_N = (64, 192)
# one K per count of 128-wide chunks in a slice that takes its own path
# through the pipelined loop (table: tests/test_linear_w4_gpu.py)
EXACT_K = (128, 256, 384, 512, 640)
EXACT_SCALES = (0.25, 0.5, 1.0)
RANDOM_SHAPES = ((1, 64, 128), (7, 128, 1024), (32, 256, 4096),
                 (64, 64, 2048))
YARDSTICK_K = (128, 1024, 4096, 14336)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def exact_offsets(M):
    """Offsets `off` whose exact_case(M, ..., off=off) together put a
    non-zero on every k position of a group: 4 per row, 128 to cover."""
    return tuple(range(0, 32, M)) if M < 32 else (0,)


def exact_case(M, N, K, seed, off=0):
    """x bf16 [M, K] with 4 non-zeros per row from {+-1, +-2}; scales from
    {0.25, 0.5, 1}; q uniform in [-8, 7].  Non-zero i of row m sits at
    position (4*(m + off) + i) % 128 of group (m + off + i) % (K/128)."""
    g = _gen(seed)
    ng = K // G
    x = torch.zeros(M, K)
    vals = torch.tensor([1.0, -1.0, 2.0, -2.0])
    for m in range(M):
        for i in range(4):
            k = ((m + off + i) % ng) * G + (4 * (m + off) + i) % G
            x[m, k] = vals[torch.randint(0, 4, (1,), generator=g)]
    q = torch.randint(-8, 8, (N, K), generator=g)
    sc = torch.tensor(EXACT_SCALES)[torch.randint(0, 3, (N, ng), generator=g)]
    return {"x": x.to(torch.bfloat16), "q": q,
            "qweight": ref.w4_pack(q), "scales": sc.to(torch.bfloat16)}


def dense_case(M, N, K, seed):
    """{-1, 0, 1} activations against {-1, 0, 1} weights at scale 1."""
    g = _gen(seed)
    x = torch.randint(-1, 2, (M, K), generator=g).float()
    q = torch.randint(-1, 2, (N, K), generator=g)
    return {"x": x.to(torch.bfloat16), "q": q, "qweight": ref.w4_pack(q),
            "scales": torch.ones(N, K // G, dtype=torch.bfloat16)}


def exact_want(c):
    """The exact product of a case in fp64 -> bf16 (no rounding happens:
    assert_exact_case_sound shows it)."""
    w = c["q"].double().view(c["q"].shape[0], -1, G) \
        * c["scales"].double().unsqueeze(-1)
    y = c["x"].double() @ w.view(c["q"].shape).T
    return y.to(torch.bfloat16)


def assert_exact_case_sound(c):
    """Any fp32 evaluation of the case is exact, whatever its order, in the
    plain form (operand q) and in the kernel's biased form (operand
    128 + nibble = 136 + q, bias removed per group).  With unit = the
    smallest scale, every term is an integer multiple of unit, and the sum
    of the terms' magnitudes stays below 2^24 units, so every partial sum of
    every order is an integer below 2^24 in units of `unit`: representable.
    The outputs round-trip through bf16."""
    x = c["x"].double()
    M, K = x.shape
    N, ng = c["scales"].shape
    s = c["scales"].double()
    unit = float(s.min())
    q = c["q"].double()
    assert torch.equal(x, x.round()) and torch.equal(s / unit,
                                                     (s / unit).round())
    xg = x.abs().view(M, ng, G)
    total = torch.zeros(M, N, dtype=torch.float64)
    for g in range(ng):
        qg = q[:, g * G:(g + 1) * G]
        plain = xg[:, g] @ qg.abs().T            # sum |x| |q|
        biased = xg[:, g] @ (qg + 136).abs().T   # sum |x| (136 + q)
        rowsum = xg[:, g].sum(-1, keepdim=True)  # sum |x|
        # biased form: the group sums P and X and the product 136 * X are
        # integers below 2^24, so P - 136 X is exact too
        assert float(biased.max()) < 2 ** 24
        assert float(136 * rowsum.max()) < 2 ** 24
        # both forms: the group's contribution s * (sum x q), in units, is
        # bounded by s / unit * sum |x||q|; so is every partial sum of the
        # plain form, within the group and over the groups
        total += s[:, g] / unit * plain
    assert float(total.max()) < 2 ** 24
    w = (q.view(N, ng, G) * s.unsqueeze(-1)).view(N, K)
    y = c["x"].double() @ w.T
    assert torch.equal(y.to(torch.bfloat16).double(), y)
    return y


def random_case(M, N, K, seed):
    g = _gen(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16)
    qweight, scales = OF.quantize_w4(w)
    return {"x": x, "w": w, "qweight": qweight, "scales": scales}


# ---------------------------------------------------------------- quantizer

def _bf16_rne(a32):
    """fp32 numpy array -> nearest bf16 (ties to even) as fp32, by bits."""
    u = a32.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def _definition(w):
    """(scale, q, w_hat) of the quantization rule, straight from its
    definition with numpy: scale = bf16(fp32(absmax) / 7), 1 where zero;
    q = clamp(rint(w / scale), -8, 7) in fp64; w_hat = scale * q."""
    a = w.double().numpy()
    N, K = a.shape
    grp = a.reshape(N, K // G, G)
    amax = np.abs(grp).max(-1).astype(np.float32)
    scale = _bf16_rne(amax / np.float32(7.0)).astype(np.float64)
    scale[scale == 0] = 1.0
    q = np.clip(np.rint(grp / scale[:, :, None]), -8, 7)
    return scale, q.reshape(N, K), (q * scale[:, :, None]).reshape(N, K)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_matches_the_definition(dtype):
    w = (0.02 * torch.randn(128, 512, generator=_gen(1))).to(dtype)
    w[3, 128:256] = 0                       # an all-zero group
    w[5] = 0                                # a whole zero row
    qweight, scales = OF.quantize_w4(w)
    assert qweight.dtype is torch.int32 and qweight.shape == (128, 64)
    assert scales.dtype is torch.bfloat16 and scales.shape == (128, 4)
    scale, q, w_hat = _definition(w)
    assert torch.equal(scales.double(), torch.from_numpy(scale))
    assert float(scales[3, 1]) == 1.0 and (scales[5] == 1).all()
    assert torch.equal(ref.w4_unpack(qweight).double(), torch.from_numpy(q))
    got = OF.dequantize_w4(qweight, scales)
    assert got.dtype is torch.float32
    assert torch.equal(got.double(), torch.from_numpy(w_hat))
    assert (got[3, 128:256] == 0).all() and (got[5] == 0).all()
    # the uint8 view of the same bytes is the same weight
    assert torch.equal(OF.dequantize_w4(qweight.view(torch.uint8), scales),
                       got)


def test_pack_roundtrips_every_nibble_at_every_position():
    """Row r holds value ((k + r) % 16) - 8 at position k: over 16 rows
    every value meets every position of a word and of a 128-group."""
    N, K = 64, 256
    k = torch.arange(K)[None, :]
    r = torch.arange(N)[:, None]
    q = ((k + r) % 16 - 8).to(torch.int32)
    seen = {(int(v), p) for row in q[:16] for p, v in enumerate(row[:G])}
    assert len(seen) == 16 * G
    packed = ref.w4_pack(q)
    assert packed.dtype is torch.int32 and packed.shape == (N, K // 8)
    assert torch.equal(ref.w4_unpack(packed), q)
    ones = torch.ones(N, K // G, dtype=torch.bfloat16)
    assert torch.equal(OF.dequantize_w4(packed, ones), q.float())
    # the documented order: k offset j at nibble j/2 (even j), 4 + j/2 (odd)
    word = int(packed[0, 0]) & 0xFFFFFFFF
    for j in range(8):
        pos = j // 2 if j % 2 == 0 else 4 + j // 2
        assert (word >> (4 * pos)) & 0xF == int(q[0, j]) + 8


def test_absmax_on_a_bf16_rounding_boundary():
    """absmax / 7 = 1 + 2^-8 is a bf16 tie and rounds DOWN to 1.0, so the
    largest quotient is 7.027, not 7.  For normal numbers the scale is off
    by at most 2^-8 of itself, the quotient stays below 7.5 and rounds to
    7.  A subnormal scale is off by more: absmax = 10 * 2^-133 has
    absmax / 7 = 1.43 * 2^-133, the nearest bf16 is 2^-133, and the
    quotient is 10 — there the clamp is what keeps q in [-8, 7]."""
    tiny = 2.0 ** -133
    w = torch.zeros(64, 256)
    w[0, 0] = 7.0 * (1 + 2.0 ** -8)
    w[0, 1] = -w[0, 0]
    w[1, 0] = 10 * tiny
    w[1, 1] = -10 * tiny
    w[1, 2] = 3 * tiny
    w[2, :128] = torch.linspace(-1, 1, 128) * 3.3
    assert float(w[1, 0]) == 10 * tiny            # no flush to zero here
    qweight, scales = OF.quantize_w4(w)
    assert float(scales[0, 0]) == 1.0 and float(scales[1, 0]) == tiny
    q = ref.w4_unpack(qweight)
    assert int(q.min()) == -8 and int(q.max()) == 7
    assert q[0, :2].tolist() == [7, -7]
    assert q[1, :3].tolist() == [7, -8, 3]
    unclamped = torch.round(w.double()[1, :2] / tiny)
    assert unclamped.tolist() == [10.0, -10.0]    # what the clamp removes
    scale, qd, w_hat = _definition(w)
    assert torch.equal(q.double(), torch.from_numpy(qd))
    assert torch.equal(OF.dequantize_w4(qweight, scales).double(),
                       torch.from_numpy(w_hat))


def test_argument_checks_raise():
    good = torch.zeros(64, 128)
    with pytest.raises(ValueError, match="multiple of 128"):
        OF.quantize_w4(torch.zeros(64, 192))
    with pytest.raises(ValueError, match="multiple of 64"):
        OF.quantize_w4(torch.zeros(96, 128))
    with pytest.raises(ValueError, match="contiguous"):
        OF.quantize_w4(torch.zeros(128, 64).T)
    with pytest.raises(ValueError):
        OF.quantize_w4(torch.zeros(2, 64, 128))
    with pytest.raises(TypeError):
        OF.quantize_w4(good.to(torch.float16))
    qw, sc = OF.quantize_w4(good)
    x = torch.zeros(3, 128)
    with pytest.raises(TypeError, match="bf16"):
        OF.linear_w4(x, qw, sc.float())
    with pytest.raises(TypeError, match="int32 or uint8"):
        OF.linear_w4(x, qw.long(), sc)
    with pytest.raises(ValueError, match="scales must be"):
        OF.linear_w4(x, qw, sc[:32].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        OF.dequantize_w4(torch.zeros(16, 64, dtype=torch.int32).T, sc)
    with pytest.raises(ValueError, match="K=128"):
        OF.linear_w4(torch.zeros(3, 256), qw, sc)
    with pytest.raises(ValueError, match="multiple of 128"):
        OF.dequantize_w4(torch.zeros(64, 24, dtype=torch.int32),
                         torch.ones(64, 1, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="multiple of 64"):
        OF.dequantize_w4(torch.zeros(32, 16, dtype=torch.int32),
                         torch.ones(32, 1, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="no rows"):
        OF.linear_w4(torch.zeros(0, 128), qw, sc)
    with pytest.raises(TypeError, match="floating"):
        OF.linear_w4(torch.zeros(3, 128, dtype=torch.int32), qw, sc)
    with pytest.raises(ValueError, match="is on"):
        OF.linear_w4(x, qw, sc.to("meta"))


# -------------------------------------------------------------------- bound

@pytest.mark.parametrize("K", YARDSTICK_K)
def test_bound_leaves_the_yardstick_half(K):
    """The fp64 product with only its output rounded to bf16 uses at most
    half of tol on every element (2^-8 |want| against 2^-7 |want| + ...)."""
    worst = 0.0
    for seed in range(3):
        c = random_case(5, 64, K, 100 * seed + K)
        want, tol = ref.linear_w4_bound_ref(c["x"], c["qweight"], c["scales"])
        pts, tol2 = ref.linear_w4_bound_ref(c["x"], c["qweight"], c["scales"],
                                            bf16_points=True)
        assert torch.equal(tol, tol2) and want.dtype is torch.float64
        A = c["x"].double().abs() @ OF.dequantize_w4(
            c["qweight"], c["scales"]).double().abs().T
        assert torch.equal(tol, 2.0 ** -7 * want.abs() + 2.0 ** -10 * A)
        ratio = (pts - want).abs() / tol
        assert bool((ratio <= 0.5).all()), float(ratio.max())
        worst = max(worst, float(ratio.max()))
    print(f"K={K}: worst yardstick ratio {worst:.3f}")


@pytest.mark.parametrize("K", (128, 1024, 4096))
def test_biased_form_in_fp32_stays_inside_the_bound(K):
    """The kernel's arithmetic replayed in fp32 on the CPU: per group
    P = x . (136 + q), X = sum x, acc += s * (P - 136 X), one rounding to
    bf16 at the end."""
    c = random_case(5, 64, K, 7 + K)
    x = c["x"].float()
    q = ref.w4_unpack(c["qweight"]).float()
    s = c["scales"].float()
    acc = torch.zeros(x.shape[0], q.shape[0])
    for g in range(K // G):
        xg, qg = x[:, g * G:(g + 1) * G], q[:, g * G:(g + 1) * G]
        P = xg @ (qg + 136.0).T
        X = xg.sum(-1, keepdim=True)
        acc = acc + s[:, g] * (P - 136.0 * X)
    got = acc.to(torch.bfloat16).double()
    want, tol = ref.linear_w4_bound_ref(c["x"], c["qweight"], c["scales"])
    ratio = (got - want).abs() / tol
    assert bool((ratio <= 1).all()), float(ratio.max())
    print(f"K={K}: worst biased-form ratio {float(ratio.max()):.3f}")


# -------------------------------------------------------------- exact cases

def _reference(c):
    return OF.linear_w4(c["x"], c["qweight"], c["scales"])


@pytest.mark.parametrize("K", EXACT_K)
def test_exact_cases_are_sound_and_cover_every_position(K):
    for M in EXACT_M:
        hit_pos, hit_grp = set(), set()
        for off in exact_offsets(M):
            c = exact_case(M, 64, K, seed=K + M, off=off)
            y = assert_exact_case_sound(c)
            assert float(y.abs().max()) <= 64
            assert torch.equal(y * 4, (y * 4).round())
            nz = c["x"].float().abs().gt(0)
            assert int(nz.sum(-1).max()) <= 4
            cols = nz.any(0).nonzero().flatten().tolist()
            hit_pos |= {k % G for k in cols}
            hit_grp |= {k // G for k in cols}
        assert hit_pos == set(range(G)), (M, K)
        assert hit_grp == set(range(K // G)), (M, K)


@pytest.mark.parametrize("N", EXACT_N)
def test_reference_reproduces_exact_cases_bitwise(N):
    for K in EXACT_K:
        for M in EXACT_M:
            c = exact_case(M, N, K, seed=K + M)
            got = _reference(c)
            assert got.dtype is torch.bfloat16 and got.shape == (M, N)
            assert torch.equal(got, exact_want(c)), (M, N, K)


@pytest.mark.parametrize("K", (128, 256))
def test_dense_case_is_sound_and_reproduced_bitwise(K):
    c = dense_case(33, 64, K, seed=K)
    y = assert_exact_case_sound(c)
    assert float(y.abs().max()) <= 256 and torch.equal(y, y.round())
    assert float(y.abs().max()) > 8   # not a degenerate case
    assert torch.equal(_reference(c), exact_want(c))


def test_grad_reaches_x_through_a_quantized_base():
    c = random_case(4, 64, 256, 3)
    x = c["x"].float().requires_grad_()
    y = OF.linear_w4(x, c["qweight"], c["scales"])
    y.sum().backward()
    w_hat = OF.dequantize_w4(c["qweight"], c["scales"])
    torch.testing.assert_close(x.grad, w_hat.sum(0).expand(4, -1))
    # batched leading dimensions
    x3 = torch.randn(2, 3, 256)
    assert OF.linear_w4(x3, c["qweight"], c["scales"]).shape == (2, 3, 64)


# ------------------------------------------------------------------- engine

PROMPTS = ([1, 17, 99, 250, 31], [5, 6, 7], [900, 3, 3, 3, 3, 3, 44, 2, 8])


def make_engine(**kw):
    kw.setdefault("kv_blocks", 128)
    kw.setdefault("cfg", LlamaConfig.small())
    return LlamaEngine(device="cpu", dtype=torch.float32, use_graph=False,
                       eos_id=-1, **kw)


def greedy(eng, n=8):
    rids = [eng.add_request(list(p), max_new_tokens=n) for p in PROMPTS]
    eng.run_until_done()
    return [eng.finished[r].out_tokens for r in rids]


def _quant_modules(eng):
    return [getattr(b, n) for b in eng.model.blocks for n in QUANT_PROJECTIONS]


@pytest.fixture(scope="module")
def int4_tokens():
    return greedy(make_engine(weight_dtype="int4"))


def test_engine_int4_equals_engine_on_dequantized_weights(int4_tokens):
    eng = make_engine()
    with torch.no_grad():
        for lin in _quant_modules(eng):
            assert isinstance(lin, torch.nn.Linear)
            q, s = OF.quantize_w4(lin.weight.detach().contiguous())
            lin.weight.copy_(OF.dequantize_w4(q, s))
    assert greedy(eng) == int4_tokens
    assert all(len(t) == 8 for t in int4_tokens)


def test_engine_int4_modules_and_bytes():
    eng = make_engine(weight_dtype="int4")
    mods = _quant_modules(eng)
    assert all(isinstance(m, QuantLinear) for m in mods)
    assert all(m.qweight.dtype is torch.int32
               and m.scales.dtype is torch.bfloat16 for m in mods)
    assert isinstance(eng.model.lm_head, torch.nn.Linear)
    n_weights = sum(m.in_features * m.out_features for m in mods)
    sd = eng.model.state_dict()
    packed = sum(v.numel() * v.element_size() for k, v in sd.items()
                 if k.endswith((".qweight", ".scales")))
    assert packed * 128 == n_weights * (64 + 2)   # 1/2 B + 2/128 B a weight
    assert not any(k.endswith(tuple(f"{n}.weight" for n in QUANT_PROJECTIONS))
                   for k in sd)
    ref_sd = make_engine().model.to(torch.bfloat16).state_dict()
    bf16 = sum(v.numel() * v.element_size() for k, v in ref_sd.items()
               if k.endswith(tuple(f"{n}.weight" for n in QUANT_PROJECTIONS)))
    assert bf16 == 2 * n_weights
    assert math.isclose(bf16 / packed, 2 / (0.5 + 2 / 128))
    # module.to(dtype) leaves the format alone
    eng.model.to(torch.float32)
    assert all(m.scales.dtype is torch.bfloat16 for m in mods)


def test_safetensors_round_trip(tmp_path, int4_tokens):
    path = str(tmp_path / "int4.safetensors")
    make_engine(weight_dtype="int4").save_safetensors(path)
    for kw in ({}, {"weight_dtype": "int4"}):
        eng = LlamaEngine.from_safetensors(
            path, LlamaConfig.small(), device="cpu", dtype=torch.float32,
            use_graph=False, eos_id=-1, kv_blocks=128, **kw)
        assert eng.weight_dtype == "int4"
        assert all(isinstance(m, QuantLinear) for m in _quant_modules(eng))
        assert greedy(eng) == int4_tokens
    with pytest.raises(ValueError, match="int4 weights"):
        LlamaEngine.from_safetensors(
            path, LlamaConfig.small(), device="cpu", dtype=torch.float32,
            use_graph=False, kv_blocks=128, weight_dtype="bf16")

    class FakeTP:
        world, rank = 2, 0

    with pytest.raises(ValueError, match="tensor parallelism"):
        LlamaEngine.from_safetensors(
            path, LlamaConfig.small(), device="cpu", dtype=torch.float32,
            use_graph=False, kv_blocks=128, tp=FakeTP())


def test_bf16_file_boots_as_int4(tmp_path, int4_tokens):
    path = str(tmp_path / "full.safetensors")
    make_engine().save_safetensors(path)
    eng = LlamaEngine.from_safetensors(
        path, LlamaConfig.small(), device="cpu", dtype=torch.float32,
        use_graph=False, eos_id=-1, kv_blocks=128, weight_dtype="int4")
    assert all(isinstance(m, QuantLinear) for m in _quant_modules(eng))
    assert greedy(eng) == int4_tokens


def test_engine_refuses_what_int4_does_not_cover():
    with pytest.raises(ValueError, match="weight_dtype"):
        make_engine(weight_dtype="int8")
    with pytest.raises(ValueError, match="MoE"):
        make_engine(cfg=LlamaConfig.moe_small(), weight_dtype="int4")
    # a TP shard whose K is no multiple of 128: down has K = 384 / 2 = 192
    cfg = dataclasses.replace(LlamaConfig.small(), ffn_dim=384)
    with pytest.raises(ValueError, match="multiple of the int4 group size"):
        LlamaBlock(cfg, tp_world=2, weight_dtype="int4")
    LlamaBlock(cfg, tp_world=1, weight_dtype="int4")   # K = 384 is fine

    class FakeTP:
        world, rank = 2, 0

        def all_reduce(self, t):
            return t

    with pytest.raises(ValueError, match="multiple of the int4 group size"):
        make_engine(cfg=cfg, tp=FakeTP(), weight_dtype="int4")
    with pytest.raises(ValueError, match="multiple of the int4 group size"):
        make_engine(cfg=cfg, tp=FakeTP(), weight_dtype="int4",
                    init_weights=False)


def test_quant_linear_lanes_agree_in_fp32():
    """Above M_KERNEL rows the forward dequantizes and calls the GEMM; in
    fp32 that is the same product as the kernel lane's reference."""
    lin = torch.nn.Linear(256, 64, bias=False)
    ql = QuantLinear.from_linear(lin)
    x = torch.randn(QuantLinear.M_KERNEL + 5, 256)
    w_hat = OF.dequantize_w4(ql.qweight, ql.scales)
    assert torch.equal(ql(x), torch.nn.functional.linear(x, w_hat))
    assert torch.equal(ql(x[:3]), torch.nn.functional.linear(x[:3], w_hat))
    with pytest.raises(ValueError, match="no bias"):
        QuantLinear.from_linear(torch.nn.Linear(256, 64))
