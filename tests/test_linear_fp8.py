"""FP8 W8A8 linear on the CPU: the weight quantizer, the reference
composition behind ops.linear_fp8, Fp8Linear and the weight_dtype="fp8" model.
The case builders here are shared with tests/test_linear_fp8_gpu.py."""
import pytest
import torch

from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.models.llama.model import (QUANT_PROJECTIONS,
                                                   Fp8Linear, LlamaConfig,
                                                   LlamaModel,
                                                   quantize_llama_fp8_,
                                                   quantize_llama_fp8_state)
from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref

FP8 = torch.float8_e4m3fn

EXACT_M = (1, 31, 32, 33, 64, 65)
EXACT_N = (64, 192)
EXACT_K = (128, 256, 384, 512, 640)   # table: tests/test_linear_fp8_gpu.py
RANDOM_SHAPES = ((1, 64, 128), (33, 192, 640), (65, 128, 1024),
                 (7, 256, 4096))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pick(values, shape, g):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def exact_offsets(M):
    """Offsets that together put a non-zero on every k of a chunk."""
    return tuple(range(0, 32, M)) if M < 32 else (0,)


def exact_case(M, N, K, seed, off=0, dense=False):
    """xq with 4 non-zeros per row from {+-1, +-2} — non-zero i of row m at
    position (4*(m + off) + i) % 128 of chunk (m + off + i) % (K/128) —
    against integers in [-8, 8] and +-16; dense=True: {-1, 0, 1} on both
    sides.  Scales are powers of two.  The asserts show that any fp32
    evaluation order reaches `want`: every term is an integer and the sum of
    magnitudes is below 2^24, so every partial sum is representable, and
    the scaled result round-trips through bf16."""
    g = _gen(seed)
    nch = K // 128
    if dense:
        xq = torch.randint(-1, 2, (M, K), generator=g).float()
        q = torch.randint(-1, 2, (N, K), generator=g).float()
    else:
        xq = torch.zeros(M, K)
        for m in range(M):
            for i in range(4):
                k = ((m + off + i) % nch) * 128 + (4 * (m + off) + i) % 128
                xq[m, k] = _pick([1.0, -1.0, 2.0, -2.0], (1,), g)
        q = _pick([float(v) for v in range(-8, 9)] + [16.0, -16.0], (N, K), g)
    xs = _pick([0.25, 0.5, 1.0, 2.0], (M,), g)
    ws = _pick([0.125, 0.25, 0.5, 1.0], (N,), g)
    assert torch.equal(xq.to(FP8).float(), xq)
    assert torch.equal(q.to(FP8).float(), q)
    assert float((xq.abs().double() @ q.abs().double().T).max()) < 2 ** 24
    y = (xq.double() @ q.double().T) * xs.double()[:, None] * ws.double()
    want = y.to(torch.bfloat16)
    assert torch.equal(want.double(), y) and float(y.abs().max()) > 0
    return {"xq": xq.to(FP8), "xscale": xs, "qweight": q.to(FP8),
            "wscale": ws, "want": want}


def random_case(M, N, K, seed):
    g = _gen(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16)
    xq, xs = ref.quantize_rows_fp8_ref(x)
    qweight, wscale = OF.quantize_fp8(w)
    return {"x": x, "xq": xq, "xscale": xs, "qweight": qweight,
            "wscale": wscale}


def quant_rows(K, seed):
    """bf16 [33, K].  Row 0 is zero.  Rows 1..3 have amax = 448 * 2^e (e = 0,
    -5, 3) in their LAST element, so scale = 2^e, and start with quotients
    that are e4m3 ties (17 .. 27 at spacing 2; 7.5, 2.5 and 0.5 * 2^-9 among
    the subnormals) and subnormals.  Row 4 has an ordinary max in its last
    element; the rest are normal data of magnitudes 10^-3 .. 10^2."""
    g = _gen(seed)
    mag = 10.0 ** (5 * torch.rand(33, 1, generator=g) - 3)
    x = torch.randn(33, K, generator=g) * mag
    x[0] = 0
    special = torch.tensor([17.0, -19.0, 21.0, 23.0, -25.0, 27.0,
                            7.5 * 2 ** -9, -0.5 * 2 ** -9, 2.0 ** -7,
                            3 * 2.0 ** -9, -2.0 ** -9, 2.5 * 2 ** -9])
    for r, e in ((1, 0), (2, -5), (3, 3)):
        x[r] = (20 * torch.randn(K, generator=g)).clamp(-400, 400) * 2.0 ** e
        x[r, :12] = special * 2.0 ** e
        x[r, -1] = 448.0 * 2.0 ** e
    x[4] = x[4].clamp(-1, 1)
    x[4, -1] = -3.0
    x = x.to(torch.bfloat16)
    assert torch.equal(x[1, :12].float(), special)   # all of them are bf16
    return x


def test_quantize_dequantize_round_trip():
    w = 0.02 * torch.randn(128, 256, generator=_gen(1))
    w[5] = 0
    q, s = OF.quantize_fp8(w)
    assert q.dtype is FP8 and s.dtype is torch.float32 and s.shape == (128,)
    qf = q.float()
    assert bool(torch.isfinite(qf).all()) and float(qf.abs().max()) == 448
    assert float(s[5]) == 1.0 and bool((qf[5] == 0).all())
    assert torch.equal(s[:5], w[:5].abs().amax(-1) / 448)
    # a weight that is already representable comes back as it is
    c = exact_case(1, 64, 128, seed=3)
    w_hat = c["qweight"].float() * c["wscale"][:, None]
    w_hat[:, 0] = 448 * c["wscale"]            # pins every row's scale
    q2, s2 = OF.quantize_fp8(w_hat)
    assert torch.equal(s2, c["wscale"])
    assert torch.equal(OF.dequantize_fp8(q2, s2), w_hat)


def test_linear_fp8_cpu_is_the_reference_composition():
    c = random_case(5, 64, 256, seed=4)
    for x in (c["x"], c["x"].float(), c["x"].float().view(5, 1, 256)):
        xq, xs = OF.quantize_rows_fp8(x)
        want = torch.nn.functional.linear(
            ref.dequantize_fp8_ref(xq, xs).to(x.dtype),
            OF.dequantize_fp8(c["qweight"], c["wscale"]).to(x.dtype))
        got = OF.linear_fp8(x, c["qweight"], c["wscale"])
        assert got.dtype is x.dtype and got.shape == (*x.shape[:-1], 64)
        assert torch.equal(got, want)
    y = OF.linear_fp8_q(c["xq"], c["xscale"], c["qweight"], c["wscale"])
    want, tol = ref.linear_fp8_bound_ref(c["xq"], c["xscale"], c["qweight"],
                                         c["wscale"])
    assert y.dtype is torch.bfloat16
    assert bool(((y.double() - want).abs() <= tol).all())
    with pytest.raises(ValueError, match="no rows"):
        OF.linear_fp8(c["x"][:0], c["qweight"], c["wscale"])


def test_fp8_linear_module():
    lin = torch.nn.Linear(256, 64, bias=False)
    fl = Fp8Linear.from_linear(lin)
    q, s = OF.quantize_fp8(lin.weight.detach())
    assert torch.equal(fl.qweight.float(), q.float())
    assert torch.equal(fl.wscale, s)
    x = torch.randn(3, 256)
    assert torch.equal(fl(x), OF.linear_fp8(x, q, s))
    fl.to(torch.bfloat16)
    assert fl.qweight.dtype is FP8 and fl.wscale.dtype is torch.float32
    assert torch.equal(fl.qweight.float(), q.float())
    assert torch.equal(fl.wscale, s)


def test_state_dict_round_trips_through_an_fp8_model():
    cfg = LlamaConfig.small()
    torch.manual_seed(0)
    base = LlamaModel(cfg)
    state = quantize_llama_fp8_state(base.state_dict())
    model = LlamaModel(cfg, weight_dtype="fp8")
    model.load_state_dict(state)
    quantize_llama_fp8_(base)
    assert base.weight_dtype == "fp8"
    for a, b in zip(base.blocks, model.blocks):
        for name in QUANT_PROJECTIONS:
            ma, mb = getattr(a, name), getattr(b, name)
            assert isinstance(ma, Fp8Linear) and isinstance(mb, Fp8Linear)
            assert torch.equal(ma.qweight.float(), mb.qweight.float())
            assert torch.equal(ma.wscale, mb.wscale)
    back = model.state_dict()
    assert back.keys() == state.keys()
    assert all(torch.equal(back[k].float(), state[k].float()) for k in state)


def test_engine_fp8_lane_and_what_it_refuses():
    def engine(**kw):
        return LlamaEngine(device="cpu", dtype=torch.float32, use_graph=False,
                           eos_id=-1, kv_blocks=128, **kw)

    eng = engine(cfg=LlamaConfig.small(), weight_dtype="fp8")
    assert eng.weight_dtype == "fp8"
    assert all(isinstance(getattr(b, n), Fp8Linear)
               for b in eng.model.blocks for n in QUANT_PROJECTIONS)
    rid = eng.add_request([1, 17, 99, 250, 31], max_new_tokens=4)
    eng.run_until_done()
    assert len(eng.finished[rid].out_tokens) == 4
    assert isinstance(eng.model.lm_head, torch.nn.Linear)
    with pytest.raises(ValueError, match="does not cover MoE"):
        engine(cfg=LlamaConfig.moe_small(), weight_dtype="fp8")
