"""MXFP4 weight linear on the CPU: the OCP MX quantizer against its
definition, the reference composition behind ops.linear_mxfp4, Mxfp4Linear
and the weight_dtype="mxfp4" model.  The case builders here are shared with
tests/test_linear_mxfp4_gpu.py."""
import pytest
import torch

from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.models.llama.model import (QUANT_PROJECTIONS,
                                                   LlamaConfig, LlamaModel,
                                                   Mxfp4Linear,
                                                   quantize_llama_mxfp4_,
                                                   quantize_llama_mxfp4_state)
from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref

FP8 = torch.float8_e4m3fn
E2M1 = torch.tensor(ref.E2M1_VALUES + tuple(-v for v in ref.E2M1_VALUES))
XQ_VALUES = (0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0)


def _hash(t, mul, shift):
    """A multiplicative hash of an index tensor: no period along any axis."""
    return ((t * mul) & 0xFFFFFFFF) >> shift


def pack(codes):
    """codes uint8 [N, K] -> [N, K/2], element 2j in the low nibble."""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def exact_case(M, N, K, seed, exponent=None):
    """xq from XQ_VALUES, weight codes from all 16 nibbles, block exponents
    in -2 .. 2 by a hash of (row, block) — or `exponent` for every block —
    and power-of-two row scales.  Every product is a multiple of 1/4 and
    every scaled product a multiple of 1/16 of magnitude at most 2 * 6 * 4;
    up to K = 1024 the magnitudes sum to less than 2^20 (asserted), that is
    2^24 sixteenths, so every fp32 partial sum is exact in any order and the
    expected value is the fp64 product rounded once to bf16."""
    i = torch.arange(M * K, dtype=torch.int64).view(M, K) + seed
    xq = torch.tensor(XQ_VALUES)[_hash(i, 2654435761, 13) % 8]
    j = torch.arange(N * K, dtype=torch.int64).view(N, K) + 7919 * seed
    codes = (_hash(j, 2246822519, 11) % 16).to(torch.uint8)
    b = torch.arange(N * (K // 32), dtype=torch.int64).view(N, K // 32) + seed
    e = _hash(b, 3266489917, 15) % 5 - 2
    if exponent is not None:
        e = torch.full_like(e, exponent)
    xs = torch.tensor([0.25, 0.5, 1.0, 2.0])[_hash(
        torch.arange(M) + seed, 668265263, 7) % 4]
    w_hat = (E2M1[codes.long()].double().view(N, -1, 32)
             * 2.0 ** e.double().unsqueeze(-1)).view(N, K)
    sc = 2.0 ** (exponent or 0)
    assert float((xq.abs().double() @ w_hat.abs().T).max()) / sc < 2 ** 20
    y = (xq.double() @ w_hat.T) * xs.double()[:, None]
    assert float(y.abs().max()) > 0
    return {"xq": xq.to(FP8), "xscale": xs, "qweight": pack(codes),
            "wscale": (e + 127).to(torch.uint8), "w_hat": w_hat,
            "want": y.to(torch.bfloat16)}


def random_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16)
    xq, xs = ref.quantize_rows_fp8_ref(x)
    qweight, wscale = OF.quantize_mxfp4(w)
    return {"x": x, "w": w, "xq": xq, "xscale": xs, "qweight": qweight,
            "wscale": wscale}


def test_quantizer_against_its_definition():
    # a weight on the MX grid whose blocks each hold a code of magnitude 4
    # or 6 (so the block exponent is pinned) round-trips exactly
    c = exact_case(1, 64, 256, seed=3)
    codes = torch.stack([c["qweight"] & 15, c["qweight"] >> 4], -1).view(64, 256)
    codes[:, 0::32] = 7                      # 6 * 2^e leads every block
    codes[::2, 0::32] = 14                   # ... or -4 * 2^e
    q0 = pack(codes)
    w_hat = OF.dequantize_mxfp4(q0, c["wscale"])
    assert w_hat.dtype is torch.float32 and w_hat.shape == (64, 256)
    q, s = OF.quantize_mxfp4(w_hat)
    assert q.dtype is torch.uint8 and q.shape == (64, 128)
    assert s.dtype is torch.uint8 and s.shape == (64, 8)
    assert torch.equal(s, c["wscale"])
    assert torch.equal(OF.dequantize_mxfp4(q, s), w_hat)
    nz = codes & 7 != 0                      # +0 and -0 may swap, nothing else
    assert torch.equal(torch.stack([q & 15, q >> 4], -1).view(64, 256)[nz],
                       codes[nz])
    # nibble order: element 2j is the low nibble of byte j
    w = torch.zeros(64, 128)
    w[0, :4] = torch.tensor([6.0, -1.0, 0.5, 3.0])
    q, s = OF.quantize_mxfp4(w)
    assert q[0, :2].tolist() == [0x7 | 0xA << 4, 0x1 | 0x5 << 4]
    assert s[0].tolist() == [127] * 4 and int(q[1:].max()) == 0  # zero blocks
    # random data: RNE to the grid with the block's own exponent, ties to
    # the even code, and the largest magnitude of a non-zero block is 4 or 6
    rc = random_case(1, 128, 256, seed=1)
    w = rc["w"].double().view(128, 8, 32)
    e = torch.floor(torch.log2(w.abs().amax(-1))) - 2
    assert torch.equal(rc["wscale"].double() - 127, e)
    v = (w / 2.0 ** e.unsqueeze(-1)).view(128, 256)
    got = OF.dequantize_mxfp4(rc["qweight"], rc["wscale"]).double().view(
        128, 8, 32) / 2.0 ** e.unsqueeze(-1)
    dist = (v.unsqueeze(-1) - E2M1.double()).abs()
    assert torch.equal((got.view(128, 256) - v).abs(), dist.amin(-1))
    assert set(got.abs().amax(-1).flatten().tolist()) <= {4.0, 6.0}
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -2.5, 7.0])
    w = torch.zeros(64, 128)
    w[0, :9], w[0, 9] = ties, 6.0
    q, s = OF.quantize_mxfp4(w)
    assert OF.dequantize_mxfp4(q, s)[0, :9].tolist() == [
        0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -2.0, 6.0]


def test_linear_mxfp4_cpu_is_the_reference_composition():
    c = random_case(5, 64, 256, seed=4)
    for x in (c["x"], c["x"].float(), c["x"].float().view(5, 1, 256)):
        xq, xs = OF.quantize_rows_fp8(x)
        want = torch.nn.functional.linear(
            ref.dequantize_fp8_ref(xq, xs).to(x.dtype),
            OF.dequantize_mxfp4(c["qweight"], c["wscale"]).to(x.dtype))
        got = OF.linear_mxfp4(x, c["qweight"], c["wscale"])
        assert got.dtype is x.dtype and got.shape == (*x.shape[:-1], 64)
        assert torch.equal(got, want)
    y = OF.linear_mxfp4_q(c["xq"], c["xscale"], c["qweight"], c["wscale"])
    want, tol = ref.linear_mxfp4_bound_ref(c["xq"], c["xscale"], c["qweight"],
                                           c["wscale"])
    assert y.dtype is torch.bfloat16
    assert bool(((y.double() - want).abs() <= tol).all())
    e = exact_case(33, 64, 256, seed=9)
    assert torch.equal(OF.linear_mxfp4_q(e["xq"], e["xscale"], e["qweight"],
                                         e["wscale"]), e["want"])
    x = c["x"].float().requires_grad_()
    OF.linear_mxfp4(x, c["qweight"], c["wscale"]).sum().backward()
    assert torch.allclose(x.grad, OF.dequantize_mxfp4(
        c["qweight"], c["wscale"]).sum(0).expand(5, 256))
    with pytest.raises(ValueError, match="no rows"):
        OF.linear_mxfp4(c["x"][:0], c["qweight"], c["wscale"])
    with pytest.raises(TypeError, match="uint8"):
        OF.linear_mxfp4(c["x"], c["qweight"].int(), c["wscale"])
    with pytest.raises(ValueError, match="K/32"):
        OF.linear_mxfp4(c["x"], c["qweight"], c["wscale"][:, :4].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        OF.linear_mxfp4(c["x"], c["qweight"].T.contiguous().T, c["wscale"])


def test_mxfp4_linear_module_and_state_dict():
    lin = torch.nn.Linear(256, 64, bias=False)
    ml = Mxfp4Linear.from_linear(lin)
    q, s = OF.quantize_mxfp4(lin.weight.detach())
    x = torch.randn(3, 256)
    assert torch.equal(ml(x), OF.linear_mxfp4(x, q, s))
    ml.to(torch.bfloat16)
    assert ml.qweight.dtype is torch.uint8 and ml.wscale.dtype is torch.uint8
    assert torch.equal(ml.qweight, q) and torch.equal(ml.wscale, s)

    cfg = LlamaConfig.small()
    torch.manual_seed(0)
    base = LlamaModel(cfg)
    state = quantize_llama_mxfp4_state(base.state_dict())
    model = LlamaModel(cfg, weight_dtype="mxfp4")
    model.load_state_dict(state)
    assert quantize_llama_mxfp4_(base).weight_dtype == "mxfp4"
    for a, b in zip(base.blocks, model.blocks):
        for name in QUANT_PROJECTIONS:
            ma, mb = getattr(a, name), getattr(b, name)
            assert isinstance(ma, Mxfp4Linear) and isinstance(mb, Mxfp4Linear)
            assert torch.equal(ma.qweight, mb.qweight)
            assert torch.equal(ma.wscale, mb.wscale)
    back = model.state_dict()
    assert back.keys() == state.keys()
    assert all(torch.equal(back[k], state[k]) for k in state)


def test_engine_mxfp4_lane_and_what_it_refuses(tmp_path):
    def engine(**kw):
        return LlamaEngine(device="cpu", dtype=torch.float32, use_graph=False,
                           eos_id=-1, kv_blocks=128, **kw)

    eng = engine(cfg=LlamaConfig.small(), weight_dtype="mxfp4")
    assert eng.weight_dtype == "mxfp4"
    assert all(isinstance(getattr(b, n), Mxfp4Linear)
               for b in eng.model.blocks for n in QUANT_PROJECTIONS)
    rid = eng.add_request([1, 17, 99, 250, 31], max_new_tokens=4)
    eng.run_until_done()
    assert len(eng.finished[rid].out_tokens) == 4
    assert isinstance(eng.model.lm_head, torch.nn.Linear)
    with pytest.raises(ValueError, match="does not cover MoE"):
        engine(cfg=LlamaConfig.moe_small(), weight_dtype="mxfp4")
    path = str(tmp_path / "mx.safetensors")
    eng.save_safetensors(path)
    with pytest.raises(ValueError, match="holds mxfp4 weights"):
        LlamaEngine.from_safetensors(path, cfg=LlamaConfig.small(),
                                     device="cpu")
