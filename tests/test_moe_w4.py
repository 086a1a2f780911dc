"""Int4 expert weights for the fused MoE FFN, the parts that need no GPU: the
expert quantizer, the argument checks, the reference path of ops.moe_ffn_w4,
the MoEFFN / LlamaEngine `expert_dtype` knob, checkpoints, the lossless
packing of the exact integer case and the bound of the random case that the
GPU tests (test_moe_w4_gpu.py) run on the kernels."""
import functools

import pytest
import torch

from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.models.llama.model import LlamaConfig, MoEFFN
from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from test_moe_fused import exact_case, random_case, sparse_idx

# (N, dim, ffn, E, k) of the random case, GPU and yardstick alike
W4_RANDOM_SHAPES = [(5, 256, 256, 4, 2), (200, 384, 640, 8, 2),
                    (64, 512, 1024, 8, 4)]


def pack_exact_case(shape):
    """exact_case(varied_gate=True) with its experts packed without loss:
    gate rows (values 32 and 64) as q = w / 16 with scale 16, up and down
    rows (+-1) as q = w with scale 1.  Every biased partial sum of the int4
    kernels, sum of x * (136 + q) over a group, is then an integer below
    2^24 (the largest is the down GEMM's 128 * 384 * 143), so a correct
    kernel is exact whatever its order and the case's `expect` stands."""
    N, d, F, E, k = shape
    idx = sparse_idx() if shape == (260, 128, 128, 128, 2) else None
    c = exact_case(*shape, idx=idx, varied_gate=True)
    gu, down = c["gate_up"].long(), c["down"].long()
    gu[:, :F] //= 16
    s_gu = torch.ones(E, 2 * F, d // 128)
    s_gu[:, :F] = 16
    c["gate_up_q"] = ref.w4_pack(gu.view(E * 2 * F, d)).view(E, 2 * F, d // 8)
    c["gate_up_s"] = s_gu.to(torch.bfloat16)
    c["down_q"] = ref.w4_pack(down.view(E * d, F)).view(E, d, F // 8)
    c["down_s"] = torch.ones(E, d, F // 128, dtype=torch.bfloat16)
    for name in ("gate_up", "down"):
        back = OF.dequantize_w4_experts(c[name + "_q"], c[name + "_s"])
        assert torch.equal(back, c[name].float()), name
    return c


@functools.lru_cache(maxsize=None)
def random_w4_case(shape):
    """random_case with quantized experts: (x, packed 4-tuple, dequantized
    gate_up and down in fp32, logits)."""
    x, gate_up, down, logits = random_case(shape)
    packed = OF.quantize_w4_experts(gate_up) + OF.quantize_w4_experts(down)
    return (x, packed, OF.dequantize_w4_experts(*packed[:2]),
            OF.dequantize_w4_experts(*packed[2:]), logits)


# ------------------------------------------------------------------ quantizer

def test_quantize_experts_is_quantize_w4_on_flat_rows():
    w = torch.randn(3, 128, 256, generator=torch.Generator().manual_seed(0))
    q, s = OF.quantize_w4_experts(w)
    q2, s2 = OF.quantize_w4(w.view(384, 256))
    assert q.shape == (3, 128, 32) and s.shape == (3, 128, 2)
    assert q.dtype is torch.int32 and s.dtype is torch.bfloat16
    assert torch.equal(q.view(384, 32), q2) and torch.equal(s.view(384, 2), s2)
    back = OF.dequantize_w4_experts(q, s)
    assert torch.equal(back, OF.dequantize_w4(q2, s2).view(3, 128, 256))
    # a dequantized stack is a fixed point: the round trip is exact
    q3, s3 = OF.quantize_w4_experts(back)
    assert torch.equal(OF.dequantize_w4_experts(q3, s3), back)


def test_exact_case_packs_without_loss():
    c = pack_exact_case((37, 256, 384, 4, 2))
    assert sorted(ref.w4_unpack(c["gate_up_q"][0, :384]).unique().tolist()) \
        == [0, 2, 4]
    out = OF.moe_ffn_w4(c["x"], c["gate_up_q"], c["gate_up_s"], c["down_q"],
                        c["down_s"], c["weights"], c["idx"])
    assert out.dtype is torch.bfloat16 and torch.equal(out.double(), c["expect"])


# ------------------------------------------------------------ argument checks

def _args(dim=128, ffn=128, E=4, k=2, N=5):
    return dict(
        x=torch.zeros(N, dim),
        gate_up_q=torch.zeros(E, 2 * ffn, dim // 8, dtype=torch.int32),
        gate_up_s=torch.ones(E, 2 * ffn, dim // 128, dtype=torch.bfloat16),
        down_q=torch.zeros(E, dim, ffn // 8, dtype=torch.int32),
        down_s=torch.ones(E, dim, ffn // 128, dtype=torch.bfloat16),
        weights=torch.zeros(N, k),
        idx=torch.arange(k, dtype=torch.int32).repeat(N, 1))


@pytest.mark.parametrize("change,exc,match", [
    (dict(x=torch.zeros(5, 192)), ValueError, "x has dim=192"),
    (dict(gate_up_s=torch.ones(4, 256, 2, dtype=torch.bfloat16)), ValueError,
     "gate_up_s must be"),
    (dict(down_s=torch.ones(4, 128, 1)), TypeError, "down_s must be bf16"),
    (dict(down_q=torch.zeros(4, 128, 16, dtype=torch.uint8)), TypeError,
     "down_q must be int32"),
    (dict(down_q=torch.zeros(4, 128, 32, dtype=torch.int32)[:, :, ::2]),
     ValueError, "down_q must be contiguous"),
    (dict(down_q=torch.zeros(4, 256, 16, dtype=torch.int32),
          down_s=torch.ones(4, 256, 1, dtype=torch.bfloat16)), ValueError,
     "down_q must be"),
    (dict(idx=torch.zeros(5, 2, dtype=torch.int64)), TypeError,
     "idx must be int32"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_argument_checks_name_the_argument(change, exc, match):
    OF.moe_ffn_w4(**_args())  # the base arguments are accepted
    with pytest.raises(exc, match=match):
        OF.moe_ffn_w4(**dict(_args(), **change))


# ------------------------------------------------------------- reference path

def test_cpu_path_is_the_reference_on_dequantized_weights():
    x, packed, gate_up, down, logits = random_w4_case(W4_RANDOM_SHAPES[0])
    w, idx = OF.moe_route(logits, 2)
    for xx in (x, x.float()):
        got = OF.moe_ffn_w4(xx, *packed, w, idx)
        assert got.dtype is xx.dtype
        assert torch.equal(got, ref.moe_ffn_ref(xx, gate_up, down, w, idx))
    xg = x.float().requires_grad_()
    wg = w.clone().requires_grad_()
    OF.moe_ffn_w4(xg, *packed, wg, idx).square().sum().backward()
    assert xg.grad.abs().max() > 0 and wg.grad.abs().max() > 0


@pytest.mark.parametrize("shape", W4_RANDOM_SHAPES, ids=str)
def test_bound_leaves_the_yardstick_half(shape):
    """ref.moe_ffn_bound_ref on the dequantized experts models exactly the
    int4 kernels (weights exact, h and the output rounded to bf16): its own
    bf16_points yardstick has to stay within half of tol on these inputs."""
    x, _, gate_up, down, logits = random_w4_case(shape)
    w, idx = ref.moe_route_ref(logits, shape[4])
    want, tol = ref.moe_ffn_bound_ref(x, gate_up, down, w, idx)
    yard, _ = ref.moe_ffn_bound_ref(x, gate_up, down, w, idx, bf16_points=True)
    ratio = ((yard - want).abs() / tol).max().item()
    print(f"MOE_FFN_W4_YARD {shape}: worst err/tol={ratio:.3f}")
    assert 0 < ratio <= 0.5


# ----------------------------------------------------------- model and engine

def _engine(**kw):
    torch.manual_seed(0)
    return LlamaEngine(LlamaConfig.moe_small(), device="cpu",
                       dtype=torch.float32, kv_blocks=64, eos_id=-1,
                       moe_impl="fused", **kw)


def _greedy(eng):
    rid = eng.add_request([5, 6, 7, 8, 9], max_new_tokens=6, temperature=0.0)
    eng.run_until_done()
    return eng.finished[rid].out_tokens


@pytest.fixture(scope="module")
def int4_tokens():
    eng = _engine(expert_dtype="int4")
    moe = eng.model.blocks[0].moe
    assert eng.cfg.expert_dtype == "int4" and moe.expert_dtype == "int4"
    assert moe.gate_up is None and moe.down is None
    assert set(dict(moe.named_buffers())) == {"gate_up_q", "gate_up_s",
                                              "down_q", "down_s"}
    assert [n for n, _ in moe.named_parameters()] == ["router.weight"]
    return _greedy(eng)


def test_engine_int4_emits_the_dequantized_model_tokens(int4_tokens):
    eng = _engine()
    assert eng.cfg.expert_dtype == "bf16"
    for blk in eng.model.blocks:
        for p in (blk.moe.gate_up, blk.moe.down):
            p.data = OF.dequantize_w4_experts(*OF.quantize_w4_experts(p.data))
    assert len(int4_tokens) == 6 and _greedy(eng) == int4_tokens


def test_prefill_lane_matches_kernel_lane_fp32(monkeypatch):
    torch.manual_seed(0)
    moe = MoEFFN(128, 256, 4, 2, impl="fused").quantize_experts_()
    x = torch.randn(2, 9, 128)
    with torch.no_grad():
        want = moe(x)
        monkeypatch.setattr(MoEFFN, "N_KERNEL", 4)
        torch.testing.assert_close(moe(x), want)
    assert moe.gate_up_s.dtype is torch.bfloat16
    assert moe.to(torch.float64).down_s.dtype is torch.bfloat16


def test_unsupported_settings_raise():
    with pytest.raises(ValueError, match="expert_dtype"):
        _engine(expert_dtype="int8")
    with pytest.raises(ValueError, match="moe_impl"):
        LlamaEngine(LlamaConfig.moe_small(), device="cpu", kv_blocks=64,
                    dtype=torch.float32, moe_impl="loop", expert_dtype="int4")
    with pytest.raises(ValueError, match="moe_impl"):
        MoEFFN(128, 128, 4, 2, impl="loop", expert_dtype="int4")
    with pytest.raises(ValueError, match="MoE"):
        LlamaEngine(LlamaConfig.small(), device="cpu", kv_blocks=64,
                    dtype=torch.float32, expert_dtype="int4")
    with pytest.raises(ValueError, match="MoE"):  # the dense knob still refuses
        _engine(weight_dtype="int4")


def test_safetensors_round_trip(tmp_path, int4_tokens):
    kw = dict(device="cpu", dtype=torch.float32, kv_blocks=64, eos_id=-1,
              moe_impl="fused")
    packed, full = str(tmp_path / "w4.safetensors"), str(tmp_path / "bf16.safetensors")
    _engine(expert_dtype="int4").save_safetensors(packed)
    _engine().save_safetensors(full)
    eng = LlamaEngine.from_safetensors(packed, LlamaConfig.moe_small(), **kw)
    assert eng.expert_dtype == "int4" and _greedy(eng) == int4_tokens
    with pytest.raises(ValueError, match="int4 experts"):
        LlamaEngine.from_safetensors(packed, LlamaConfig.moe_small(),
                                     expert_dtype="bf16", **kw)
    eng = LlamaEngine.from_safetensors(full, LlamaConfig.moe_small(),
                                       expert_dtype="int4", **kw)
    assert eng.model.blocks[0].moe.expert_dtype == "int4"
    assert _greedy(eng) == int4_tokens
