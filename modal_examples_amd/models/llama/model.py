"""Llama-3-class decoder-only transformer, MI355X-first.

The model family behind the reference's canonical LLM-serving examples
(trigger: 06_gpu_and_ml/llm-serving/vllm_inference.py:158-209 — Llama/Qwen
class models under vLLM; trtllm_latency.py:10-21 LLaMA-3-8B).

MI355X mapping:
  K7 prefill  → gfx950 flash attention (causal, GQA, D=128)
  K6 decode   → gfx950 paged decode kernel over the paged KV cache
  RMSNorm / RoPE / SwiGLU → fused gfx950 kernels
  QKV and gate_up projections → single fused GEMMs (hipBLASLt), or the
  int4 / fp8 / mxfp4 kernels under weight_dtype (QuantLinear, Fp8Linear,
  Mxfp4Linear)
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import torch
import torch.nn as nn

from ...ops import functional as OF
from ..sdxl.layers import RMSNormK


@dataclass
class LlamaConfig:
    vocab_size: int = 128256
    dim: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 8
    head_dim: int = 128
    ffn_dim: int = 14336
    rope_base: float = 500000.0
    norm_eps: float = 1e-5
    max_seq: int = 8192
    n_experts: int = 0   # >0: MoE FFN (Mixtral/DeepSeek-class)
    experts_per_tok: int = 2
    moe_impl: str = "loop"  # MoEFFN forward: "loop" or "fused" (ops.moe_ffn)
    expert_dtype: str = "bf16"  # MoE expert weights: "bf16", "int4", "mxfp4"

    @staticmethod
    def llama3_8b() -> "LlamaConfig":
        return LlamaConfig()

    @staticmethod
    def small() -> "LlamaConfig":
        return LlamaConfig(vocab_size=1024, dim=256, n_layers=2, n_heads=4,
                           n_kv_heads=2, head_dim=64, ffn_dim=512,
                           rope_base=10000.0, max_seq=512)

    @staticmethod
    def moe_small() -> "LlamaConfig":
        return LlamaConfig(vocab_size=1024, dim=256, n_layers=2, n_heads=4,
                           n_kv_heads=2, head_dim=64, ffn_dim=256,
                           rope_base=10000.0, max_seq=512, n_experts=4)


WEIGHT_DTYPES = ("bf16", "int4", "fp8", "mxfp4")
EXPERT_DTYPES = ("bf16", "int4", "mxfp4")


class QuantLinear(nn.Module):
    """Bias-free linear layer over int4 weights (ops.quantize_w4): buffers
    `qweight` int32 [out, in/8] and `scales` bf16 [out, in/128].

    Two lanes.  Up to M_KERNEL rows (decode) the forward is ops.linear_w4:
    on the GPU the csrc/linear_w4.hip kernel, which applies each group's
    scale to its fp32 partial sum and never rounds a dequantized weight.
    Above that (prefill) the weight is dequantized into a scratch tensor of
    the activation dtype and goes through the ordinary GEMM; in bf16 that
    rounds every w_hat = scale * q to bf16, so the two lanes differ by that
    rounding (in fp32 they are the same product).  On the CPU, in fp32 or
    under autograd, both lanes are the reference composition."""

    # rows up to which the kernel lane is taken.  Measured
    # (profiles/linear_w4.txt, second table): at 1024 rows the kernel beats
    # the dequantize lane on all four Llama-3-8B projections (188 / 255,
    # 135 / 171, 765 / 1214, 395 / 665 us), at 2048 rows it loses on all
    # four (376 / 280, 267 / 193, 1518 / 1361, 789 / 731 us).  1024 is the
    # largest measured count on the kernel's side of the crossover.
    M_KERNEL = 1024

    def __init__(self, in_features: int, out_features: int, device=None):
        super().__init__()
        if in_features % 128 != 0 or in_features < 128:
            raise ValueError(f"QuantLinear: in_features={in_features} must "
                             f"be a multiple of the int4 group size 128")
        if out_features % 64 != 0 or out_features < 64:
            raise ValueError(f"QuantLinear: out_features={out_features} "
                             f"must be a multiple of 64")
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("qweight", torch.zeros(
            out_features, in_features // 8, dtype=torch.int32, device=device))
        self.register_buffer("scales", torch.ones(
            out_features, in_features // 128, dtype=torch.bfloat16,
            device=device))

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "QuantLinear":
        if lin.bias is not None:
            raise ValueError("QuantLinear has no bias")
        w = lin.weight.detach()
        if w.dtype not in (torch.bfloat16, torch.float32):
            w = w.float()
        m = cls(lin.in_features, lin.out_features, device="meta")
        q, s = OF.quantize_w4(w.contiguous())
        m.qweight, m.scales = q, s
        return m

    def _apply(self, fn, recurse=True):
        # module.to(dtype) casts every floating buffer; the scales are bf16
        # by format (a round trip through a wider type loses nothing)
        super()._apply(fn, recurse)
        if self.scales.dtype is not torch.bfloat16:
            self.scales = self.scales.to(torch.bfloat16)
        return self

    def forward(self, x):
        rows = x.numel() // self.in_features
        if rows <= self.M_KERNEL:
            return OF.linear_w4(x, self.qweight, self.scales)
        w = OF.dequantize_w4(self.qweight, self.scales).to(x.dtype)
        return nn.functional.linear(x, w)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, int4 g128")


class Fp8Linear(nn.Module):
    """Bias-free linear layer over fp8 weights (ops.quantize_fp8): buffers
    `qweight` float8_e4m3fn [out, in] and `wscale` fp32 [out], activations
    quantized per row at run time ("W8A8 dynamic").

    Two lanes, as QuantLinear.  Up to M_KERNEL rows the forward is
    ops.linear_fp8: on the GPU the row-quantization kernel and the fp8 MFMA
    GEMM of csrc/linear_fp8.hip, which multiply the fp8 values exactly and
    apply both scales to the fp32 sum.  Above that, PREFILL_LANE picks.
    "tiled" (on the GPU in bf16 without grad): ops.linear_fp8(tiled=True),
    the same row quantizer and the workgroup-tiled fp8 GEMM of the same
    file, so a token's projection is the same arithmetic in prefill and in
    decode and no weight-sized scratch is made.  "dequant" (and "tiled"
    anywhere else): the weight is dequantized into a scratch tensor of the
    activation dtype and goes through the ordinary GEMM on the unquantized
    activations; in bf16 that rounds every w_hat = wscale * q to bf16 and
    skips the activation quantization, so it differs from the kernel lanes
    by those roundings.  On the CPU, in fp32 or under autograd, the kernel
    lane is the reference composition."""

    # rows up to which the kernel lane is taken.  Measured
    # (profiles/linear_fp8.txt, second table, "fp8" against "fp8deq"): at
    # 1024 rows the kernel lane beats the dequantize lane on three of the
    # four Llama-3-8B projections and is level on the fourth (142 / 147,
    # 107 / 106, 510 / 749, 269 / 427 us), at 2048 rows it loses on all four
    # (273 / 179, 204 / 127, 962 / 898, 508 / 491 us).  1024 is the largest
    # measured count on the kernel's side of the crossover.
    M_KERNEL = 1024

    # the lane above M_KERNEL rows on the GPU in bf16 without grad: "tiled"
    # (ops.linear_fp8(tiled=True)) or "dequant".  Measured
    # (profiles/linear_fp8_tiled.txt, "fp8tile" against the faster of "fp8"
    # and "fp8deq" in the same windows): the tiled lane wins on all four
    # Llama-3-8B projections at 2048, 4096 and 8192 rows (2048: 89 / 180,
    # 58 / 129, 343 / 901, 178 / 488 us; 8192, the narrowest: 298 / 381,
    # 206 / 246, 1304 / 1822, 671 / 876 us), against a spread of under 1 %
    # between the windows of either arm.  The M_KERNEL figures above are from
    # the earlier table and have not moved with this lane.
    PREFILL_LANE = "tiled"

    def __init__(self, in_features: int, out_features: int, device=None):
        super().__init__()
        if in_features % 128 != 0 or in_features < 128:
            raise ValueError(f"Fp8Linear: in_features={in_features} must "
                             f"be a multiple of 128")
        if out_features % 64 != 0 or out_features < 64:
            raise ValueError(f"Fp8Linear: out_features={out_features} "
                             f"must be a multiple of 64")
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("qweight", torch.zeros(
            out_features, in_features, dtype=torch.float8_e4m3fn,
            device=device))
        self.register_buffer("wscale", torch.ones(
            out_features, dtype=torch.float32, device=device))

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "Fp8Linear":
        if lin.bias is not None:
            raise ValueError("Fp8Linear has no bias")
        w = lin.weight.detach()
        if w.dtype not in (torch.bfloat16, torch.float32):
            w = w.float()
        m = cls(lin.in_features, lin.out_features, device="meta")
        m.qweight, m.wscale = OF.quantize_fp8(w.contiguous())
        return m

    def _apply(self, fn, recurse=True):
        # module.to(dtype) casts every floating buffer; both are what they
        # are by format.  The weight bytes are kept aside (a cast to bf16
        # and back would be exact but doubles the memory in between); the
        # scale's round trip would not be exact, so it is moved by device
        # only.
        q, s = self.qweight, self.wscale
        super()._apply(fn, recurse)
        if self.qweight.dtype is not torch.float8_e4m3fn:
            self.qweight = q.to(self.qweight.device)
        if self.wscale.dtype is not torch.float32:
            self.wscale = s.to(self.wscale.device)
        return self

    def forward(self, x):
        rows = x.numel() // self.in_features
        if rows <= self.M_KERNEL:
            return OF.linear_fp8(x, self.qweight, self.wscale)
        if self.PREFILL_LANE not in ("tiled", "dequant"):
            raise ValueError(f"Fp8Linear.PREFILL_LANE={self.PREFILL_LANE!r} "
                             f"(must be 'tiled' or 'dequant')")
        if (self.PREFILL_LANE == "tiled" and x.is_cuda
                and x.dtype is torch.bfloat16
                and not (torch.is_grad_enabled() and x.requires_grad)):
            return OF.linear_fp8(x, self.qweight, self.wscale, tiled=True)
        w = OF.dequantize_fp8(self.qweight, self.wscale).to(x.dtype)
        return nn.functional.linear(x, w)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, fp8 e4m3 per-channel")


class Mxfp4Linear(nn.Module):
    """Bias-free linear layer over MXFP4 weights (ops.quantize_mxfp4):
    buffers `qweight` uint8 [out, in/2] (two e2m1 codes a byte) and `wscale`
    uint8 [out, in/32] (E8M0 block scales), activations quantized per row to
    e4m3 at run time.  Both buffers are integers, so `.to(dtype)` leaves
    them alone.

    Two lanes, as Fp8Linear.  Up to M_KERNEL rows the forward is
    ops.linear_mxfp4: on the GPU the row-quantization kernel and the
    block-scaled fp4 MFMA GEMM of csrc/linear_mxfp4.hip.  Above that the
    weight is dequantized (exactly: w_hat has two mantissa bits) into a
    scratch tensor of the activation dtype and goes through the ordinary
    GEMM on the unquantized activations, so the two lanes differ by the
    activation quantization.  On the CPU, in fp32 or under autograd, the
    kernel lane is the reference composition."""

    # rows up to which the kernel lane is taken.  Measured
    # (profiles/linear_mxfp4.txt, first table, "mxfp4" against "mxfp4deq"):
    # the kernel lane beats the dequantize lane on all four Llama-3-8B
    # projections at every measured row count, at 2048 rows still by 246 /
    # 991, 184 / 685, 856 / 4742 and 452 / 2418 us (the dequantization is
    # several torch passes over the weight).  2048 is the largest count
    # measured, so the switch stays there.
    M_KERNEL = 2048

    def __init__(self, in_features: int, out_features: int, device=None):
        super().__init__()
        if in_features % 128 != 0 or in_features < 128:
            raise ValueError(f"Mxfp4Linear: in_features={in_features} must "
                             f"be a multiple of 128")
        if out_features % 64 != 0 or out_features < 64:
            raise ValueError(f"Mxfp4Linear: out_features={out_features} "
                             f"must be a multiple of 64")
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("qweight", torch.zeros(
            out_features, in_features // 2, dtype=torch.uint8, device=device))
        self.register_buffer("wscale", torch.full(
            (out_features, in_features // 32), 127, dtype=torch.uint8,
            device=device))

    @classmethod
    def from_linear(cls, lin: nn.Linear) -> "Mxfp4Linear":
        if lin.bias is not None:
            raise ValueError("Mxfp4Linear has no bias")
        w = lin.weight.detach()
        if w.dtype not in (torch.bfloat16, torch.float32):
            w = w.float()
        m = cls(lin.in_features, lin.out_features, device="meta")
        m.qweight, m.wscale = OF.quantize_mxfp4(w.contiguous())
        return m

    def forward(self, x):
        rows = x.numel() // self.in_features
        if rows <= self.M_KERNEL:
            return OF.linear_mxfp4(x, self.qweight, self.wscale)
        w = OF.dequantize_mxfp4(self.qweight, self.wscale).to(x.dtype)
        return nn.functional.linear(x, w)

    def extra_repr(self):
        return (f"in_features={self.in_features}, "
                f"out_features={self.out_features}, mxfp4 e2m1 b32")


QUANT_PROJECTIONS = ("qkv", "o_proj", "gate_up", "down")


def quantize_llama_(model: "LlamaModel") -> "LlamaModel":
    """Replace qkv, o_proj, gate_up and down of every block by QuantLinear
    modules quantized from the current weights, one projection at a time so
    the bf16 copy of each is released as it goes.  Embedding, norms and
    lm_head stay as they are."""
    for blk in model.blocks:
        if blk.moe is not None:
            raise ValueError("int4 weights do not cover MoE experts")
        for name in QUANT_PROJECTIONS:
            lin = getattr(blk, name)
            if isinstance(lin, nn.Linear):
                setattr(blk, name, QuantLinear.from_linear(lin))
    model.weight_dtype = "int4"
    return model


def quantize_llama_state(state: dict) -> dict:
    """A bf16 state dict of a dense LlamaModel (or of one TP shard) with the
    four block projections replaced by their `qweight` / `scales` pair."""
    out = {}
    for k, v in state.items():
        parts = k.split(".")
        if (len(parts) == 4 and parts[0] == "blocks"
                and parts[2] in QUANT_PROJECTIONS and parts[3] == "weight"):
            if v.dtype not in (torch.bfloat16, torch.float32):
                v = v.float()
            q, s = OF.quantize_w4(v.contiguous())
            out[k[:-len("weight")] + "qweight"] = q
            out[k[:-len("weight")] + "scales"] = s
        else:
            out[k] = v
    return out


def quantize_llama_fp8_(model: "LlamaModel") -> "LlamaModel":
    """`quantize_llama_` for fp8: the four block projections become
    Fp8Linear modules, one projection at a time."""
    for blk in model.blocks:
        if blk.moe is not None:
            raise ValueError("fp8 weights do not cover MoE experts")
        for name in QUANT_PROJECTIONS:
            lin = getattr(blk, name)
            if isinstance(lin, nn.Linear):
                setattr(blk, name, Fp8Linear.from_linear(lin))
    model.weight_dtype = "fp8"
    return model


def quantize_llama_fp8_state(state: dict) -> dict:
    """`quantize_llama_state` for fp8: the four block projections replaced
    by their `qweight` / `wscale` pair."""
    out = {}
    for k, v in state.items():
        parts = k.split(".")
        if (len(parts) == 4 and parts[0] == "blocks"
                and parts[2] in QUANT_PROJECTIONS and parts[3] == "weight"):
            if v.dtype not in (torch.bfloat16, torch.float32):
                v = v.float()
            q, s = OF.quantize_fp8(v.contiguous())
            out[k[:-len("weight")] + "qweight"] = q
            out[k[:-len("weight")] + "wscale"] = s
        else:
            out[k] = v
    return out


def quantize_llama_mxfp4_(model: "LlamaModel") -> "LlamaModel":
    """`quantize_llama_` for MXFP4: the four block projections become
    Mxfp4Linear modules, one projection at a time."""
    for blk in model.blocks:
        if blk.moe is not None:
            raise ValueError("mxfp4 weights do not cover MoE experts")
        for name in QUANT_PROJECTIONS:
            lin = getattr(blk, name)
            if isinstance(lin, nn.Linear):
                setattr(blk, name, Mxfp4Linear.from_linear(lin))
    model.weight_dtype = "mxfp4"
    return model


def quantize_llama_mxfp4_state(state: dict) -> dict:
    """`quantize_llama_state` for MXFP4: the four block projections replaced
    by their uint8 `qweight` / `wscale` pair."""
    out = {}
    for k, v in state.items():
        parts = k.split(".")
        if (len(parts) == 4 and parts[0] == "blocks"
                and parts[2] in QUANT_PROJECTIONS and parts[3] == "weight"):
            if v.dtype not in (torch.bfloat16, torch.float32):
                v = v.float()
            q, s = OF.quantize_mxfp4(v.contiguous())
            out[k[:-len("weight")] + "qweight"] = q
            out[k[:-len("weight")] + "wscale"] = s
        else:
            out[k] = v
    return out


# the packed expert formats: their quantizers, and the dtype of the _q buffer,
# which tells the formats apart in a module and in a file
_EXPERT_QUANTIZERS = {"int4": OF.quantize_w4_experts,
                      "mxfp4": OF.quantize_mxfp4_experts}
_EXPERT_Q_DTYPES = {torch.int32: "int4", torch.uint8: "mxfp4"}


def quantize_llama_experts_(model: "LlamaModel",
                            expert_dtype: str = "int4") -> "LlamaModel":
    """Quantize the experts of every MoE block in place to `expert_dtype`
    ("int4" or "mxfp4"; MoEFFN.quantize_experts_), one matrix at a time so the
    bf16 copy of each is released as it goes.  Router, attention projections,
    embedding, norms and lm_head stay as they are."""
    if model.cfg.n_experts <= 0:
        raise ValueError(f"expert_dtype={expert_dtype!r} needs an MoE config "
                         "(n_experts > 0)")
    for blk in model.blocks:
        blk.moe.quantize_experts_(expert_dtype)
    model.cfg = dataclasses.replace(model.cfg, expert_dtype=expert_dtype)
    return model


def quantize_llama_expert_state(state: dict,
                                expert_dtype: str = "int4") -> dict:
    """A bf16 state dict of an MoE LlamaModel with every block's
    `moe.gate_up` / `moe.down` replaced by its `_q` / `_s` pair in
    `expert_dtype` ("int4" or "mxfp4")."""
    quantize = _EXPERT_QUANTIZERS[expert_dtype]
    out = {}
    for k, v in state.items():
        parts = k.split(".")
        if (len(parts) == 4 and parts[0] == "blocks" and parts[2] == "moe"
                and parts[3] in ("gate_up", "down")):
            if v.dtype not in (torch.bfloat16, torch.float32):
                v = v.float()
            out[k + "_q"], out[k + "_s"] = quantize(v.contiguous())
        else:
            out[k] = v
    return out


class LlamaBlock(nn.Module):
    def __init__(self, cfg: LlamaConfig, tp_world: int = 1,
                 weight_dtype: str = "bf16"):
        """tp_world>1: Megatron head-sharded block (the --tensor-parallel-size
        role of vllm_inference.py:180 / trtllm tensor_parallel_size).  qkv and
        gate_up are column-sharded (this rank's q/kv-head and gate/up slices,
        NO comm in forward), o_proj and down are row-sharded — the model adds
        ONE all-reduce after each (two collectives per block over xGMI)."""
        super().__init__()
        d, hd = cfg.dim, cfg.head_dim
        assert cfg.n_heads % tp_world == 0 and cfg.n_kv_heads % tp_world == 0 \
            and cfg.ffn_dim % tp_world == 0, \
            f"tp={tp_world} must divide heads {cfg.n_heads}/{cfg.n_kv_heads}" \
            f" and ffn {cfg.ffn_dim}"
        self.nq, self.nkv = cfg.n_heads // tp_world, cfg.n_kv_heads // tp_world
        if weight_dtype not in WEIGHT_DTYPES:
            raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES}, "
                             f"got {weight_dtype!r}")
        if weight_dtype != "bf16":
            # built with buffers of the right shape (meta-device boot);
            # a shard whose K is no multiple of 128 raises here
            if cfg.n_experts > 0:
                raise ValueError(f"weight_dtype={weight_dtype!r} does not "
                                 f"cover MoE models; their experts take "
                                 f"expert_dtype='int4'|'mxfp4'")
            quant = {"int4": QuantLinear, "fp8": Fp8Linear,
                     "mxfp4": Mxfp4Linear}[weight_dtype]

            def linear(i, o, bias=False):
                return quant(i, o)
        else:
            linear = nn.Linear
        self.attn_norm = RMSNormK(d, cfg.norm_eps)
        self.qkv = linear(d, (self.nq + 2 * self.nkv) * hd, bias=False)
        self.o_proj = linear(self.nq * hd, d, bias=False)
        self.ffn_norm = RMSNormK(d, cfg.norm_eps)
        if cfg.n_experts > 0:
            assert tp_world == 1, "MoE + TP not supported (EP is a non-goal)"
            self.moe = MoEFFN(d, cfg.ffn_dim, cfg.n_experts,
                              cfg.experts_per_tok, impl=cfg.moe_impl,
                              expert_dtype=cfg.expert_dtype)
            self.gate_up = self.down = None
        else:
            self.moe = None
            self.gate_up = linear(d, 2 * cfg.ffn_dim // tp_world, bias=False)
            self.down = linear(cfg.ffn_dim // tp_world, d, bias=False)
        self.hd = hd
        self.ffn_dim = cfg.ffn_dim // tp_world

    def project_qkv(self, x, lora=None, li: int = 0):
        """x [B,S,d] → BSHD views of the fused projection (zero copies):
        q [B,S,nq,hd], k/v [B,S,nkv,hd].  lora (lora.LoraRows) adds layer
        li's adapter deltas to the projection output, as in out_proj / ffn."""
        B, S, _ = x.shape
        qkv = self.qkv(x)
        if lora is not None:
            lora.apply_(li, "qkv", qkv, x)
        q, k, v = qkv.split(
            [self.nq * self.hd, self.nkv * self.hd, self.nkv * self.hd], dim=-1
        )
        return (q.view(B, S, self.nq, self.hd), k.view(B, S, self.nkv, self.hd),
                v.view(B, S, self.nkv, self.hd))

    def out_proj(self, o, lora=None, li: int = 0):
        y = self.o_proj(o)
        if lora is not None:
            lora.apply_(li, "o_proj", y, o)
        return y

    def ffn(self, x, lora=None, li: int = 0):
        if self.moe is not None:
            return self.moe(x)
        # fused kernel reads both halves of the gate_up output in place
        if lora is None:
            return self.down(OF.glu_fused(self.gate_up(x), gelu=False))
        h = OF.glu_fused(lora.apply_(li, "gate_up", self.gate_up(x), x),
                         gelu=False)
        return lora.apply_(li, "down", self.down(h), h)


class LlamaModel(nn.Module):
    def __init__(self, cfg: LlamaConfig, tp=None, weight_dtype: str = "bf16"):
        """tp: optional parallel.tp.TPGroup — shards every block across the
        group (embed/norms/lm_head replicated; activations stay replicated,
        so logits are identical on every rank and sampling needs no extra
        broadcast).

        weight_dtype="int4" builds qkv, o_proj, gate_up and down of every
        block as QuantLinear modules with empty buffers (for loading a
        quantized state); `quantize_llama_` converts an initialised bf16
        model in place.  weight_dtype="fp8" does the same with Fp8Linear
        modules and `quantize_llama_fp8_`, weight_dtype="mxfp4" with
        Mxfp4Linear modules and `quantize_llama_mxfp4_`."""
        super().__init__()
        self.cfg = cfg
        self.weight_dtype = weight_dtype
        self.tp = tp if (tp is not None and tp.world > 1) else None
        w = self.tp.world if self.tp else 1
        self.embed = nn.Embedding(cfg.vocab_size, cfg.dim)
        self.blocks = nn.ModuleList(
            [LlamaBlock(cfg, tp_world=w, weight_dtype=weight_dtype)
             for _ in range(cfg.n_layers)])
        self.norm = RMSNormK(cfg.dim, cfg.norm_eps)
        self.lm_head = nn.Linear(cfg.dim, cfg.vocab_size, bias=False)
        # NOT buffers: module .to(bf16) must not downcast the f32 trig tables
        # (forced onto cpu so meta-device construction still gets real tables)
        with torch.device("cpu"):
            cos, sin = OF.rope_tables(cfg.max_seq, cfg.head_dim, cfg.rope_base)
        self._rope_cpu = (cos, sin)
        self._rope_cache = {}

    def _ar(self, t):
        """Sum-reduce a row-parallel partial across the TP group (no-op
        single-rank)."""
        return self.tp.all_reduce(t) if self.tp is not None else t

    def _rope_tables(self, device) -> tuple:
        key = str(device)
        if key not in self._rope_cache:
            self._rope_cache[key] = tuple(t.to(device) for t in self._rope_cpu)
        return self._rope_cache[key]

    @torch.no_grad()
    def _lora_rows(self, adapter_idx, lora_bank, rows: int):
        if adapter_idx is None and lora_bank is None:
            return None
        if adapter_idx is None or lora_bank is None:
            raise ValueError("adapter_idx and lora_bank go together")
        if self.tp is not None:
            raise ValueError("LoRA under tensor parallelism is not "
                             "supported")
        if adapter_idx.numel() != rows:
            raise ValueError(f"adapter_idx has {adapter_idx.numel()} "
                             f"entries for {rows} rows")
        return lora_bank.bind(adapter_idx)

    @torch.no_grad()
    def prefill(self, tokens: torch.Tensor, kv_writer=None, last_pos=None,
                adapter_idx=None, lora_bank=None):
        """tokens [B,S] → logits [B, vocab] (last position only).
        kv_writer(layer_idx, k, v): callback storing [B,nkv,S,hd] into cache.
        last_pos [B] int64: per-row index of the last REAL token — the ragged
        path right-pads shorter prompts and samples at each row's own end
        (vLLM-style mixed-length prefill; role of vllm_inference.py:158-209).
        adapter_idx int32 [B,S] with lora_bank (lora.LoraBank): each row's
        adapter slot, -1 = none; the deltas are added after qkv, o_proj,
        gate_up and down.  Without them the forward is the base model's."""
        x = self.embed(tokens)
        lora = self._lora_rows(adapter_idx, lora_bank, tokens.numel())
        rc, rs = self._rope_tables(x.device)
        gpu = x.is_cuda
        for li, blk in enumerate(self.blocks):
            h = blk.attn_norm(x)
            q, k, v = blk.project_qkv(h, lora, li)  # BSHD views
            q = OF.rope(q.transpose(1, 2), rc, rs, inplace=gpu).transpose(1, 2)
            k = OF.rope(k.transpose(1, 2), rc, rs, inplace=gpu).transpose(1, 2)
            if kv_writer is not None:
                kv_writer(li, k, v)  # [B,S,nkv_local,hd]
            o = OF.attention_qkv(q, k, v, causal=True)
            x = x + self._ar(blk.out_proj(o, lora, li))
            x = x + self._ar(blk.ffn(blk.ffn_norm(x), lora, li))
        if last_pos is None:
            x = self.norm(x[:, -1:])
        else:
            idx = last_pos.view(-1, 1, 1).expand(-1, 1, x.shape[-1])
            x = self.norm(x.gather(1, idx))
        return self.lm_head(x)[:, 0].float()

    @torch.no_grad()
    def decode_step(self, tokens, positions, kv_append, kv_attend,
                    adapter_idx=None, lora_bank=None):
        """One token per sequence. tokens [B], positions [B] int32;
        kv_append(li, k, v): store [B,nkv,1,hd] at per-seq positions;
        kv_attend(li, q): paged attention of q [B,nq,hd] vs the cache.
        adapter_idx int32 [B] with lora_bank: as in prefill; the ids are
        read on the device only, so the step still captures into a graph."""
        x = self.embed(tokens).unsqueeze(1)  # [B,1,d]
        lora = self._lora_rows(adapter_idx, lora_bank, tokens.numel())
        rc, rs = self._rope_tables(x.device)
        gpu = x.is_cuda
        for li, blk in enumerate(self.blocks):
            h = blk.attn_norm(x)
            q, k, v = blk.project_qkv(h, lora, li)  # BSHD views [B,1,h,hd]
            q = OF.rope(q.transpose(1, 2), rc, rs, positions=positions,
                        inplace=gpu).transpose(1, 2)
            k = OF.rope(k.transpose(1, 2), rc, rs, positions=positions,
                        inplace=gpu).transpose(1, 2)
            kv_append(li, k, v)  # [B,1,nkv_local,hd]
            o = kv_attend(li, q[:, 0].contiguous() if not q[:, 0].is_contiguous() else q[:, 0])
            x = x + self._ar(blk.out_proj(o.reshape(o.shape[0], 1, -1), lora,
                                          li))
            x = x + self._ar(blk.ffn(blk.ffn_norm(x), lora, li))
        x = self.norm(x[:, -1:])
        return self.lm_head(x)[:, 0].float()


def shard_llama_state(state: dict, cfg: LlamaConfig, rank: int,
                      world: int) -> dict:
    """Slice a FULL single-GPU state dict into rank's TP shard.

    Matches LlamaBlock(tp_world=world): per block, qkv/gate_up rows are this
    rank's q/kv-head and gate/up slices, o_proj/down columns are the
    matching input slices; embed/norms/lm_head replicate.  Used to TP-ify a
    baked checkpoint (fastload file) without materializing N copies.
    """
    hd = cfg.head_dim
    nq_l, nkv_l = cfg.n_heads // world, cfg.n_kv_heads // world
    ffn_l = cfg.ffn_dim // world
    q_off, k_off = 0, cfg.n_heads * hd
    v_off = k_off + cfg.n_kv_heads * hd
    out = {}
    for k, v in state.items():
        if k.endswith(".qkv.weight"):
            rows = torch.cat([
                v[q_off + rank * nq_l * hd: q_off + (rank + 1) * nq_l * hd],
                v[k_off + rank * nkv_l * hd: k_off + (rank + 1) * nkv_l * hd],
                v[v_off + rank * nkv_l * hd: v_off + (rank + 1) * nkv_l * hd],
            ])
            out[k] = rows
        elif k.endswith(".o_proj.weight"):
            out[k] = v[:, rank * nq_l * hd: (rank + 1) * nq_l * hd].contiguous()
        elif k.endswith(".gate_up.weight"):
            out[k] = torch.cat([
                v[rank * ffn_l: (rank + 1) * ffn_l],
                v[cfg.ffn_dim + rank * ffn_l: cfg.ffn_dim + (rank + 1) * ffn_l],
            ])
        elif k.endswith(".down.weight"):
            out[k] = v[:, rank * ffn_l: (rank + 1) * ffn_l].contiguous()
        else:
            out[k] = v
    return out


class MoEFFN(nn.Module):
    """Top-k mixture-of-experts FFN (the MoE model class the reference
    serves: deepseek_v4.py, gpt_oss_inference.py, misc/trtllm_deepseek.py —
    Mixtral/DeepSeek-style routed experts).

    Router scores per token; top-k experts run their SwiGLU on the tokens
    routed to them (token-dispatch loop: E is small, every expert GEMM is a
    dense hipBLASLt call over its token group; glu_fused reads both halves
    of the fused gate_up in place).

    impl="loop" (default) is that host loop: it reads the routing back to
    the host in every call, so it cannot be captured into a graph.
    impl="fused" is router -> ops.moe_route -> ops.moe_ffn: routing, the
    grouped-GEMM schedule, both expert GEMMs and the combine stay on the
    device (csrc/moe.hip), sync-free and capturable; the routing weights
    stay fp32 and each token's expert outputs are summed in fp32.  Shared
    experts, expert parallelism and fp8 expert weights are not supported by
    either.

    expert_dtype="int4" (impl="fused" only) holds the experts as 4-bit
    weights with one bf16 scale per 128 inputs (ops.quantize_w4_experts) in
    four buffers, gate_up_q / gate_up_s / down_q / down_s, instead of the two
    Parameters: 0.52 bytes per weight.  The router stays as it is.  Two
    lanes.  Up to N_KERNEL tokens (decode, speculative verification, small
    chunks) the forward is ops.moe_route -> ops.moe_ffn_w4: the int4 grouped
    GEMMs of csrc/moe.hip, which apply each group's scale to its fp32 partial
    sum and never round a dequantized weight.  Above that (prefill) it is the
    host loop over the active experts, each expert's two matrices
    dequantized into a reusable scratch of the activation dtype just before
    its GEMMs; in bf16 that rounds every scale * q to bf16, like
    QuantLinear's prefill lane, so the two lanes differ by that rounding (in
    fp32 they are the same products).  The prefill lane reads the routing
    back to the host; decode stays under N_KERNEL and captures.

    expert_dtype="mxfp4" (impl="fused" only) holds them as OCP MX fp4: two
    e2m1 codes a byte with one E8M0 scale byte per 32 inputs
    (ops.quantize_mxfp4_experts), 0.53 bytes per weight, in four uint8
    buffers of the same names — the dtype of gate_up_q tells the two packed
    formats apart.  Again two lanes.  Up to N_KERNEL_MXFP4 tokens the forward
    is ops.moe_route -> ops.moe_ffn_mxfp4 (csrc/moe_mxfp4.hip), which
    quantizes x per token and h per (token, expert) row to e4m3 and feeds
    the packed bytes to the block-scaled MFMA as loaded.  Above that it is
    the same dequantize-and-loop lane as int4's: w_hat has two mantissa bits
    and is exact in bf16, and the activations are NOT quantized there, as in
    Mxfp4Linear's prefill lane, so the two lanes differ by the activation
    quantization."""

    IMPLS = ("loop", "fused")

    # tokens up to which the int4 kernel lane is taken.  Measured at the
    # benchmark's expert shape (profiles/moe_ffn_w4.txt, "crossover" lines):
    # the dequantize-and-loop lane pays about 4.6 ms for dequantizing eight
    # experts whatever N, and the kernel lane is still ahead at 4096 tokens
    # (3147 / 5419 us; 1596 / 5092 at 2048).  4096 is the largest measured
    # count, and it is on the kernel's side; the crossover lies above it.
    N_KERNEL = 4096
    # the same for the mxfp4 kernel lane, from its own measurement at the same
    # shape (profiles/moe_ffn_mxfp4.txt, "crossover" lines): dequantizing
    # eight experts in torch ops costs about 16 ms whatever N, and the kernel
    # lane is far ahead at every measured count (2080 / 16844 us at 4096
    # tokens, 1158 / 16483 at 2048).  4096 is the largest measured count; the
    # crossover lies above it.
    N_KERNEL_MXFP4 = 4096

    def __init__(self, dim: int, ffn_dim: int, n_experts: int, top_k: int,
                 impl: str = "loop", expert_dtype: str = "bf16"):
        super().__init__()
        if impl not in self.IMPLS:
            raise ValueError(f"moe impl must be one of {self.IMPLS}, got "
                             f"{impl!r}")
        if expert_dtype not in EXPERT_DTYPES:
            raise ValueError(f"expert_dtype must be one of {EXPERT_DTYPES}, "
                             f"got {expert_dtype!r}")
        self.impl = impl
        self.expert_dtype = "bf16"
        self.dim, self.ffn_dim = dim, ffn_dim
        self.n_experts, self.top_k = n_experts, top_k
        self.router = nn.Linear(dim, n_experts, bias=False)
        if expert_dtype != "bf16":
            # empty packed buffers, for loading a quantized state: zero
            # weights under unit scales (bf16 1, E8M0 byte 127)
            self._check_packed(expert_dtype)
            self.gate_up = self.down = None
            if expert_dtype == "int4":
                qdt, per_q, per_s, sdt, one = (torch.int32, 8, 128,
                                               torch.bfloat16, 1)
            else:
                qdt, per_q, per_s, sdt, one = (torch.uint8, 2, 32,
                                               torch.uint8, 127)
            self._set_packed(
                torch.zeros(n_experts, 2 * ffn_dim, dim // per_q, dtype=qdt),
                torch.full((n_experts, 2 * ffn_dim, dim // per_s), one,
                           dtype=sdt),
                torch.zeros(n_experts, dim, ffn_dim // per_q, dtype=qdt),
                torch.full((n_experts, dim, ffn_dim // per_s), one,
                           dtype=sdt))
            return
        self.gate_up = nn.Parameter(
            torch.empty(n_experts, 2 * ffn_dim, dim).normal_(std=0.02))
        self.down = nn.Parameter(
            torch.empty(n_experts, dim, ffn_dim).normal_(std=0.02))

    def _check_packed(self, expert_dtype):
        if self.impl != "fused":
            raise ValueError(f"expert_dtype={expert_dtype!r} needs "
                             f"moe_impl='fused', got moe_impl={self.impl!r}")
        if self.dim % 128 or self.ffn_dim % 128:
            raise ValueError(f"expert_dtype={expert_dtype!r} needs dim="
                             f"{self.dim} and ffn_dim={self.ffn_dim} to be "
                             f"multiples of 128 (the int4 group, the mxfp4 "
                             f"kernel's chunk)")

    def _set_packed(self, gate_up_q, gate_up_s, down_q, down_s):
        for name, t in (("gate_up_q", gate_up_q), ("gate_up_s", gate_up_s),
                        ("down_q", down_q), ("down_s", down_s)):
            self.register_buffer(name, t)
        self.expert_dtype = _EXPERT_Q_DTYPES[gate_up_q.dtype]
        self._scratch = {}

    def quantize_experts_(self, expert_dtype: str = "int4") -> "MoEFFN":
        """Convert an initialised bf16-expert module in place to
        `expert_dtype` ("int4" or "mxfp4"), one matrix at a time, and free
        the two Parameters."""
        if self.expert_dtype == expert_dtype:
            return self
        if self.expert_dtype != "bf16" or expert_dtype not in _EXPERT_QUANTIZERS:
            raise ValueError(f"cannot quantize {self.expert_dtype} experts to "
                             f"{expert_dtype!r}")
        self._check_packed(expert_dtype)
        packed = []
        for name in ("gate_up", "down"):
            w = getattr(self, name).detach()
            if w.dtype not in (torch.bfloat16, torch.float32):
                w = w.float()
            setattr(self, name, None)  # drops the Parameter
            packed.extend(_EXPERT_QUANTIZERS[expert_dtype](w.contiguous()))
            del w
        self._set_packed(*packed)
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # the buffers' dtype is the format: an int4 state does not load into
        # mxfp4 buffers (copy_ would cast it silently), nor the reverse
        q = state_dict.get(prefix + "gate_up_q")
        if (q is not None and self.expert_dtype != "bf16"
                and _EXPERT_Q_DTYPES.get(q.dtype) != self.expert_dtype):
            raise ValueError(f"{prefix}gate_up_q is {q.dtype}: not an "
                             f"{self.expert_dtype} expert state")
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _apply(self, fn, recurse=True):
        # module.to(dtype) casts every floating buffer; the scales are bf16
        # by format (a round trip through a wider type loses nothing)
        # (mxfp4's four buffers are uint8, which no cast touches)
        super()._apply(fn, recurse)
        if self.expert_dtype == "int4":
            for name in ("gate_up_s", "down_s"):
                t = getattr(self, name)
                if t.dtype is not torch.bfloat16:
                    setattr(self, name, t.to(torch.bfloat16))
        if self.expert_dtype != "bf16":
            self._scratch = {}
        return self

    def _dequantized(self, name, e, dtype):
        """Expert e's matrix `name` in `dtype`, in a scratch reused across
        experts and calls (one per matrix)."""
        q, s = getattr(self, name + "_q")[e], getattr(self, name + "_s")[e]
        int4 = self.expert_dtype == "int4"
        buf = self._scratch.get(name)
        if buf is None or buf.dtype is not dtype or buf.device != q.device:
            buf = torch.empty(q.shape[0], q.shape[1] * (8 if int4 else 2),
                              dtype=dtype, device=q.device)
            self._scratch[name] = buf
        buf.copy_(OF.dequantize_w4(q, s) if int4
                  else OF.dequantize_mxfp4(q, s))
        return buf

    def forward(self, x):
        from ...ops import functional as OF

        B, S, d = x.shape
        flat = x.reshape(-1, d)
        scores = self.router(flat).float()                  # [N, E]
        packed = self.expert_dtype != "bf16"
        if packed:
            ffn, limit = ((OF.moe_ffn_w4, self.N_KERNEL)
                          if self.expert_dtype == "int4"
                          else (OF.moe_ffn_mxfp4, self.N_KERNEL_MXFP4))
            if flat.shape[0] <= limit:
                w, idx = OF.moe_route(scores, self.top_k)
                return ffn(flat.contiguous(), self.gate_up_q, self.gate_up_s,
                           self.down_q, self.down_s, w, idx).view(B, S, d)
        if self.impl == "fused" and not packed:
            w, idx = OF.moe_route(scores, self.top_k)
            return OF.moe_ffn(flat.contiguous(), self.gate_up, self.down, w,
                              idx).view(B, S, d)
        w, idx = scores.topk(self.top_k, dim=-1)            # [N, k]
        w = torch.softmax(w, dim=-1).to(x.dtype)
        out = torch.zeros_like(flat)
        for e in idx.unique().tolist():
            hit = (idx == e)                                # [N, k]
            rows = hit.any(-1).nonzero(as_tuple=True)[0]
            contrib = (w * hit).sum(-1)[rows].unsqueeze(-1)  # routed weight
            if packed:
                gate_up = self._dequantized("gate_up", e, x.dtype)
                down = self._dequantized("down", e, x.dtype)
            else:
                gate_up, down = self.gate_up[e], self.down[e]
            h = OF.glu_fused(flat[rows] @ gate_up.T, gelu=False)
            out[rows] += contrib * (h @ down.T)
        return out.view(B, S, d)
