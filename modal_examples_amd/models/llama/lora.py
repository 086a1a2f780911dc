"""Adapter banks for multi-LoRA serving: one base model, up to 32 adapters
resident, chosen per row of a batch (ops.lora_apply_, csrc/lora.hip).

A bank holds, for every targeted projection of every layer, the stacked
adapter matrices of all slots: a[target] [L, S, R, in] and b[target]
[L, S, out, R] in the model's dtype.  Adapters of a lower rank sit
zero-padded; alpha / r is folded into b in fp32 before the one rounding.  The
bank lives outside the module tree: the base model's state dict and its
no-adapter forward do not know it exists.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from ...ops import functional as OF

LORA_TARGETS = ("qkv", "o_proj", "gate_up", "down")
LORA_RANKS = (16, 32, 64)
LORA_MAX_SLOTS = 32


def projection_shapes(cfg) -> Dict[str, Tuple[int, int]]:
    """(in, out) of each targetable projection of an unsharded block."""
    d, hd = cfg.dim, cfg.head_dim
    return {"qkv": (d, (cfg.n_heads + 2 * cfg.n_kv_heads) * hd),
            "o_proj": (cfg.n_heads * hd, d),
            "gate_up": (d, 2 * cfg.ffn_dim),
            "down": (cfg.ffn_dim, d)}


class LoraBank:
    def __init__(self, cfg, slots: int, rank: int = 16,
                 targets: Optional[Sequence[str]] = None, device="cpu",
                 dtype=torch.bfloat16):
        if isinstance(slots, bool) or not isinstance(slots, int) \
                or not 1 <= slots <= LORA_MAX_SLOTS:
            raise ValueError(f"lora_slots={slots!r} (supported: 1.."
                             f"{LORA_MAX_SLOTS})")
        if rank not in LORA_RANKS:
            raise ValueError(f"lora_rank={rank!r} (supported: {LORA_RANKS})")
        moe = cfg.n_experts > 0
        if targets is None:
            targets = LORA_TARGETS[:2] if moe else LORA_TARGETS
        targets = tuple(targets)
        for t in targets:
            if t not in LORA_TARGETS:
                raise ValueError(f"lora target {t!r} is not one of "
                                 f"{LORA_TARGETS}")
            if moe and t in ("gate_up", "down"):
                raise ValueError(f"lora target {t!r} is not supported on an "
                                 f"MoE config (qkv and o_proj are)")
        if not targets:
            raise ValueError("lora_targets is empty")
        self.slots, self.rank, self.targets = slots, rank, targets
        self.n_layers = cfg.n_layers
        self.shapes = {t: projection_shapes(cfg)[t] for t in targets}
        self.a: Dict[str, torch.Tensor] = {}
        self.b: Dict[str, torch.Tensor] = {}
        for t, (i, o) in self.shapes.items():
            self.a[t] = torch.zeros(cfg.n_layers, slots, rank, i,
                                    device=device, dtype=dtype)
            self.b[t] = torch.zeros(cfg.n_layers, slots, o, rank,
                                    device=device, dtype=dtype)

    def parse_state(self, state: Dict[str, torch.Tensor]):
        """Adapter tensors by (layer, target): the `blocks.<i>.<proj>.lora_a`
        [r, in] / `.lora_b` [out, r] names train.lora.lora_state_dict gives a
        wrapped LlamaModel.  Returns ({(layer, target): (a, b)}, r)."""
        pairs: Dict[tuple, dict] = {}
        for key, t in state.items():
            parts = key.split(".")
            if (len(parts) != 4 or parts[0] != "blocks"
                    or not parts[1].isdigit()
                    or parts[3] not in ("lora_a", "lora_b")):
                raise ValueError(f"adapter key {key!r} is not "
                                 f"blocks.<layer>.<projection>.lora_a/lora_b")
            li, name = int(parts[1]), parts[2]
            if name not in self.targets or li >= self.n_layers:
                raise ValueError(f"adapter key {key!r}: the engine's "
                                 f"lora_targets are {self.targets} over "
                                 f"{self.n_layers} layers")
            pairs.setdefault((li, name), {})[parts[3]] = t
        if not pairs:
            raise ValueError("adapter state is empty")
        r = None
        out = {}
        for (li, name), p in pairs.items():
            if set(p) != {"lora_a", "lora_b"}:
                raise ValueError(f"blocks.{li}.{name}: lora_a and lora_b "
                                 f"must both be given")
            a, b = p["lora_a"], p["lora_b"]
            i, o = self.shapes[name]
            if a.dim() != 2 or b.dim() != 2 or a.shape[1] != i \
                    or b.shape[0] != o or a.shape[0] != b.shape[1]:
                raise ValueError(
                    f"blocks.{li}.{name}: lora_a {tuple(a.shape)} / lora_b "
                    f"{tuple(b.shape)} do not match [r, {i}] / [{o}, r]")
            if r is None:
                r = a.shape[0]
            if a.shape[0] != r or not 1 <= r <= self.rank:
                raise ValueError(
                    f"blocks.{li}.{name}: rank {a.shape[0]} (one rank per "
                    f"adapter, at most the bank's {self.rank})")
            out[(li, name)] = (a, b)
        return out, r

    @torch.no_grad()
    def write(self, slot: int, state: Dict[str, torch.Tensor],
              alpha: float) -> None:
        """Put an adapter into `slot`: pad to the bank rank, fold alpha / r
        into b in fp32, round once.  Projections the adapter does not cover
        are zero there."""
        pairs, r = self.parse_state(state)
        scale = float(alpha) / r
        self.clear(slot)
        for (li, name), (a, b) in pairs.items():
            ta, tb = self.a[name], self.b[name]
            ta[li, slot, :r] = a.detach().to(ta.device, torch.float32) \
                .to(ta.dtype)
            tb[li, slot, :, :r] = (b.detach().to(tb.device, torch.float32)
                                   * scale).to(tb.dtype)

    @torch.no_grad()
    def clear(self, slot: int) -> None:
        for t in self.targets:
            self.a[t][:, slot].zero_()
            self.b[t][:, slot].zero_()

    def bind(self, adapter_idx: torch.Tensor) -> "LoraRows":
        """The per-forward view: the row schedule of `adapter_idx` (int32,
        one adapter slot per row of the flattened batch, -1 = none), built
        once and shared by every projection of every layer."""
        return LoraRows(self, OF.lora_schedule(
            adapter_idx.reshape(-1).to(torch.int32).contiguous(), self.slots))


class LoraRows:
    def __init__(self, bank: LoraBank, sched):
        self.bank, self.sched = bank, sched

    def apply_(self, li: int, name: str, y: torch.Tensor, x: torch.Tensor):
        """Add layer li's `name` deltas to the projection output y (input
        x), in place; y is returned.  A projection outside the bank's
        targets is left alone."""
        if name not in self.bank.a:
            return y
        y2 = y.view(-1, y.shape[-1])
        OF.lora_apply_(y2, x.reshape(-1, x.shape[-1]).contiguous(),
                       self.bank.a[name][li], self.bank.b[name][li],
                       self.sched)
        return y
