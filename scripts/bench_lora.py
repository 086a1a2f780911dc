"""Multi-LoRA benchmark: ops.lora_apply_ (csrc/lora.hip) against the host-loop
composition, at Llama-3-8B's four projection shapes on one GPU.

Method (as scripts/bench_moe.py): one process; per (projection, N, distinct
adapters in the batch) all arms are built on the same tensors and warmed,
then timed in alternation (ROUNDS windows each), every window bracketed by
device events.  Reported per arm: median / min / max microseconds per call.

  lora_op     ops.lora_apply_ with the schedule given (one schedule serves
              every projection of a forward; `schedule` times it alone)
  host_loop   the composition a host would run: read idx back, then per
              adapter index_select its rows, two GEMMs, index_add_ — the
              read-back is inside the window, it is what a decode step pays
  base_gemm   the projection's own x @ W^T, to state the adapter overhead as
              a share of the projection

--sweep adds, at N = 64 with 4 adapters, the shrink GEMM's K forced into 1,
2, 4, 8 and 16 slices and the untransposed expand layout, beside the shipped
rule.  --e2e adds decode tokens/s of an 8-layer cut of Llama-3-8B at batch 64
for lora_slots=0, slots allocated but unused, and four adapters mixed.

Usage: python scripts/bench_lora.py [--tokens 1 64 256 2048] [--sweep] [--e2e]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS = 5
WINDOW_S = 0.1
SLOTS, RANK = 16, 16
SWEEP_SLICES = (1, 2, 4, 8, 16)


def _window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def _iters_for(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return max(3, int(WINDOW_S * 1e6 / _window(fn, 5)))


def time_arms(arms):
    """arms: {name: fn}.  Warm all, then alternate windows; us per call."""
    iters = {n: _iters_for(f) for n, f in arms.items()}
    samples = {n: [] for n in arms}
    for _ in range(ROUNDS):
        for n, f in arms.items():
            samples[n].append(_window(f, iters[n]))
    return {n: (statistics.median(s), min(s), max(s), iters[n])
            for n, s in samples.items()}


def host_loop(y, x, bank_a, bank_b, idx):
    """The composition without the kernel: one pass per adapter present."""
    for s in idx.unique().tolist():  # the read-back
        if s < 0:
            continue
        rows = (idx == s).nonzero(as_tuple=True)[0]
        t = x.index_select(0, rows) @ bank_a[s].T
        y.index_add_(0, rows, t @ bank_b[s].T)
    return y


def bench_projection(name, K, O, N, adapters, out, sweep):
    from modal_examples_amd.ops import functional as OF
    from modal_examples_amd.ops._build import get_ext

    g = torch.Generator().manual_seed(0)
    dev, bf = "cuda", torch.bfloat16
    x = torch.randn(N, K, generator=g).to(dev, bf)
    w = (torch.randn(O, K, generator=g) * K ** -0.5).to(dev, bf)
    bank_a = (torch.randn(SLOTS, RANK, K, generator=g) * K ** -0.5).to(dev, bf)
    bank_b = (torch.randn(SLOTS, O, RANK, generator=g) * 0.1).to(dev, bf)
    idx = (torch.arange(N) % min(adapters, N)).to(torch.int32).to(dev)
    y = torch.randn(N, O, generator=g).to(dev, bf)
    sched = OF.lora_schedule(idx, SLOTS)
    arms = {
        "lora_op": lambda: OF.lora_apply_(y, x, bank_a, bank_b, sched),
        "schedule": lambda: OF.lora_schedule(idx, SLOTS),
        "host_loop": lambda: host_loop(y, x, bank_a, bank_b, idx),
        "base_gemm": lambda: torch.nn.functional.linear(x, w),
    }
    if sweep:
        ext = get_ext(required=True)
        for z in SWEEP_SLICES:
            if ext.lora_slices(K, z) >= 1:
                arms[f"lora_op[z{z}]"] = lambda z=z: ext.lora_apply_(
                    y, x, bank_a, bank_b, sched.sched, z, True)
        arms["lora_op[noswap]"] = lambda: ext.lora_apply_(
            y, x, bank_a, bank_b, sched.sched, 0, False)
    res = time_arms(arms)
    base = res["base_gemm"][0]
    for arm, (med, lo, hi, iters) in res.items():
        line = (f"{name:8s} K={K:5d} O={O:5d} N={N:4d} adapters={adapters:2d} "
                f"{arm:16s} {med:9.1f} us  [{lo:9.1f} .. {hi:9.1f}] x{iters}")
        if arm == "lora_op":
            line += (f"  = {med / base:5.2f} x base_gemm, host_loop / lora_op "
                     f"= {res['host_loop'][0] / med:5.2f}")
        print(line, flush=True)
        out.append(line)


def bench_e2e(out, batch=64, steps=20):
    """Decode tokens/s of an 8-layer Llama-3-8B cut, three engines alternated
    in windows of `steps` decode steps."""
    import dataclasses

    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.lora import projection_shapes
    from modal_examples_amd.models.llama.model import LlamaConfig

    cfg = dataclasses.replace(LlamaConfig.llama3_8b(), n_layers=8)
    g = torch.Generator().manual_seed(1)
    engines = {}
    for arm, slots in (("slots0", 0), ("slots4_unused", 4),
                       ("slots4_mixed", 4)):
        torch.manual_seed(0)
        eng = LlamaEngine(cfg, max_batch=batch, kv_blocks=4096, eos_id=-1,
                          lora_slots=slots)
        names = [None]
        if arm == "slots4_mixed":
            for a in range(4):
                state = {}
                for li in range(cfg.n_layers):
                    for t, (i, o) in projection_shapes(cfg).items():
                        state[f"blocks.{li}.{t}.lora_a"] = \
                            torch.randn(16, i, generator=g) * 0.01
                        state[f"blocks.{li}.{t}.lora_b"] = \
                            torch.randn(o, 16, generator=g) * 0.01
                eng.load_adapter(f"a{a}", state)
            names = [f"a{a}" for a in range(4)]
        for i in range(batch):
            eng.add_request([1 + (i * 13 + j) % 1000 for j in range(32)],
                            max_new_tokens=(ROUNDS + 2) * steps + 8,
                            adapter=names[i % len(names)])
        for _ in range(steps):  # prefill, capture, warm
            eng.step()
        engines[arm] = eng
    samples = {arm: [] for arm in engines}
    for _ in range(ROUNDS):
        for arm, eng in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                eng.step()
            torch.cuda.synchronize()
            samples[arm].append(batch * steps / (time.perf_counter() - t0))
    for arm, s in samples.items():
        assert len(engines[arm].running) == batch
        line = (f"e2e 8-layer batch={batch} {arm:14s} "
                f"{statistics.median(s):9.0f} tok/s  [{min(s):9.0f} .. "
                f"{max(s):9.0f}]")
        print(line, flush=True)
        out.append(line)
        engines[arm].close()


def main():
    from modal_examples_amd.models.llama.lora import projection_shapes
    from modal_examples_amd.models.llama.model import LlamaConfig

    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="*", default=[1, 64, 256, 2048])
    ap.add_argument("--adapters", type=int, nargs="*", default=[1, 4, 16])
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = []
    shapes = projection_shapes(LlamaConfig.llama3_8b())
    for name, (K, O) in shapes.items():
        for N in args.tokens:
            for adapters in args.adapters:
                if adapters > N and adapters != args.adapters[0]:
                    continue  # N = 1 has one adapter whatever is asked
                bench_projection(name, K, O, N, adapters, out, False)
    if args.sweep:
        for name, (K, O) in shapes.items():
            bench_projection(name, K, O, 64, 4, out, True)
    if args.e2e:
        bench_e2e(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
