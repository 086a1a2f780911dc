"""MoE FFN benchmark: the host loop of MoEFFN(impl="loop") against the fused
lane (ops.moe_route + ops.moe_ffn, csrc/moe.hip) on one GPU.

Method: one process; per token count both arms are built on the same
weights and warmed, then timed in alternation (loop window, fused window,
... ROUNDS times), each window bracketed by device events and long enough
to fill a good fraction of a second.  Reported per arm: median / min / max
microseconds per forward over the windows.  The loop arm's host round trips
are inside its windows — they are what a decode step pays.

Also reported: ops.moe_ffn alone (routing given) with its algorithmic bytes
over time against the measured HBM copy rate, the fused forward replayed
from a captured graph, and (--e2e) decode tokens/s of an 8-layer cut of the
serving example for loop+eager, fused+eager and fused+graph.

Usage: python scripts/bench_moe.py [--tokens 64 256 4096] [--e2e]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBS = 6.29   # measured float4-copy rate of the MI355X (8.0 spec)
ROUNDS = 5
WINDOW_S = 0.3


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


def ffn_bytes(N, dim, ffn, k, touched, slots):
    """Algorithmic bytes of ops.moe_ffn: every touched expert's weights
    once, x and out, the bf16 h and fp32 y workspaces written and read."""
    weights = touched * 3 * ffn * dim * 2
    act = 2 * N * dim * 2
    work = 2 * slots * ffn * 2 + 2 * N * k * dim * 4
    return weights, act + work


def bench_ffn(N, dim, ffn, E, k, out):
    from modal_examples_amd.models.llama.model import MoEFFN
    from modal_examples_amd.ops import functional as OF

    torch.manual_seed(0)
    with torch.device("cuda"):
        loop = MoEFFN(dim, ffn, E, k, impl="loop").to(torch.bfloat16).eval()
    with torch.device("meta"):  # shares the loop arm's parameters
        fused = MoEFFN(dim, ffn, E, k, impl="fused")
    fused.router, fused.gate_up, fused.down = loop.router, loop.gate_up, loop.down
    x = torch.randn(1, N, dim, device="cuda").to(torch.bfloat16)
    with torch.no_grad():
        w, idx = OF.moe_route(loop.router(x[0]).float(), k)
        flat = x[0].contiguous()
        static_x = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fused(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fused(static_x)
        arms = {
            "loop": lambda: loop(x),
            "fused": lambda: fused(x),
            "fused_graph": graph.replay,
            "moe_ffn_only": lambda: OF.moe_ffn(flat, loop.gate_up, loop.down,
                                               w, idx),
        }
        res = time_arms(arms)
        diff = (fused(x).float() - loop(x).float()).abs().max().item()
    counts = torch.bincount(idx.flatten().long(), minlength=E)
    touched = int((counts > 0).sum())
    slots = int(((counts + 31) // 32 * 32).sum())
    wb, ob = ffn_bytes(N, dim, ffn, k, touched, slots)
    for n, (med, lo, hi, it) in res.items():
        out(f"N={N:5d} {n:13s} {med:9.1f} us  (min {lo:.1f} max {hi:.1f}, "
            f"{ROUNDS} windows x {it} calls)")
    t = res["moe_ffn_only"][0] * 1e-6
    out(f"N={N:5d} loop/fused = {res['loop'][0] / res['fused'][0]:.2f}x   "
        f"max|fused-loop| = {diff:.3e}")
    out(f"N={N:5d} moe_ffn_only: {touched}/{E} experts touched, "
        f"{wb / 1e6:.1f} MB weights + {ob / 1e6:.1f} MB activations/workspaces"
        f" -> {(wb + ob) / t / 1e12:.2f} TB/s algorithmic = "
        f"{(wb + ob) / t / 1e12 / HBM_COPY_TBS:.0%} of the {HBM_COPY_TBS} TB/s"
        f" copy rate (memory bound: {2 * 3 * N * k * dim * ffn / t / 1e12:.0f}"
        f" TFLOP/s is far below the MFMA peak)")
    del graph


def bench_e2e(out, layers=8, batch=64, steps=24):
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    for impl, graph in (("loop", False), ("fused", False), ("fused", True)):
        torch.manual_seed(0)
        cfg = LlamaConfig(n_experts=8, ffn_dim=4096, n_layers=layers)
        eng = LlamaEngine(cfg, device="cuda", dtype=torch.bfloat16,
                          moe_impl=impl, use_graph=graph, kv_blocks=4096,
                          max_batch=batch, eos_id=-1)
        for i in range(batch):
            eng.add_request([1 + i, 7, 9, 11], max_new_tokens=steps + 16,
                            temperature=0.0)
        while len(eng.running) < batch or any(
                len(r.out_tokens) < 4 for r in eng.running):
            eng.step()
        torch.cuda.synchronize()
        n0 = sum(len(r.out_tokens) for r in eng.running)
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n1 = sum(len(r.out_tokens) for r in eng.running)
        out(f"e2e {layers} layers batch {batch}: moe_impl={impl:5s} "
            f"graph={graph!s:5s} {(n1 - n0) / dt:9.1f} tok/s "
            f"({dt / steps * 1e3:.2f} ms/step over {steps} steps)")
        eng.close()
        del eng
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, nargs="+", default=[64, 256, 4096])
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--ffn", type=int, default=4096)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--top-k", type=int, default=2)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default=None, help="also append the lines here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe.py measures on a GPU; none found")

    def out(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    out(f"# bench_moe: dim={a.dim} ffn={a.ffn} E={a.experts} k={a.top_k} bf16,"
        f" {torch.cuda.get_device_name(0)}")
    for N in a.tokens:
        bench_ffn(N, a.dim, a.ffn, a.experts, a.top_k, out)
    if a.e2e:
        bench_e2e(out)


if __name__ == "__main__":
    main()
