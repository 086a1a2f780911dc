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

--expert-dtype int4 adds the int4-expert lane (ops.moe_ffn_w4) on the same
weights, quantized, to the same alternation: moe_ffn_w4_only, fused_w4,
fused_w4_graph, and dequant_loop_w4, MoEFFN's prefill lane forced at every N
(the crossover of the two lanes fixes MoEFFN.N_KERNEL).  Its bytes count
0.52 B per weight (4 bits + one bf16 scale per 128).  --w4-sweep also times
ops.moe_ffn_w4 with the down GEMM's K forced into 1, 2, 4 and 8 slices,
beside the shipped rule.

--expert-dtype mxfp4 does the same for the MXFP4-expert lane
(ops.moe_ffn_mxfp4, csrc/moe_mxfp4.hip): moe_ffn_mxfp4_only, fused_mxfp4,
fused_mxfp4_graph, dequant_loop_mxfp4 and, with --w4-sweep, mxfp4_only[sS].
Its yardsticks, moe_ffn_only (bf16) and moe_ffn_w4_only (int4), run in the
same alternation on the same weights.  Its bytes count 0.53 B per weight
(4 bits + one E8M0 byte per 32) and the lane's own workspaces (xq, hq).

Usage: python scripts/bench_moe.py [--tokens 64 256 4096] [--e2e]
                                   [--expert-dtype int4|mxfp4] [--w4-sweep]
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


W4_BYTES = 0.5 + 2 / 128   # per weight: a nibble + a bf16 scale per 128
W4_DOWN_SLICES = 2         # csrc/moe.hip's rule: min(2, ffn / 128)
W4_SWEEP = (1, 2, 4, 8)    # K slices of the down GEMM, forced
MX_BYTES = 0.5 + 1 / 32    # per weight: a nibble + an E8M0 byte per 32
MX_DOWN_SLICES = 1         # csrc/moe_mxfp4.hip's rule: one slice


def ffn_bytes(N, dim, ffn, k, touched, slots, wbytes=2, planes=1):
    """Algorithmic bytes of ops.moe_ffn: every touched expert's weights
    once, x and out, the bf16 h and fp32 y workspaces written and read."""
    weights = touched * 3 * ffn * dim * wbytes
    act = 2 * N * dim * 2
    work = 2 * slots * ffn * 2 + 2 * planes * N * k * dim * 4
    return int(weights), act + work


def _capture(module, static_x):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            module(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        module(static_x)
    return graph


def packed_arms(kind, loop, x, flat, w, idx, sweep, only=False):
    """The arms of packed format `kind` ("w4" or "mxfp4") over loop's
    weights, quantized; (arms, graph, fused module).  only=True builds the
    moe_ffn_<kind>_only arm alone (a yardstick for another format's run)."""
    from modal_examples_amd.models.llama.model import MoEFFN
    from modal_examples_amd.ops import functional as OF
    from modal_examples_amd.ops._build import get_ext

    E, _, dim = loop.gate_up.shape
    ffn, k = loop.down.shape[2], loop.top_k
    w4 = kind == "w4"
    quantize = OF.quantize_w4_experts if w4 else OF.quantize_mxfp4_experts
    ffn_op = OF.moe_ffn_w4 if w4 else OF.moe_ffn_mxfp4
    packed = quantize(loop.gate_up.data) + quantize(loop.down.data)
    arms = {f"moe_ffn_{kind}_only": lambda: ffn_op(flat, *packed, w, idx)}
    if only:
        return arms, None, None
    limit = "N_KERNEL" if w4 else "N_KERNEL_MXFP4"
    mods = []
    for _ in range(2):
        with torch.device("meta"):
            m = MoEFFN(dim, ffn, E, k, impl="fused",
                       expert_dtype="int4" if w4 else "mxfp4")
        m.router = loop.router
        m.gate_up_q, m.gate_up_s, m.down_q, m.down_s = packed
        mods.append(m)
    fused_q, prefill_q = mods
    setattr(fused_q, limit, 1 << 30)  # this arm is the kernel lane at every N
    setattr(prefill_q, limit, 0)      # and this one the dequantize-and-loop lane
    graph = _capture(fused_q, x.clone())
    arms.update({
        f"fused_{kind}": lambda: fused_q(x),
        f"fused_{kind}_graph": graph.replay,
        f"dequant_loop_{kind}": lambda: prefill_q(x),
    })
    if sweep:
        ext = get_ext(required=True)
        forced = ext.moe_ffn_w4 if w4 else ext.moe_ffn_mxfp4
        for s in W4_SWEEP:
            if s <= ffn // 128:
                arms[f"{kind}_only[s{s}]"] = (
                    lambda s=s: forced(flat, *packed, w, idx, s))
    return arms, graph, fused_q


def bench_ffn(N, dim, ffn, E, k, out, expert_dtype="bf16", sweep=False):
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
        kind = {"int4": "w4", "mxfp4": "mxfp4"}.get(expert_dtype)
        if kind == "mxfp4":  # the int4 kernel lane is a yardstick here
            arms.update(packed_arms("w4", loop, x, flat, w, idx, False,
                                    only=True)[0])
        if kind:
            more, graph_q, fused_q = packed_arms(kind, loop, x, flat, w, idx,
                                                 sweep)
            arms.update(more)
        res = time_arms(arms)
        diff = (fused(x).float() - loop(x).float()).abs().max().item()
        if kind:
            diff_q = (fused_q(x).float() - fused(x).float()).abs().max().item()
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
    if kind:
        a, b = res[f"moe_ffn_{kind}_only"], res["moe_ffn_only"]
        tq = a[0] * 1e-6
        if kind == "w4":
            planes = min(W4_DOWN_SLICES, ffn // 128)
            wbq, obq = ffn_bytes(N, dim, ffn, k, touched, slots, W4_BYTES,
                                 planes)
        else:
            planes = min(MX_DOWN_SLICES, ffn // 128)
            wbq, obq = ffn_bytes(N, dim, ffn, k, touched, slots, MX_BYTES,
                                 planes)
            # xq written once, read by every up tile row; hq written and read
            obq += 2 * N * dim + 2 * slots * ffn
        out(f"N={N:5d} {expert_dtype}/bf16 moe_ffn_only = {a[0] / b[0]:.3f} "
            f"({b[0] / a[0]:.2f}x; spreads: {expert_dtype} {a[2] - a[1]:.1f} "
            f"us, bf16 {b[2] - b[1]:.1f} us, gap {b[0] - a[0]:.1f} us)   "
            f"max|fused_{kind}-fused| = {diff_q:.3e} (quantization included)")
        if kind == "mxfp4":
            c = res["moe_ffn_w4_only"]
            out(f"N={N:5d} mxfp4/int4 moe_ffn_only = {a[0] / c[0]:.3f} "
                f"({c[0] / a[0]:.2f}x; spreads: mxfp4 {a[2] - a[1]:.1f} us, "
                f"int4 {c[2] - c[1]:.1f} us, gap {c[0] - a[0]:.1f} us)")
        out(f"N={N:5d} moe_ffn_{kind}_only: {wbq / 1e6:.1f} MB weights + "
            f"{obq / 1e6:.1f} MB activations/workspaces -> "
            f"{(wbq + obq) / tq / 1e12:.2f} TB/s algorithmic = "
            f"{(wbq + obq) / tq / 1e12 / HBM_COPY_TBS:.0%} of the "
            f"{HBM_COPY_TBS} TB/s copy rate")
        out(f"N={N:5d} crossover: kernel lane {res[f'fused_{kind}'][0]:.1f} us, "
            f"dequantize-and-loop lane {res[f'dequant_loop_{kind}'][0]:.1f} us")
        del graph_q
    del graph


def bench_e2e(out, layers=8, batch=64, steps=24, expert_dtype="bf16"):
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    lanes = [("loop", False, "bf16"), ("fused", False, "bf16"),
             ("fused", True, "bf16")]
    if expert_dtype != "bf16":
        lanes += [("fused", False, expert_dtype), ("fused", True, expert_dtype)]
    for impl, graph, edt in lanes:
        torch.manual_seed(0)
        cfg = LlamaConfig(n_experts=8, ffn_dim=4096, n_layers=layers)
        eng = LlamaEngine(cfg, device="cuda", dtype=torch.bfloat16,
                          moe_impl=impl, use_graph=graph, kv_blocks=4096,
                          max_batch=batch, eos_id=-1, expert_dtype=edt)
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
            f"experts={edt:4s} graph={graph!s:5s} {(n1 - n0) / dt:9.1f} tok/s "
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
    ap.add_argument("--expert-dtype", choices=("bf16", "int4", "mxfp4"),
                    default="bf16")
    ap.add_argument("--w4-sweep", action="store_true")
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
        bench_ffn(N, a.dim, a.ffn, a.experts, a.top_k, out, a.expert_dtype,
                  a.w4_sweep)
    if a.e2e:
        bench_e2e(out, expert_dtype=a.expert_dtype)


if __name__ == "__main__":
    main()
