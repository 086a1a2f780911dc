"""Int4 weight-only linear benchmark: ops.linear_w4 (csrc/linear_w4.hip)
against the bf16 nn.Linear it replaces (hipBLASLt) and against the
dequantize-then-GEMM lane of QuantLinear, on the four Llama-3-8B projections.

Method: one process.  Every arm reads its weights from a rotation of R
copies, R chosen so that the copies together exceed the L2 and the
Infinity Cache (ROTATE_BYTES): each call streams its weights from HBM, as a
decode step does.  An arm is one captured graph of R calls, one per copy, so
the time is device time with the calls back to back and no host gaps — the
engine replays its decode step the same way.  Arms are warmed, then timed in
alternation (ROUNDS windows each); reported per arm: median microseconds per
call and the arm's own weight bytes over that time.

--sweep adds, per shape, the kernel under forced split counts (the binding's
test-only argument): the data behind the split rule.

Usage: python scripts/bench_linear_w4.py [--rows 1 8 32] [--sweep] [--out F]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = (("qkv", 6144, 4096), ("o_proj", 4096, 4096),
          ("gate_up", 28672, 4096), ("down", 4096, 14336))
ROWS = (1, 8, 32, 64, 128, 256)
ROTATE_BYTES = 600 << 20   # > 4 MB L2 + 256 MB Infinity Cache, with margin
MAX_COPIES = 64
ROUNDS = 5
WINDOW_S = 0.08


def w4_bytes(N, K):
    return N * K // 2 + N * (K // 128) * 2


def copies_for(nbytes):
    return max(2, min(MAX_COPIES, -(-ROTATE_BYTES // nbytes)))


def capture(call, R):
    """One graph of call(0) .. call(R-1)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(0)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(R):
            call(i)
    return g


def _window(g, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per replay


def time_graphs(graphs):
    """graphs: {name: (graph, R)} -> {name: (median, min, max) us per call},
    windows of the arms alternating."""
    reps = {}
    for n, (g, R) in graphs.items():
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        reps[n] = max(2, int(WINDOW_S * 1e6 / _window(g, 2)))
    samples = {n: [] for n in graphs}
    for _ in range(ROUNDS):
        for n, (g, R) in graphs.items():
            samples[n].append(_window(g, reps[n]) / R)
    return {n: (statistics.median(s), min(s), max(s))
            for n, s in samples.items()}


def bench_shape(name, N, K, rows, sweep, out):
    from modal_examples_amd.ops import functional as OF
    from modal_examples_amd.ops._build import get_ext

    ext = get_ext(required=True)
    gen = torch.Generator(device="cuda").manual_seed(N + K)
    Rq, Rb = copies_for(w4_bytes(N, K)), copies_for(2 * N * K)
    qw = [torch.randint(-2 ** 31, 2 ** 31 - 1, (N, K // 8), device="cuda",
                        dtype=torch.int32, generator=gen) for _ in range(Rq)]
    sc = [(0.003 * (1 + torch.rand(N, K // 128, device="cuda", generator=gen))
           ).to(torch.bfloat16) for _ in range(Rq)]
    wb = [(0.02 * torch.randn(N, K, device="cuda", generator=gen)
           ).to(torch.bfloat16) for _ in range(Rb)]
    out(f"## {name}: N={N} K={K}; int4 {w4_bytes(N, K) / 1e6:.1f} MB x {Rq} "
        f"copies, bf16 {2 * N * K / 1e6:.1f} MB x {Rb} copies; split rule "
        f"S={ext.linear_w4_splits(1, N, K)}")
    with torch.no_grad():
        for M in rows:
            x = torch.randn(M, K, device="cuda", generator=gen).to(torch.bfloat16)

            def deq(i):
                w = OF.dequantize_w4(qw[i], sc[i]).to(torch.bfloat16)
                return torch.nn.functional.linear(x, w)

            graphs = {
                "w4": (capture(lambda i: OF.linear_w4(x, qw[i], sc[i]), Rq), Rq),
                "bf16": (capture(
                    lambda i: torch.nn.functional.linear(x, wb[i]), Rb), Rb),
                "dequant": (capture(deq, 2), 2),
            }
            res = time_graphs(graphs)
            nbytes = {"w4": w4_bytes(N, K), "bf16": 2 * N * K,
                      "dequant": w4_bytes(N, K)}
            line = f"{name:8s} M={M:4d}"
            for n in ("w4", "bf16", "dequant"):
                med, lo, hi = res[n]
                line += (f" | {n} {med:8.1f} us [{lo:.1f}..{hi:.1f}] "
                         f"{nbytes[n] / med / 1e3:7.1f} GB/s")
            line += f" | bf16/w4 {res['bf16'][0] / res['w4'][0]:.2f}x"
            out(line)
            del graphs
            if sweep and M in (1, 32):
                nch = K // 128
                cands = sorted({min(nch, max(1, -(-t // (N // 64))))
                                for t in (128, 256, 512, 1024, 2048, 4096)})
                sg = {f"S={s}": (capture(
                    lambda i, s=s: ext.linear_w4(x, qw[i], sc[i], s), Rq), Rq)
                    for s in cands}
                sres = time_graphs(sg)
                out(f"{name:8s} M={M:4d} splits sweep: " + "  ".join(
                    f"{n} ({int(n[2:]) * (N // 64)} waves) {v[0]:.1f} us"
                    for n, v in sres.items()))
                del sg
    del qw, sc, wb
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=list(ROWS))
    ap.add_argument("--shapes", nargs="+", default=[s[0] for s in SHAPES])
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None, help="also append the lines here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_w4.py measures on a GPU; none found")

    def out(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    out(f"# bench_linear_w4: {torch.cuda.get_device_name(0)}; us per call, "
        f"median [min..max] of {ROUNDS} windows, weights rotated through "
        f">= {ROTATE_BYTES >> 20} MB; GB/s = the arm's weight bytes / time")
    for name, N, K in SHAPES:
        if name in a.shapes:
            bench_shape(name, N, K, a.rows, a.sweep, out)


if __name__ == "__main__":
    main()
