#!/usr/bin/env python3
"""Per-kernel micro-benchmarks vs speed-of-light on MI355X.

Ceilings (MI355X_MICROARCH.md): bf16 MFMA dense ≈2.5 PF, HBM ≈8 TB/s peak
(~6.3 achievable).  Prints TFLOP/s for compute kernels and GB/s for
memory-bound ones, with % of the relevant ceiling.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import modal_examples_amd.ops.functional as F  # noqa: E402

HBM_CEIL_GBS = 6300.0
MFMA_CEIL_TF = 2500.0


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_attention(results):
    shapes = [
        ("sdxl_self_s4096_d64", 4, 10, 4096, 4096, 64, False),
        ("sdxl_cross_s4096_kv77", 4, 10, 4096, 77, 64, False),
        ("sdxl_self_s1024_d64", 4, 20, 1024, 1024, 64, False),
        ("whisper_enc_s1500_d64", 8, 20, 1500, 1500, 64, False),
        ("llama_prefill_s2048_d128", 1, 32, 2048, 2048, 128, True),
        ("llama_prefill_s8192_d128", 1, 32, 8192, 8192, 128, True),
    ]
    for name, B, H, Sq, Sk, D, causal in shapes:
        q = torch.randn(B, H, Sq, D, device="cuda", dtype=torch.bfloat16)
        kv_h = H if "llama" not in name else 8
        k = torch.randn(B, kv_h, Sk, D, device="cuda", dtype=torch.bfloat16)
        v = torch.randn(B, kv_h, Sk, D, device="cuda", dtype=torch.bfloat16)
        dt = timeit(lambda: F.attention(q, k, v, causal=causal))
        flops = 4.0 * B * H * Sq * Sk * D * (0.5 if causal else 1.0)
        tf = flops / dt / 1e12
        results[f"attn/{name}"] = {"ms": round(dt * 1e3, 3), "TF": round(tf, 1),
                                   "pct_peak": round(100 * tf / MFMA_CEIL_TF, 1)}


def bench_attention_bwd(results):
    """Forward+backward through F.attention: the HIP backward against the
    same call under MODAL_AMD_ATTN_BWD=ref (differentiable reference math,
    the behaviour before the backward kernel existed).  FLOPs: 4*B*Hq*Sq*Sk*D
    forward + 10*... backward, halved under the causal mask."""
    shapes = [
        ("sdxl_self_s1024_d64", 3, 10, 10, 1024, 1024, 64, False),
        ("sdxl_self_s256_d64", 3, 20, 20, 256, 256, 64, False),
        ("sdxl_cross_s1024_kv77", 3, 10, 10, 1024, 77, 64, False),
        ("llama_gqa_s2048_d128", 4, 32, 8, 2048, 2048, 128, True),
    ]
    for name, B, Hq, Hkv, Sq, Sk, D, causal in shapes:
        q, k, v = (torch.randn(B, h, s, D, device="cuda", dtype=torch.bfloat16,
                               requires_grad=True)
                   for h, s in ((Hq, Sq), (Hkv, Sk), (Hkv, Sk)))
        dout = torch.randn(B, Hq, Sq, D, device="cuda", dtype=torch.bfloat16)

        def step():
            q.grad = k.grad = v.grad = None
            F.attention(q, k, v, causal=causal).backward(dout)

        flops = 14.0 * B * Hq * Sq * Sk * D * (0.5 if causal else 1.0)
        saved = os.environ.pop("MODAL_AMD_ATTN_BWD", None)
        for path in ("hip", "ref"):
            if path == "ref":
                os.environ["MODAL_AMD_ATTN_BWD"] = "ref"
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            dt = timeit(step, iters=200 if Sq * Sk <= 1 << 20 else 50,
                        warmup=10)
            peak = torch.cuda.max_memory_allocated() - base
            tf = flops / dt / 1e12
            results[f"attn_fwd_bwd/{name}/{path}"] = {
                "ms": round(dt * 1e3, 3), "TF": round(tf, 1),
                "pct_peak": round(100 * tf / MFMA_CEIL_TF, 1),
                "peak_MB": round(peak / 2**20, 1)}
        os.environ.pop("MODAL_AMD_ATTN_BWD", None)
        if saved is not None:
            os.environ["MODAL_AMD_ATTN_BWD"] = saved
        q.grad = k.grad = v.grad = None


def bench_decode(results):
    for name, B, Hq, Hkv, S, D in [
        ("llama_b64_s1024", 64, 32, 8, 1024, 128),
        ("llama_b1_s4096", 1, 32, 8, 4096, 128),
        ("whisper_dec_b16_s448", 16, 20, 20, 448, 64),
    ]:
        q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16)
        kc = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
        vc = torch.randn(B, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
        lens = torch.full((B,), S, device="cuda", dtype=torch.int32)
        dt = timeit(lambda: F.paged_decode(q, kc, vc, None, lens))
        gb = 2 * B * Hkv * S * D * 2 / 1e9  # K+V bytes actually read
        results[f"decode/{name}"] = {
            "ms": round(dt * 1e3, 3), "GBps": round(gb / dt, 0),
            "pct_hbm": round(100 * gb / dt / HBM_CEIL_GBS, 1)}


def _alternate(fns, window_s=0.25, rounds=3):
    """Best per-call time of each fn, timed in alternating windows of about
    window_s (at least 3 calls) after a warm-up of every fn."""
    iters = []
    for fn in fns:
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        iters.append(max(3, int(window_s / (time.perf_counter() - t0))))
    best = [float("inf")] * len(fns)
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], timeit(fn, iters=iters[i], warmup=1))
    return best


def bench_paged_prefill(results):
    """A chunk of C new tokens over a cached prefix of P (Llama-3-8B heads,
    block 16, shuffled table): F.paged_prefill against the lane it replaces,
    F.paged_decode over C rows with the table repeated and lens = P+1..P+C.
    Both are timed in one process, alternating; FLOPs = 4*Hq*D*sum_i(P+i+1).
    The outputs are compared at every timed shape (each kernel is held to
    2e-2/2e-2 of the truth by the tests, so to twice that of each other).
    At P = 0 the dense causal F.attention at S = C is the upper yardstick."""
    Hq, Hkv, D, bs = 32, 8, 128, 16
    g = torch.Generator(device="cuda").manual_seed(0)

    def randn(*shape):
        return torch.randn(*shape, device="cuda", generator=g)

    for fp8 in (False, True):
        cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
        amp = 0.5 if fp8 else 1.0
        for C in (128, 512, 2048):
            for P in (0, 2048, 8192, 32768):
                S = P + C
                nblk = S // bs
                kc = (randn(nblk, Hkv, bs, D) * amp).to(cdt)
                vc = (randn(nblk, Hkv, bs, D) * amp).to(cdt)
                q = randn(C, Hq, D).to(torch.bfloat16)
                row = torch.randperm(nblk, device="cuda", generator=g).int()
                bt1 = row.unsqueeze(0)
                cu = torch.tensor([0, C], dtype=torch.int32, device="cuda")
                sl = torch.tensor([S], dtype=torch.int32, device="cuda")
                btc = row.unsqueeze(0).repeat(C, 1)
                lens = torch.arange(P + 1, S + 1, dtype=torch.int32,
                                    device="cuda")

                def new():
                    return F.paged_prefill(q, kc, vc, bt1, cu, sl, bs,
                                           max_q_len=C)

                def old():
                    return F.paged_decode(q, kc, vc, btc, lens, bs)

                a, b = new().float(), old().float()
                diff = (a - b).abs()
                agree = bool((diff <= 4e-2 + 4e-2 * b.abs()).all())
                fns = [new, old]
                if P == 0 and not fp8:
                    qd = q.transpose(0, 1).unsqueeze(0).contiguous()
                    kd = randn(1, Hkv, C, D).to(torch.bfloat16)
                    vd = randn(1, Hkv, C, D).to(torch.bfloat16)
                    fns.append(lambda: F.attention(qd, kd, vd, causal=True))
                ts = _alternate(fns)
                flops = 4.0 * Hq * D * (C * P + C * (C + 1) / 2)
                r = {"paged_ms": round(ts[0] * 1e3, 4),
                     "paged_TF": round(flops / ts[0] / 1e12, 1),
                     "decode_lane_ms": round(ts[1] * 1e3, 4),
                     "decode_lane_TF": round(flops / ts[1] / 1e12, 1),
                     "speedup": round(ts[1] / ts[0], 2),
                     "max_abs_diff": round(float(diff.max()), 5),
                     "outputs_agree": agree}
                if len(ts) == 3:
                    r["dense_causal_ms"] = round(ts[2] * 1e3, 4)
                    r["dense_causal_TF"] = round(flops / ts[2] / 1e12, 1)
                name = f"paged_prefill/{'fp8' if fp8 else 'bf16'}_c{C}_p{P}"
                results[name] = r
                print(name, json.dumps(r), flush=True)


def bench_memory_ops(results):
    x = torch.randn(16, 1280, 64, 64, device="cuda", dtype=torch.bfloat16)
    g = torch.randn(1280, device="cuda")
    b = torch.randn(1280, device="cuda")
    dt = timeit(lambda: F.groupnorm_silu(x, g, b, 32))
    gb = 2 * x.numel() * 2 / 1e9
    results["gn_silu/16x1280x64x64"] = {
        "ms": round(dt * 1e3, 3), "GBps": round(gb / dt, 0),
        "pct_hbm": round(100 * gb / dt / HBM_CEIL_GBS, 1)}

    x2 = torch.randn(65536, 4096, device="cuda", dtype=torch.bfloat16)
    g2 = torch.randn(4096, device="cuda")
    dt = timeit(lambda: F.rmsnorm(x2, g2))
    gb = 2 * x2.numel() * 2 / 1e9
    results["rmsnorm/64k_rows_4096"] = {
        "ms": round(dt * 1e3, 3), "GBps": round(gb / dt, 0),
        "pct_hbm": round(100 * gb / dt / HBM_CEIL_GBS, 1)}

    x3 = torch.randn(8192, 1280, device="cuda", dtype=torch.bfloat16)
    g3 = torch.randn(1280, device="cuda")
    b3 = torch.randn(1280, device="cuda")
    dt = timeit(lambda: F.layernorm(x3, g3, b3))
    gb = 2 * x3.numel() * 2 / 1e9
    results["layernorm/8192x1280"] = {
        "ms": round(dt * 1e3, 3), "GBps": round(gb / dt, 0),
        "pct_hbm": round(100 * gb / dt / HBM_CEIL_GBS, 1)}

    a = torch.randn(64 * 1024 * 1024, device="cuda", dtype=torch.bfloat16)
    bb = torch.randn_like(a)
    dt = timeit(lambda: F.silu_mul(a, bb))
    gb = 3 * a.numel() * 2 / 1e9
    results["silu_mul/64M"] = {
        "ms": round(dt * 1e3, 3), "GBps": round(gb / dt, 0),
        "pct_hbm": round(100 * gb / dt / HBM_CEIL_GBS, 1)}

    lo = torch.randn(64, 128256, device="cuda")
    dt = timeit(lambda: F.sample(lo, 1.0, seed=1))
    gb = lo.numel() * 4 / 1e9
    results["sample/64x128k"] = {
        "ms": round(dt * 1e3, 3), "GBps": round(gb / dt, 0),
        "pct_hbm": round(100 * gb / dt / HBM_CEIL_GBS, 1)}


def bench_sdxl_glue(results):
    """The fused glue ops of the SDXL step at their workload shapes, each
    timed in alternating windows beside the torch chain it replaced in the
    models.  GB counts the bytes the fused op has to move (inputs read once,
    outputs written once), for both columns, so chain_TBps is the chain's
    useful rate, not its traffic."""
    bf = dict(device="cuda", dtype=torch.bfloat16)

    def graphed(fn, reps=16):
        """Calls under 0.2 ms are bound by the host's launches when issued
        one by one; those are timed as `reps` calls replayed from one
        captured graph, which is also how the denoise step runs them."""
        fn()
        torch.cuda.synchronize()
        if timeit(fn, iters=5, warmup=1) >= 2e-4:
            return fn, 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        return g.replay, reps

    def record(name, fused, chain, gb):
        (fused, rf), (chain, rc) = graphed(fused), graphed(chain)
        tf, tc = _alternate([fused, chain])
        tf, tc = tf / rf, tc / rc
        r = {"fused_ms": round(tf * 1e3, 4), "chain_ms": round(tc * 1e3, 4),
             "speedup": round(tc / tf, 2),
             "fused_TBps": round(gb / tf / 1e3, 2),
             "chain_TBps": round(gb / tc / 1e3, 2),
             "fused_pct_hbm": round(100 * gb / tf / HBM_CEIL_GBS, 1)}
        results[name] = r
        print(name, json.dumps(r), flush=True)

    s = torch.randn(16, 2048, 16384, **bf)
    scale = 512 ** -0.5
    record("scaled_softmax/16x2048x16384",
           lambda: F.scaled_softmax(s, scale),
           lambda: torch.softmax((s * scale).float(), -1).to(torch.bfloat16),
           2 * s.numel() * 2 / 1e9)
    del s

    for N, C, H in ((16, 640, 64), (16, 1280, 32), (16, 512, 128)):
        x = torch.randn(N, C, H, H, **bf)
        g = torch.randn(C, device="cuda")
        b = torch.randn(C, device="cuda")
        # statistics pass reads x, apply pass reads x and writes y.  The
        # chain's reshape is a view; the transposing copy ran inside the
        # Linear that followed, hence .contiguous() here
        record(f"gn_nhwc/{N}x{C}x{H}x{H}",
               lambda: F.groupnorm_silu(x, g, b, 32, do_silu=False,
                                        out_nhwc=True),
               lambda: F.groupnorm_silu(x, g, b, 32, do_silu=False)
               .permute(0, 2, 3, 1).reshape(N, H * H, C).contiguous(),
               3 * x.numel() * 2 / 1e9)
        h = torch.randn(N, H * H, C, **bf)
        record(f"add_nhwc_to_nchw/{N}x{C}x{H}x{H}",
               lambda: F.add_nhwc_to_nchw(x, h),
               lambda: x + h.reshape(N, H, H, C).permute(0, 3, 1, 2),
               3 * x.numel() * 2 / 1e9)

    N, C, K, H = 16, 320, 320, 128
    x = torch.randn(N, C, H, H, **bf)
    w = torch.randn(K, C, 3, 3, **bf) / (3 * C ** 0.5)
    wr = F.repack_conv3x3_weight(w)
    bias = torch.randn(K, device="cuda")
    t = torch.randn(N, K, **bf)
    tf, tc, tp = _alternate([
        lambda: F.conv3x3(x, wr, bias, K, raw_weight=w, addend=t),
        lambda: F.conv3x3(x, wr, bias, K, raw_weight=w) + t[:, :, None, None],
        lambda: F.conv3x3(x, wr, bias, K, raw_weight=w)])
    flops = 2.0 * N * K * C * 9 * H * H
    r = {"fused_ms": round(tf * 1e3, 4), "chain_ms": round(tc * 1e3, 4),
         "conv_alone_ms": round(tp * 1e3, 4), "speedup": round(tc / tf, 2),
         "fused_TF": round(flops / tf / 1e12, 1),
         "conv_alone_TF": round(flops / tp / 1e12, 1)}
    results[f"conv3x3_addend/{N}x{C}to{K}at{H}"] = r
    print(f"conv3x3_addend/{N}x{C}to{K}at{H}", json.dumps(r), flush=True)
    del x, w, wr

    for rows, D in ((65536, 640), (16384, 1280)):
        a = torch.randn(rows, D, **bf)
        c = torch.randn(rows, D, **bf)
        g = torch.randn(D, device="cuda")
        b = torch.randn(D, device="cuda")

        def chain():
            y = a + c
            return y, F.layernorm(y, g, b)

        record(f"add_layernorm/{rows}x{D}",
               lambda: F.add_layernorm(a, c, g, b), chain,
               4 * a.numel() * 2 / 1e9)


def bench_gemm_reference(results):
    """hipBLASLt via torch for context."""
    for n in (4096, 8192):
        a = torch.randn(n, n, device="cuda", dtype=torch.bfloat16)
        b = torch.randn(n, n, device="cuda", dtype=torch.bfloat16)
        dt = timeit(lambda: a @ b)
        tf = 2 * n**3 / dt / 1e12
        results[f"hipblaslt_gemm/{n}"] = {"ms": round(dt * 1e3, 3),
                                          "TF": round(tf, 1),
                                          "pct_peak": round(100 * tf / MFMA_CEIL_TF, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="",
                    help="comma-separated groups: attention, attention_bwd, "
                         "decode, paged_prefill, memory_ops, sdxl_glue, "
                         "gemm_reference (default: all)")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    groups = {"attention": bench_attention,
              "attention_bwd": bench_attention_bwd,
              "decode": bench_decode, "paged_prefill": bench_paged_prefill,
              "memory_ops": bench_memory_ops,
              "sdxl_glue": bench_sdxl_glue,
              "gemm_reference": bench_gemm_reference}
    only = [g for g in args.only.split(",") if g] or list(groups)
    results = {}
    for g in only:
        groups[g](results)
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
