#!/usr/bin/env python3
"""Conv memory-format experiment: NCHW vs channels_last for the SDXL/VAE
conv shapes, plus a TunableOp check for the Llama decode GEMM shapes."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import torch  # noqa: E402


def timeit(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def conv_exp():
    from modal_examples_amd.gpu import kernel_cache

    kernel_cache.restore()
    shapes = [  # (B, Cin, Cout, H, W) — VAE + UNet hot convs
        (4, 128, 128, 1024, 1024),
        (4, 256, 256, 512, 512),
        (4, 512, 512, 256, 256),
        (4, 512, 512, 128, 128),
        (4, 320, 320, 128, 128),
        (4, 640, 640, 64, 64),
        (4, 1280, 1280, 32, 32),
    ]
    print(f"{'shape':28s} {'nchw_ms':>8s} {'nhwc_ms':>8s} {'speedup':>8s}")
    for B, Ci, Co, H, W in shapes:
        x = torch.randn(B, Ci, H, W, device="cuda", dtype=torch.bfloat16)
        conv = torch.nn.Conv2d(Ci, Co, 3, padding=1).to("cuda", torch.bfloat16)
        t_nchw = timeit(lambda: conv(x))
        xc = x.to(memory_format=torch.channels_last)
        convc = conv.to(memory_format=torch.channels_last)
        t_nhwc = timeit(lambda: convc(xc))
        print(f"{B}x{Ci}->{Co}@{H}x{W:<12} {t_nchw:8.2f} {t_nhwc:8.2f} "
              f"{t_nchw / t_nhwc:7.2f}x")


def gemm_exp():
    print("\nskinny decode GEMMs (batch=64 tokens):")
    for n, k in [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336),
                 (128256, 4096)]:
        a = torch.randn(64, k, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(n, k, device="cuda", dtype=torch.bfloat16)
        dt = timeit(lambda: a @ w.T, iters=20)
        gb = (64 * k + n * k) * 2 / 1e9
        print(f"  64x{k} @ {k}x{n}: {dt:6.3f} ms  {gb/dt*1000:6.0f} GB/s")




def timeit_span(fn, span=0.25, warmup=3):
    """ms per call over enough iterations that the timed window lasts at
    least `span` seconds (a window of a few ms measures the clock ramp)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-6)
    return timeit(fn, iters=max(10, int(span / one) + 1), warmup=0)


def kernel_exp(miopen=True):
    """Hand conv3x3 kernel (K3) per hot shape: plain, with the fused residual
    add, and the fused-upsample variant; TF rate of the plain call and, with
    `miopen`, the MIOpen NCHW time beside it.  Every figure spans >= 0.2 s."""
    import math

    from modal_examples_amd.gpu import kernel_cache
    from modal_examples_amd.ops import functional as F

    kernel_cache.restore()
    shapes = [  # (B, Cin, Cout, H, W, upsample) - H, W of the OUTPUT
        (4, 128, 128, 1024, 1024, False),
        (4, 256, 256, 512, 512, False),
        (4, 512, 512, 256, 256, False),
        (4, 512, 512, 128, 128, False),
        (4, 512, 256, 512, 512, False),
        (4, 320, 320, 128, 128, False),
        (4, 640, 640, 64, 64, False),
        (4, 1280, 1280, 32, 32, False),
        (4, 4, 512, 128, 128, False),
        (4, 256, 256, 1024, 1024, True),   # VAE upsample convs: the source
        (4, 512, 512, 256, 256, True),     # is half the output size
    ]
    print(f"{'shape':30s} {'miopen':>8s} {'hand':>8s} {'hand+res':>9s} "
          f"{'speedup':>8s} {'TF':>6s}")
    tot_mi = tot_hand = tot_res = 0.0
    for B, Ci, Co, H, W, up in shapes:
        Hs, Ws = (H // 2, W // 2) if up else (H, W)
        x = torch.randn(B, Ci, Hs, Ws, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(Co, Ci, 3, 3, device="cuda",
                        dtype=torch.bfloat16) / math.sqrt(Ci * 9)
        b = torch.randn(Co, device="cuda", dtype=torch.float32)
        res = torch.randn(B, Co, H, W, device="cuda", dtype=torch.bfloat16)
        t_mi = float("nan")
        if miopen and not up:
            conv = torch.nn.Conv2d(Ci, Co, 3, padding=1).to("cuda",
                                                            torch.bfloat16)
            with torch.no_grad():
                conv.weight.copy_(w)
                conv.bias.copy_(b.to(torch.bfloat16))
                t_mi = timeit_span(lambda: conv(x))
            del conv
        wr = F.repack_conv3x3_weight(w)
        t_k = timeit_span(lambda: F.conv3x3(x, wr, b, Co, raw_weight=w,
                                            upsample=up))
        t_r = timeit_span(lambda: F.conv3x3(x, wr, b, Co, residual=res,
                                            raw_weight=w, upsample=up))
        flops = 2.0 * B * Ci * Co * 9 * H * W
        tf = flops / (t_k * 1e-3) / 1e12
        if not up:
            tot_mi += t_mi
        tot_hand += t_k
        tot_res += t_r
        name = f"{B}x{Ci}->{Co}@{H}x{W}" + (" up" if up else "")
        print(f"{name:30s} {t_mi:8.3f} {t_k:8.3f} {t_r:9.3f} "
              f"{t_mi / t_k:7.2f}x {tf:6.0f}", flush=True)
    print(f"{'TOTAL':30s} {tot_mi:8.3f} {tot_hand:8.3f} {tot_res:9.3f}")


if __name__ == "__main__":
    import sys as _sys

    if "--kernel" in _sys.argv:
        kernel_exp(miopen="--no-miopen" not in _sys.argv)
    else:
        conv_exp()
        gemm_exp()
