"""Compile-time kernel resource audit (no GPU needed): hipcc cross-compiles
each gfx950 kernel with -Rpass-analysis=kernel-resource-usage and this script
enforces the budgets that kept round-1 performance:

- ZERO scratch and ZERO spills everywhere (guide rule #20: a runtime-indexed
  register array silently spills and costs 3x — measured on the decode
  kernel, 3.5 -> 1.0 TB/s),
- occupancy floors for the hot kernels (occupancy drops are how attention
  regressions sneak in: the forward runs 3 waves/SIMD at D=64, 2 at D=128).

Usage: python scripts/check_kernel_resources.py [file.hip ...]
"""
import re
import subprocess
import sys
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "modal_examples_amd" / "ops" / "csrc"

# kernel-name substring -> minimum waves/SIMD (from the shipped builds)
OCCUPANCY_FLOORS = {
    "fa32_kernelILi64ELb1": 3,   # D=64 causal
    "fa32_kernelILi64ELb0": 3,   # D=64
    "fa32_kernelILi128ELb1": 2,  # D=128 causal (llama prefill)
    "fa32_kernelILi128ELb0": 2,  # D=128
    "fa_bwd_dq_kernelILi64E": 3,     # backward dQ, D=64
    "fa_bwd_dq_kernelILi128E": 2,    # backward dQ, D=128
    "fa_bwd_dkdv_kernelILi64E": 2,   # backward dK/dV, D=64
    "fa_bwd_dkdv_kernelILi128E": 1,  # dK^T+dV^T accumulators take 128 AGPRs
    "fa_bwd_delta_kernel": 8,
    "paged_prefill_kernelILi64E": 3,   # bf16 and fp8 cache, the forward's 3
    "paged_prefill_kernelILi128E": 2,  # bf16 and fp8 cache, the forward's 2
    "decode_kernel": 2,
    # conv3x3_kernel<UP, GN, RPW=2>: 64 accumulators + a chunk of staged
    # loads in flight must stay within 168 registers
    "conv3x3_kernelILb0ELb0ELi2E": 3,
    "conv3x3_kernelILb1ELb0ELi2E": 3,
    "conv3x3_kernelILb0ELb1ELi2E": 3,
    "conv3x3_kernelILb1ELb1ELi2E": 3,
    "decode_merge_kernel": 4,
    # moe_gemm_kernel<UP, NF>: two register sets of NF-step chunks in flight
    # beside 32 accumulators; one wave per SIMD already covers the decode
    # case (a wave per 32x64 output tile), the floors guard the rest
    "moe_gemm_kernelILb1ELi8E": 1,   # up GEMM, 128-deep chunks
    "moe_gemm_kernelILb1ELi4E": 2,   # up GEMM, 64-deep chunks
    "moe_gemm_kernelILb0ELi8E": 2,   # down GEMM, 128-deep chunks
    "moe_gemm_kernelILb0ELi4E": 2,   # down GEMM, 64-deep chunks
    "moe_route_kernel": 8,
    "moe_align_kernel": 8,
    "moe_combine_kernel": 8,
    # w4_gemm_kernel: two register sets of a 128-deep chunk (x fragments,
    # packed words, scales) beside 32 accumulators and the group's 48 partial
    # sums; built for two waves per SIMD (242 VGPRs), the second wave hides
    # a chunk's load latency
    "w4_gemm_kernel": 2,
    "w4_reduce_kernel": 8,
}


def audit(path: Path) -> dict:
    r = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-O3", "-c", str(path),
         "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"{path.name}: compile failed\n{r.stderr[-2000:]}")
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]+\])?: (\S+)", line)
        if m and cur:
            kernels[cur][m.group(1).strip()] = m.group(2)
    return kernels


def main(files):
    failures = []
    for f in files:
        for name, k in audit(f).items():
            scratch = int(k.get("ScratchSize", "0"))
            vspill = int(k.get("VGPRs Spill", "0"))
            sspill = int(k.get("SGPRs Spill", "0"))
            occ = int(k.get("Occupancy", "0"))
            line = (f"{f.name:24s} {name[:52]:52s} VGPR={k.get('VGPRs', '?'):>4s}"
                    f" AGPR={k.get('AGPRs', '?'):>4s} occ={occ} scratch={scratch}")
            print(line)
            if scratch or vspill or sspill:
                failures.append(f"{name}: scratch={scratch} spills={vspill}/{sspill}")
            for frag, floor in OCCUPANCY_FLOORS.items():
                if frag in name and occ < floor:
                    failures.append(f"{name}: occupancy {occ} < floor {floor}")
    if failures:
        print("\nBUDGET VIOLATIONS:")
        for x in failures:
            print(" -", x)
        return 1
    print("\nall kernels within budget (no scratch, no spills, occupancy floors hold)")
    return 0


if __name__ == "__main__":
    files = [Path(a) for a in sys.argv[1:]] or sorted(CSRC.glob("*.hip"))
    raise SystemExit(main(files))
