"""bench.py driver contract: the exact torchrun launch the driver uses must
produce ONE valid JSON line from rank 0 (gloo on CPU, RCCL on GPU boxes)."""
import json
import socket
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _parse_json_line(out: str) -> dict:
    lines = [ln for ln in out.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, f"expected exactly one JSON line, got:\n{out[-2000:]}"
    return json.loads(lines[0])


def _check_contract(d: dict, n: int):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, f"missing {key}"
    assert d["n_gpus"] == n
    assert d["dtype"] == "bf16"
    assert d["scaling"] == "weak"
    assert d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["parallelism"] == f"dp{n}"


def test_bench_single_process_contract():
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "1", "--warmup", "1",
         "--small", "--latent", "32", "--batch", "1"],
        capture_output=True, text=True, cwd=REPO, timeout=420)
    assert r.returncode == 0, r.stderr[-2000:]
    _check_contract(_parse_json_line(r.stdout), 1)


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's images as float32 .npy,
    identical from run to run; --steps sets the timed steps; --full is
    accepted and leaves the result line's contract intact.  Runs on the CPU
    backend, whose arithmetic is order-fixed, so equal inputs must give
    bit-equal images; GPU reductions may reorder from process to process."""
    import os

    import numpy as np

    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out = tmp_path / name
        r = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
             "--warmup", "1", "--small", "--latent", "16", "--batch", "2",
             "--dump-outputs", str(out), *extra],
            capture_output=True, text=True, cwd=REPO, timeout=420, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        d = _parse_json_line(r.stdout)
        _check_contract(d, 1)
        assert d["steps"] == 2
        files = sorted(p.name for p in out.iterdir())
        assert files == ["images.npy"], files
        dumps.append(np.load(out / "images.npy"))
    a, b = dumps
    assert a.dtype == np.float32 and a.shape == (2, 128, 128, 3)
    assert a.min() >= 0 and a.max() <= 255 and a.std() > 0
    assert np.array_equal(a, b)


def test_bench_dump_outputs_sample_is_capped():
    """An output over the cap is reduced to a fixed sample: same picks every
    time, float32, within the byte budget."""
    import importlib.util
    import tempfile

    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location("bench", REPO / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.DUMP_CAP_BYTES // 4 + 1000
    img = (torch.arange(n, dtype=torch.int64) % 251).to(torch.uint8)
    arrs = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            bench._dump_outputs(d, img, 0, 1)
            files = sorted(Path(d).iterdir())
            assert [f.name for f in files] == ["images_sample.npy"]
            assert files[0].stat().st_size <= 64 << 20
            arrs.append(np.load(files[0]))
    assert arrs[0].dtype == np.float32
    assert arrs[0].size == bench.DUMP_CAP_BYTES // 4
    assert np.array_equal(arrs[0], arrs[1])


import pytest


@pytest.mark.parametrize("n", [2, 4])
def test_bench_torchrun_contract(n):
    """The driver's N>1 launcher: torch.distributed.run, one rank per GPU."""
    import os

    import torch

    env = None
    if torch.cuda.is_available() and torch.cuda.device_count() < n:
        # fewer GPUs than ranks: the same launch on the CPU/gloo path
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    port = str(_free_port())
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
         "--master-port", port, "bench.py", "--gpus", str(n), "--steps", "1",
         "--warmup", "1", "--small", "--latent", "16", "--batch", "1"],
        capture_output=True, text=True, cwd=REPO, timeout=420, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _parse_json_line(r.stdout)
    _check_contract(d, n)
    assert d["config"]["global_batch"] == n  # whole-job aggregate, not per-rank
