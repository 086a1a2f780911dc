"""ops.linear_fp8(tiled=True) off the GPU: the arithmetic contract is the
rows kernel's, so the reference composition is the same one."""
import torch

from modal_examples_amd.models.llama.model import Fp8Linear
from modal_examples_amd.ops import functional as OF
from test_linear_fp8 import random_case


def test_tiled_on_the_cpu_is_the_reference_composition(monkeypatch):
    c = random_case(5, 64, 256, seed=4)
    q, s = c["qweight"], c["wscale"]
    for x in (c["x"], c["x"].float()):
        assert torch.equal(OF.linear_fp8(x, q, s, tiled=True),
                           OF.linear_fp8(x, q, s, tiled=False))
    assert torch.equal(
        OF.linear_fp8_q(c["xq"], c["xscale"], q, s, tiled=True),
        OF.linear_fp8_q(c["xq"], c["xscale"], q, s))
    # off the GPU the prefill lane of the module stays the dequantize lane
    fl = Fp8Linear(256, 64)
    fl.qweight, fl.wscale = q, s
    x = torch.randn(Fp8Linear.M_KERNEL + 1, 256,
                    generator=torch.Generator().manual_seed(1))
    want = torch.nn.functional.linear(x, OF.dequantize_fp8(q, s))
    for lane in ("tiled", "dequant"):
        monkeypatch.setattr(Fp8Linear, "PREFILL_LANE", lane)
        assert torch.equal(fl(x), want)
