"""SDXL-class model stack: shape/dtype correctness on CPU (reference op paths),
plus the scheduler math.  GPU end-to-end lives in test_sdxl_gpu.py."""
import pytest
import torch

from modal_examples_amd.models.sdxl.pipeline import SDXLPipeline, euler_sigmas
from modal_examples_amd.models.sdxl.text import encode_prompts
from modal_examples_amd.models.sdxl.unet import UNetConfig, UNetXL


def test_unet_small_forward():
    torch.manual_seed(0)
    cfg = UNetConfig.small()
    net = UNetXL(cfg).to(torch.bfloat16)
    x = torch.randn(2, 4, 32, 32, dtype=torch.bfloat16)
    t = torch.tensor([999.0, 500.0])
    ctx = torch.randn(2, 77, cfg.ctx_dim, dtype=torch.bfloat16)
    add = torch.randn(2, cfg.addition_dim, dtype=torch.bfloat16)
    out = net(x, t, ctx, add)
    assert out.shape == x.shape
    assert out.dtype == torch.bfloat16
    assert torch.isfinite(out.float()).all()


def test_unet_sdxl_param_count():
    """Full-size config must be in the SDXL-base class (~2.6B)."""
    cfg = UNetConfig.sdxl()
    net = UNetXL(cfg)
    n = sum(p.numel() for p in net.parameters())
    assert 2.0e9 < n < 3.3e9, f"param count {n/1e9:.2f}B out of SDXL range"
    del net


def test_sigma_schedule():
    sig, ts = euler_sigmas(4)
    assert len(sig) == 5 and sig[-1] == 0
    assert (sig[:-1] > 0).all()
    assert (sig.diff()[:-1] < 0).all()  # strictly decreasing
    assert ts[0] == 999


def test_encode_prompts_deterministic():
    a1, p1 = encode_prompts(["a cat"], 256, 128)
    a2, p2 = encode_prompts(["a cat"], 256, 128)
    b, _ = encode_prompts(["a dog"], 256, 128)
    assert torch.equal(a1, a2) and torch.equal(p1, p2)
    assert not torch.equal(a1, b)
    assert a1.shape == (1, 77, 256)


@pytest.mark.slow
def test_pipeline_small_cpu_end_to_end():
    pipe = SDXLPipeline(UNetConfig.small(), device="cpu", latent_size=16,
                        use_graph=False)
    imgs = pipe.generate(["test prompt"], steps=2)
    assert imgs.shape == (1, 128, 128, 3)
    assert imgs.dtype == torch.uint8
    # determinism with same seed
    imgs2 = pipe.generate(["test prompt"], steps=2)
    assert torch.equal(imgs, imgs2)


def test_conv3x3_module_cpu_fallback_matches_conv2d():
    """Conv3x3 module on CPU == nn.Conv2d with the same params (the kernel
    path is GPU-only; CPU uses F.conv2d)."""
    import torch

    from modal_examples_amd.models.sdxl.layers import Conv1x1, Conv3x3

    torch.manual_seed(0)
    m = Conv3x3(8, 16).eval()
    x = torch.randn(2, 8, 12, 12)
    want = torch.nn.functional.conv2d(x, m.weight, m.bias, padding=1)
    assert torch.allclose(m(x), want, atol=1e-6)
    r = torch.randn(2, 16, 12, 12)
    assert torch.allclose(m(x, residual=r), want + r, atol=1e-6)
    s = Conv1x1(8, 16).eval()
    assert torch.allclose(
        s(x), torch.nn.functional.conv2d(x, s.weight, s.bias), atol=1e-6)


def test_conv3x3_packed_follows_bias_and_weight_updates():
    """The cached (repacked weight, f32 bias) pair is refreshed by an
    in-place update of the bias alone, as it is by one of the weight."""
    from modal_examples_amd.models.sdxl.layers import Conv3x3
    from modal_examples_amd.ops import functional as OF

    torch.manual_seed(0)
    # bf16 is the case that matters: there the f32 bias of the pack is a
    # copy, while for an f32 module it aliases the parameter's storage
    for dtype in (torch.bfloat16, torch.float32):
        m = Conv3x3(8, 16).to(dtype).eval()
        wr0, b0 = m._packed()
        assert b0.dtype is torch.float32
        assert torch.equal(b0, m.bias.detach().float())
        assert m._packed()[0] is wr0, "an unchanged module must reuse its pack"
        old = m.bias.detach().clone()
        with torch.no_grad():
            m.bias.add_(1)
        assert not torch.equal(m.bias.detach(), old)
        assert torch.equal(m._packed()[1], (old + 1).float())
        assert torch.equal(m._packed()[1], m.bias.detach().float())
        with torch.no_grad():
            m.weight.mul_(2)
        wr2, b2 = m._packed()
        assert torch.equal(wr2, OF.repack_conv3x3_weight(m.weight.detach()))
        assert not torch.equal(wr2, wr0)
        assert torch.equal(b2, m.bias.detach().float())
        # a replaced bias parameter is a new identity at version 0
        m.bias = torch.nn.Parameter(torch.full((16,), 3.0, dtype=dtype))
        assert torch.equal(m._packed()[1], torch.full((16,), 3.0))
    nb = Conv3x3(8, 16).eval()
    nb.bias = None
    assert torch.equal(nb._packed()[1], torch.zeros(16))
    assert nb._packed()[0] is nb._packed()[0]


def test_repack_conv3x3_weight_layout():
    import torch

    from modal_examples_amd.ops import functional as OF

    w = torch.arange(5 * 7 * 9, dtype=torch.float32).reshape(5, 7, 3, 3)
    wr = OF.repack_conv3x3_weight(w)
    assert wr.shape == (9, 64, 16)
    # wr[tap, k, c] == w[k, c, tap//3, tap%3]
    for tap in (0, 4, 8):
        assert torch.equal(wr[tap, :5, :7],
                           w[:, :, tap // 3, tap % 3].to(torch.bfloat16))
    assert (wr[:, 5:, :] == 0).all() and (wr[:, :, 7:] == 0).all()
