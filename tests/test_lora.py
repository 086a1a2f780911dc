"""Multi-LoRA serving on the CPU: the reference op against LoRALinear, rows
without an adapter, and the engine's adapter lane on LlamaConfig.small()."""
import types

import pytest
import torch

from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.models.llama.lora import projection_shapes
from modal_examples_amd.models.llama.model import LlamaConfig
from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from modal_examples_amd.train.lora import LoRALinear

CFG = LlamaConfig.small()
PROMPT = [1 + (7 * i) % 900 for i in range(40)]  # two full KV blocks and a bit


def adapter_state(cfg, seed, r, targets=("qkv", "o_proj", "gate_up", "down")):
    """A random adapter under the names train.lora.lora_state_dict gives,
    large enough to move the greedy tokens of a randomly initialised model."""
    g = torch.Generator().manual_seed(seed)
    state = {}
    for li in range(cfg.n_layers):
        for t in targets:
            i, o = projection_shapes(cfg)[t]
            state[f"blocks.{li}.{t}.lora_a"] = torch.randn(r, i, generator=g) * 0.1
            state[f"blocks.{li}.{t}.lora_b"] = torch.randn(o, r, generator=g) * 0.1
    return state


def make_engine(**kw):
    torch.manual_seed(0)
    kw.setdefault("lora_slots", 2)
    return LlamaEngine(CFG, device="cpu", dtype=torch.float32, max_batch=4,
                       kv_blocks=128, use_graph=False, **kw)


def serve(eng, jobs):
    """jobs: (prompt, adapter) pairs in one batch -> out_tokens per job."""
    rids = [eng.add_request(p, max_new_tokens=6, adapter=a) for p, a in jobs]
    while eng.has_work:
        eng.step()
    return [eng.finished[r].out_tokens for r in rids]


def test_reference_matches_lora_linear():
    torch.manual_seed(1)
    base = torch.nn.Linear(64, 128, bias=False)
    lin = LoRALinear(base, rank=16, alpha=32.0)
    lin.lora_b.data.normal_()
    x = torch.randn(5, 64)
    bank_a = torch.zeros(3, 16, 64)
    bank_b = torch.zeros(3, 128, 16)
    bank_a[2], bank_b[2] = lin.lora_a.data, lin.lora_b.data * lin.scale
    idx = torch.full((5,), 2, dtype=torch.int32)
    got = ref.lora_apply_ref(base(x).detach(), x, bank_a, bank_b, idx)
    torch.testing.assert_close(got, lin(x).detach(), atol=1e-5, rtol=1e-5)


def test_rows_without_adapter_are_untouched():
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(6, 64, generator=g), torch.randn(6, 128, generator=g)
    bank_a = torch.randn(2, 16, 64, generator=g)
    bank_b = torch.randn(2, 128, 16, generator=g)
    idx = torch.tensor([-1, 0, 5, 1, -7, 0], dtype=torch.int32)
    y0 = y.clone()
    OF.lora_apply_(y, x, bank_a, bank_b, OF.lora_schedule(idx, 2))
    off = torch.tensor([True, False, True, False, True, False])
    assert torch.equal(y[off], y0[off])
    assert not torch.equal(y[1], y0[1]) and not torch.equal(y[3], y0[3])
    want, tol = ref.lora_bound_ref(y0, x, bank_a, bank_b, idx)
    assert torch.equal(tol[off], torch.zeros_like(tol[off]))
    assert ((y.double() - want).abs() <= tol + 1e-5).all()


def test_engine_mixed_batch_matches_solo():
    eng = make_engine()
    assert eng.load_adapter("a", adapter_state(CFG, 10, r=8), alpha=16.0) == 0
    assert eng.load_adapter("b", adapter_state(CFG, 11, r=16,
                                               targets=("qkv", "down"))) == 1
    keys = set(eng.model.state_dict())
    [solo_a] = serve(eng, [(PROMPT, "a")])
    [solo_base] = serve(eng, [(PROMPT, None)])
    mixed = serve(eng, [(PROMPT, None), (PROMPT, "a"), (PROMPT[:9], "b"),
                        (PROMPT[:23], "a")])
    assert mixed[1] == solo_a and mixed[0] == solo_base
    assert solo_a != solo_base
    [plain] = serve(make_engine(lora_slots=0), [(PROMPT, None)])
    assert plain == solo_base
    assert set(eng.model.state_dict()) == keys  # banks stay off the module


@pytest.mark.parametrize("lane", [{"chunked_prefill": 16}, {"spec_tokens": 2}])
def test_engine_lanes_carry_the_adapter(lane):
    want = make_engine()
    want.load_adapter("a", adapter_state(CFG, 10, r=8))
    eng = make_engine(**lane)
    eng.load_adapter("a", adapter_state(CFG, 10, r=8))
    jobs = [(PROMPT, "a"), (PROMPT, None)]
    assert serve(eng, jobs) == serve(want, jobs)


def test_prefix_cache_is_per_adapter():
    eng = make_engine(prefix_cache=True)
    eng.load_adapter("a", adapter_state(CFG, 10, r=8))
    [base] = serve(eng, [(PROMPT, None)])
    assert eng.prefix_hit_tokens == 0
    [first] = serve(eng, [(PROMPT, "a")])      # base blocks are not shared
    assert eng.prefix_hit_tokens == 0
    [again] = serve(eng, [(PROMPT, "a")])      # its own are
    assert eng.prefix_hit_tokens == 32 and again == first != base
    eng.unload_adapter("a")
    eng.load_adapter("a", adapter_state(CFG, 12, r=8))  # same name, new load
    serve(eng, [(PROMPT, "a")])
    assert eng.prefix_hit_tokens == 32
    serve(eng, [(PROMPT, None)])               # the base still hits its own
    assert eng.prefix_hit_tokens == 64


def test_engine_errors():
    with pytest.raises(ValueError, match="tensor parallelism"):
        make_engine(tp=types.SimpleNamespace(world=2, rank=0))
    with pytest.raises(ValueError, match="MoE"):
        LlamaEngine(LlamaConfig.moe_small(), device="cpu", kv_blocks=32,
                    dtype=torch.float32, lora_slots=2,
                    lora_targets=("qkv", "gate_up"))
    eng = make_engine()
    with pytest.raises(ValueError, match="unknown adapter"):
        eng.add_request(PROMPT, adapter="nope")
    eng.load_adapter("a", adapter_state(CFG, 10, r=8))
    eng.add_request(PROMPT, max_new_tokens=2, adapter="a")
    with pytest.raises(ValueError, match="in use"):
        eng.unload_adapter("a")
    eng.run_until_done()
    eng.unload_adapter("a")
    with pytest.raises(ValueError, match="rank"):
        eng.load_adapter("big", adapter_state(CFG, 10, r=32))


def test_server_selects_adapter_by_model_name():
    import asyncio

    import httpx

    from modal_examples_amd.models.llama.server import (LLMServer,
                                                        create_openai_app)

    eng = make_engine()
    eng.load_adapter("tenant-a", adapter_state(CFG, 10, r=8))
    srv = LLMServer(eng, "base")

    async def go():
        transport = httpx.ASGITransport(app=create_openai_app(srv))
        async with httpx.AsyncClient(transport=transport,
                                     base_url="http://t") as c:
            ids = [m["id"] for m in (await c.get("/v1/models")).json()["data"]]
            assert ids == ["base", "tenant-a"]
            texts = []
            for model in ("base", "tenant-a", "nope"):
                r = await c.post("/v1/completions", json={
                    "model": model, "prompt": "abc def ghi", "max_tokens": 6})
                texts.append((r.status_code, r.json()))
            assert [t[0] for t in texts] == [200, 200, 404]
            assert texts[2][1]["error"]["code"] == "model_not_found"
            assert (texts[0][1]["choices"][0]["text"]
                    != texts[1][1]["choices"][0]["text"])

    try:
        asyncio.run(go())
    finally:
        srv.shutdown()
