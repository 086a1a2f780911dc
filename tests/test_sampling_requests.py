"""Per-request top_k / top_p / min_p / seed in the Llama engine and server.

The engine's guarantee: token n of a seeded request is
`F.sample_batch(its logits row, its parameters, seed, counter = n)` — whatever
slot the request sits in, whoever shares the batch, however many steps the
engine has run, chunked prefill or speculative decode, graph or eager.  The
plumbing tests record every call of the batched sampler and recompute each
emitted token from the recorded row alone, so they do not depend on GEMM
rounding across batch shapes.

CPU tests on `LlamaConfig.small()`, plus GPU-marked twins of the plumbing and
same-seed tests.
"""
import asyncio

import pytest
import torch

import modal_examples_amd.ops.functional as F
from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.models.llama.model import LlamaConfig
from modal_examples_amd.models.llama.server import LLMServer, create_openai_app

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def gpu_test(fn):
    return pytest.mark.gpu(requires_gpu(fn))


PROMPT = [1, 17, 99, 250, 31, 7, 88, 412, 5, 64, 300]
FIELDS = dict(temperature=.8, top_k=40, top_p=.9, min_p=.02)
SEED = 2 ** 40 + 12345


def make_engine(device="cpu", **kw):
    torch.manual_seed(0)
    kw.setdefault("kv_blocks", 128)
    kw.setdefault("use_graph", False)
    dtype = torch.float32 if device == "cpu" else torch.bfloat16
    return LlamaEngine(LlamaConfig.small(), device=device, dtype=dtype, **kw)


def drain(eng, max_steps=400):
    # has_work also sees prompts that are mid chunked prefill
    steps = 0
    while eng.has_work and steps < max_steps:
        eng.step()
        steps += 1
    assert not eng.has_work


def record_batched(eng):
    """Wrap the batched sampler: one (logits row, parameters, token) entry
    per sampled row."""
    calls, inner = [], eng._sample_rows_batched

    def wrapped(logits, temps, top_k, top_p, min_p, seeds, counters):
        out = inner(logits, temps, top_k, top_p, min_p, seeds, counters)
        cols = [t.cpu() for t in (temps, top_k, top_p, min_p, seeds, counters, out)]
        lg = logits.detach().float().cpu()
        assert all(c.shape == (lg.shape[0],) for c in cols)
        for i in range(lg.shape[0]):
            calls.append((lg[i].clone(), *(c[i].item() for c in cols)))
        return out

    eng._sample_rows_batched = wrapped
    return calls


def check_seeded_request(eng, calls, req, device):
    """Every token of `req` is sample_batch of its own recorded row."""
    mine = [c for c in calls if c[5] == SEED]
    # rows that were sampled but not emitted exist only under speculation
    by_counter = {}
    for row, T, k, p, q, seed, ctr, tok in mine:
        assert T == pytest.approx(FIELDS["temperature"])
        assert k == FIELDS["top_k"]
        assert p == pytest.approx(FIELDS["top_p"]) and q == pytest.approx(FIELDS["min_p"])
        want = F.sample_batch(row[None].to(device), T, top_k=k, top_p=p, min_p=q,
                              seeds=seed, counters=ctr).cpu().item()
        assert tok == want, (ctr, tok, want)
        by_counter.setdefault(ctr, tok)
    assert len(req.out_tokens) >= 1
    assert sorted(by_counter) == list(range(len(req.out_tokens))), sorted(by_counter)
    assert [by_counter[n] for n in range(len(req.out_tokens))] == req.out_tokens


def run_scenario(scenario, device="cpu", **kw):
    eng = make_engine(device, **kw)
    calls = record_batched(eng)
    if scenario == "late":
        for i in range(3):
            eng.add_request([1, 40 + i, 9, 300 + i], max_new_tokens=12, temperature=1.0)
        eng.step()
        eng.step()
    rid = eng.add_request(PROMPT, max_new_tokens=10, seed=SEED, **FIELDS)
    drain(eng)
    req = eng.finished[rid]
    assert req.error is None
    check_seeded_request(eng, calls, req, device)
    if scenario == "late":
        # the unset rows took the engine-wide values: top_p, counter = row
        others = [c for c in calls if c[5] != SEED]
        assert others and all(c[2] == 0 and c[3] == 1.0 and c[4] == 0.0 for c in others)
    eng.close()
    return req.out_tokens


# ---- a. parameter plumbing

@pytest.mark.parametrize("scenario,kw", [
    ("alone", {}), ("late", {}), ("chunked", dict(chunked_prefill=4)),
    ("spec", dict(spec_tokens=3)), ("late", dict(chunked_prefill=4))])
def test_seeded_request_draws_from_its_own_stream(scenario, kw):
    run_scenario(scenario, **kw)


@gpu_test
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("scenario", ["alone", "late"])
def test_seeded_request_draws_from_its_own_stream_gpu(scenario, use_graph):
    run_scenario(scenario, device="cuda", use_graph=use_graph, kv_blocks=256)


def test_seeded_request_survives_preemption():
    """Preempted and recomputed: the counter restarts at the tokens kept."""
    eng = make_engine()
    calls = record_batched(eng)
    rid = eng.add_request(PROMPT, max_new_tokens=10, seed=SEED, **FIELDS)
    for _ in range(4):
        eng.step()
    req = eng.running[0]
    assert 1 < len(req.out_tokens) < 10
    eng._release(req)  # what the scheduler does under KV pressure
    eng.running.remove(req)
    eng.waiting.insert(0, req)
    drain(eng)
    check_seeded_request(eng, calls, eng.finished[rid], "cpu")


# ---- b. same seed twice

def _same_seed_twice(device, **kw):
    outs = []
    for seed in (SEED, SEED, SEED + 1):
        eng = make_engine(device, **kw)
        rid = eng.add_request(PROMPT, max_new_tokens=10, seed=seed, **FIELDS)
        drain(eng)
        outs.append(eng.finished[rid].out_tokens)
        eng.close()
    assert outs[0] == outs[1] and len(outs[0]) >= 1
    assert outs[0] != outs[2]


def test_same_seed_same_tokens():
    _same_seed_twice("cpu")


@gpu_test
@pytest.mark.parametrize("use_graph", [False, True])
def test_same_seed_same_tokens_gpu(use_graph):
    _same_seed_twice("cuda", use_graph=use_graph, kv_blocks=256)


# ---- c. default requests keep the engine-wide sampler

def _default_run(patch_parent):
    eng = make_engine(top_p=.9, chunked_prefill=6)
    if patch_parent:
        # the parent's call sites, literally
        eng._sample_requests = lambda lg, temps, reqs: eng._sample_rows(lg, temps, eng.top_p)
        eng._sample_slots = None
    rids = [eng.add_request([1, 30 + i, 200, 5 + i], max_new_tokens=8,
                            temperature=(0.0, 1.0, 1.3)[i % 3]) for i in range(4)]
    rids.append(eng.add_request(PROMPT, max_new_tokens=8, temperature=1.0))
    drain(eng)
    return eng, [eng.finished[r].out_tokens for r in rids]


def test_default_requests_never_enter_the_batched_path():
    eng, outs = _default_run(False)
    assert eng.batched_sample_calls == 0
    _, parent = _default_run(True)
    assert outs == parent
    # ... and one request with a field routes the calls it takes part in
    rid = eng.add_request(PROMPT, max_new_tokens=3, temperature=1.0, min_p=.1)
    drain(eng)
    assert eng.batched_sample_calls == len(eng.finished[rid].out_tokens)


# ---- d. filter effectiveness

@pytest.mark.parametrize("fields", [dict(top_k=1), dict(min_p=1.0),
                                    dict(top_p=1e-6), dict(top_k=1, seed=3)])
def test_filters_that_leave_only_the_argmax(fields):
    outs = []
    for kw in (dict(temperature=0.0), dict(temperature=1.0, **fields)):
        eng = make_engine()
        rid = eng.add_request(PROMPT, max_new_tokens=8, **kw)
        drain(eng)
        outs.append(eng.finished[rid].out_tokens)
    assert outs[0] == outs[1]


# ---- e. validation

@pytest.mark.parametrize("bad", [
    dict(top_p=0.0), dict(top_p=-.1), dict(top_p=1.0001), dict(top_p=float("nan")),
    dict(top_k=-1), dict(top_k=2.5), dict(min_p=-.01), dict(min_p=1.5),
    dict(min_p=float("nan")), dict(seed="7")])
def test_add_request_rejects_out_of_range(bad):
    eng = make_engine()
    with pytest.raises(ValueError):
        eng.add_request(PROMPT, temperature=1.0, **bad)
    assert not eng.waiting
    for ok in (dict(top_p=1.0), dict(top_p=1e-6), dict(top_k=0), dict(min_p=0.0),
               dict(min_p=1.0), dict(seed=-5), dict(seed=2 ** 64 + 1)):
        eng.add_request(PROMPT, temperature=1.0, **ok)


# ---- f. server

def _with_client(fn):
    import httpx

    srv = LLMServer(make_engine(), "test-model")
    try:
        app = create_openai_app(srv)

        async def go():
            transport = httpx.ASGITransport(app=app)
            async with httpx.AsyncClient(transport=transport, base_url="http://t") as c:
                await fn(c, srv)

        asyncio.run(go())
    finally:
        srv.shutdown()


def test_openai_routes_honour_seed_and_filters():
    async def go(c, srv):
        async def text(route, **body):
            body.setdefault("max_tokens", 8)
            if route == "/v1/completions":
                body["prompt"] = "tell me a story"
                r = await c.post(route, json=body)
                return [ch["text"] for ch in r.json()["choices"]]
            body["messages"] = [{"role": "user", "content": "tell me a story"}]
            r = await c.post(route, json=body)
            return [ch["message"]["content"] for ch in r.json()["choices"]]

        for route in ("/v1/completions", "/v1/chat/completions"):
            a = await text(route, temperature=1.0, seed=11, top_p=.95)
            b = await text(route, temperature=1.0, seed=11, top_p=.95)
            other = await text(route, temperature=1.0, seed=12, top_p=.95)
            assert a == b and a != other, (route, a, b, other)
            greedy = await text(route, temperature=0.0)
            assert await text(route, temperature=1.0, top_k=1) == greedy
            assert await text(route, temperature=1.0, min_p=1.0) == greedy
        two = await text("/v1/completions", temperature=1.0, seed=11, n=2, top_k=50)
        again = await text("/v1/completions", temperature=1.0, seed=11, n=2, top_k=50)
        assert len(two) == 2 and two[0] != two[1] and two == again

    _with_client(go)
    # choice j of a seeded request draws under seed + j
    from modal_examples_amd.models.llama.server import sampling_fields

    body = {"seed": 11, "top_k": 50, "top_p": None}
    assert sampling_fields(body, 0) == {"seed": 11, "top_k": 50}
    assert sampling_fields(body, 1) == {"seed": 12, "top_k": 50}
    assert sampling_fields({"min_p": 0.1}, 1) == {"min_p": 0.1}


def test_server_reports_bad_sampling_values():
    srv = LLMServer(make_engine(), "test-model")
    try:
        with pytest.raises(ValueError):
            srv.generate("hi", max_tokens=2, temperature=1.0, top_p=1.5)
        with pytest.raises(ValueError):
            srv.submit("hi", max_tokens=2, temperature=1.0, top_k=-3)
        assert srv.generate("hi", max_tokens=2, temperature=1.0, top_k=5, seed=1)
    finally:
        srv.shutdown()
