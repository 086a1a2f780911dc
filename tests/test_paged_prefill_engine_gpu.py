"""The engine's prefill_attn="paged" lane on the MI355X: chunked prefill and
the suffix after a prefix-cache hit run through the MFMA paged prefill
kernel and emit the tokens of the monolithic / cold run.  Same engine
shape, prompts and seeds as test_chunked_prefill_matches_on_gpu and
test_prefix_cache_matches_on_gpu in test_llama_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def _engine(**kw):
    from modal_examples_amd.models.llama.engine import LlamaEngine
    from modal_examples_amd.models.llama.model import LlamaConfig

    torch.manual_seed(0)
    return LlamaEngine(LlamaConfig.small(), device="cuda",
                       dtype=torch.bfloat16, use_graph=False, kv_blocks=256,
                       eos_id=-1, **kw)


def _generate(eng, prompts):
    outs = []
    for p in prompts:
        rid = eng.add_request(p, max_new_tokens=6, temperature=0.0)
        while eng.has_work:
            eng.step()
        outs.append(eng.finished[rid].out_tokens)
    return outs


def _prompt(seed, n):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, (n,), generator=g).tolist()


@requires_gpu
@pytest.mark.parametrize("chunk,length", [(8, 37), (40, 100)])
def test_chunked_prefill_paged_lane_matches_monolithic(chunk, length):
    prompt = _prompt(2, length)
    mono = _generate(_engine(), [prompt])
    paged = _generate(_engine(chunked_prefill=chunk, prefill_attn="paged"),
                      [prompt])
    assert paged == mono


@requires_gpu
def test_prefix_cache_paged_lane_matches_cold():
    from modal_examples_amd.models.llama.engine import BLOCK

    g = torch.Generator().manual_seed(6)
    system = torch.randint(0, 1024, (3 * BLOCK,), generator=g).tolist()
    prompts = [system + [7, 8, 9], system + [11, 12]]
    cold = _generate(_engine(), prompts)
    eng = _engine(prefix_cache=True, prefill_attn="paged")
    assert _generate(eng, prompts) == cold
    assert eng.prefix_hit_tokens == 3 * BLOCK


@requires_gpu
def test_fp8_kv_paged_lane_matches_decode_lane():
    prompt = _prompt(2, 37)
    kw = dict(kv_dtype="fp8", chunked_prefill=8)
    assert (_generate(_engine(prefill_attn="paged", **kw), [prompt])
            == _generate(_engine(**kw), [prompt]))
