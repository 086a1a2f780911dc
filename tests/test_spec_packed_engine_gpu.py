"""LlamaEngine(spec_attn="packed") on the MI355X against spec_attn="rows":
greedy output of the small config, token for token, with oracle drafts (every
verify step carries full runs of spec_tokens + 1 positions) and with ngram
drafts, for a bf16 and an fp8 KV cache.

The two lanes verify with different kernels, so a near-tie in the logits may
resolve differently (docs/ENGINE.md).  What was measured for this model and
these prompts, both cache types, 24 new tokens per prompt: the plain lane's
smallest top-two logit gap is 0 or one bf16 ulp of the logits (0.0078) at
every seed probed, 0..5 (the logits of a random-init small model are nearly
flat, median gap 0.02 to 0.07), so no seed has a margin comfortably above
bf16 attention noise at all 72 positions.  The lanes nevertheless emit the
same tokens as plain decode at seeds 0, 1, 2, 3, 5 and 6 of 0..7, both caches;
"packed" leaves "rows" at seed 4 (bf16 cache) and seed 7 (both), "rows" never
leaves plain decode.  The test pins seed 0 and compares every token.
"""
import pytest
import torch

from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.models.llama.model import LlamaConfig
from test_kernel_edges_gpu import gpu_test

N_NEW = 24
PROMPTS = ([9, 8, 7, 6, 5], [3, 4, 5, 3, 4, 5, 3, 4], list(range(40, 75)))


def _mk(kv_dtype, spec_tokens, **kw):
    return LlamaEngine(LlamaConfig.small(), device="cuda",
                       dtype=torch.bfloat16, max_batch=4, kv_blocks=64,
                       use_graph=False, eos_id=-1, seed=0, kv_dtype=kv_dtype,
                       spec_tokens=spec_tokens, **kw)


def _greedy(eng, oracle=None):
    if oracle is not None:
        by_prompt = {tuple(p): o for p, o in zip(PROMPTS, oracle)}
        eng._propose = lambda r: by_prompt[tuple(r.prompt)][
            len(r.out_tokens): len(r.out_tokens) + eng.spec_tokens]
    for p in PROMPTS:
        eng.add_request(p, max_new_tokens=N_NEW, temperature=0.0)
    steps = 0
    while eng.has_work:
        eng.step()
        steps += 1
    outs = [eng.finished[i].out_tokens for i in sorted(eng.finished)]
    eng.close()
    return outs, steps


@gpu_test
@pytest.mark.parametrize("kv_dtype", ("bf16", "fp8"))
def test_packed_lane_emits_the_rows_lanes_tokens(kv_dtype):
    want, plain_steps = _greedy(_mk(kv_dtype, 0))
    for drafts in ("oracle", "ngram"):
        oracle = want if drafts == "oracle" else None
        rows, rows_steps = _greedy(_mk(kv_dtype, 4, spec_attn="rows"), oracle)
        packed, steps = _greedy(_mk(kv_dtype, 4, spec_attn="packed"), oracle)
        assert rows == want and packed == want, drafts
        assert steps == rows_steps
        if drafts == "oracle":
            assert steps < plain_steps / 2, (steps, plain_steps)
