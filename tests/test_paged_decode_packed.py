"""F.paged_decode_packed off the GPU (the reference, by specification) and the
engine's spec_attn knob, on the pattern of test_spec_decode.py."""
import pytest
import torch

import modal_examples_amd.ops.functional as F
import modal_examples_amd.ops.reference as ref
from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.models.llama.model import LlamaConfig
from test_paged_prefill_gpu import _prefill_case
from test_spec_decode import _greedy


def test_cpu_op_is_the_reference_and_checks_its_arguments():
    c = _prefill_case(64, 4, ((3, 5), (8, 0), (0, 9), (1, 40)))
    args = (c.q, c.kc, c.vc, c.bt, c.cu, c.lens, c.block_size)
    want = ref.paged_prefill_ref(*args)
    assert torch.equal(F.paged_decode_packed(*args, max_q_len=8), want)
    k8, v8 = (t.nan_to_num(0.0).to(torch.float8_e4m3fn) for t in (c.kc, c.vc))
    want8 = ref.paged_prefill_ref(c.q, k8.float(), v8.float(), *args[3:])
    assert torch.equal(
        F.paged_decode_packed(c.q, k8, v8, *args[3:], max_q_len=8), want8)
    assert F.paged_decode_packed(c.q[:0], c.kc, c.vc, c.bt,
                                 torch.zeros_like(c.cu), c.lens,
                                 c.block_size).shape == (0, 8, 64)
    with pytest.raises(ValueError, match="32"):
        F.paged_decode_packed(*args)  # max_q_len = R = 12, G = 4
    with pytest.raises(ValueError, match="32"):
        F.paged_decode_packed(*args, max_q_len=9)
    with pytest.raises(ValueError, match="block_table"):
        F.paged_decode_packed(c.q, c.kc, c.vc, None, *args[4:], max_q_len=8)


def _mk(spec_tokens=0, **kw):
    return LlamaEngine(LlamaConfig.small(), device="cpu", dtype=torch.bfloat16,
                       use_graph=False, eos_id=-1, seed=0,
                       spec_tokens=spec_tokens, **kw)


def test_packed_spec_lane_matches_plain_decode():
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(0, 1024, (7,), generator=g).tolist(),
               [3, 4, 5, 3, 4, 5, 3, 4],  # repetitive: drafts will fire
               torch.randint(0, 1024, (11,), generator=g).tolist()]
    want, _ = _greedy(_mk(0), prompts)
    got, _ = _greedy(_mk(4, spec_attn="packed"), prompts)
    assert got == want

    # oracle drafts: full runs every step, fewer than half the steps
    want, plain_steps = _greedy(_mk(0), prompts[:1], n=12)
    eng = _mk(4, spec_attn="packed")
    eng._propose = lambda r: want[0][len(r.out_tokens):
                                     len(r.out_tokens) + eng.spec_tokens]
    got, spec_steps = _greedy(eng, prompts[:1], n=12)
    assert got == want and eng.spec_accepted >= 8
    assert spec_steps < plain_steps / 2, (spec_steps, plain_steps)


def test_spec_attn_knob_is_checked_at_construction():
    with pytest.raises(ValueError, match="spec_attn"):
        _mk(4, spec_attn="bogus")
    with pytest.raises(ValueError, match="32"):
        _mk(16, spec_attn="packed")  # 17 positions x G = 2
    assert _mk(16).spec_attn == "rows"
