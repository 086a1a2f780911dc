"""CPU side of test_attention_fwd_paths_gpu.py: the judge of
test_attention_forward.py can be trusted with a non-positive scale.  For the
shapes and scales of the GPU file, its yardstick has a positive error e_y,
it accepts what a correct kernel returns (the fp64 truth rounded to bf16)
and the fp32 reference, and it still rejects a result computed with the
sign of the scale lost, or with the scale taken for the default."""
import pytest
import torch

from modal_examples_amd.ops import reference as ref
from test_attention_forward import (DS, judge, kernel_like, random_case,
                                    rejected, shape_id)
from test_attention_fwd_paths_gpu import PATH_SHAPES, SCALES

NON_POSITIVE = [s for s in SCALES if s is not None and s <= 0]


def test_the_gpu_file_runs_both_non_positive_scales():
    assert NON_POSITIVE == [-0.25, 0.0]


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("scale", NON_POSITIVE, ids=lambda s: f"scale{s}")
@pytest.mark.parametrize("shape", PATH_SHAPES, ids=shape_id)
def test_judge_takes_a_non_positive_scale(shape, scale, D):
    c = random_case(*shape, D, scale)
    label = f"random scale={scale} {shape_id(shape)} D{D}"
    assert c["scale"] == scale and c["e_y"] > 0
    judge(c, *kernel_like(c), label)
    o32 = ref.attention_ref(c["q"], c["k"], c["v"], c["causal"], scale)
    l32 = ref.attention_lse_ref(c["q"], c["k"], c["causal"], scale)
    judge(c, o32, l32, label + " fp32 ref")
    # a kernel that drops the sign, or ignores the scale, does not pass
    q, k, v = (c[n].double() for n in "qkv")
    for wrong in (abs(scale), None) if scale else (None,):
        o, lse = ref.attention_fwd_ref(q, k, v, c["causal"], wrong)
        assert rejected(c, o.to(torch.bfloat16), lse.float()), (label, wrong)
