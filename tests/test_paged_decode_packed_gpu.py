"""Packed multi-token paged decode (csrc/attention_decode_packed.hip) on the
MI355X, held to the comparator of test_kernel_edges_gpu.py: every output
finite and within atol + rtol*|want| of the fp64 reference (BF16_TOL for a
bf16 cache, FP8_TOL for an fp8 one), no share excused.  The cases come from
`_prefill_case` of test_paged_prefill_gpu.py: shuffled tables, NaN in
everything the kernel must not read, the fp64 reference.  Hkv = 2 there, so
every call has B*2 workgroups per split.

splits: 0 is the binding's rule, a positive value forces that many.  The rule
sees max_blocks * block_size of about 1040 rows here and picks 8 for the tile
case, so the default path already merges splits of which most are empty for
the short sequences.
"""
import pytest
import torch

import modal_examples_amd.ops.functional as F
import modal_examples_amd.ops.reference as ref
from modal_examples_amd.ops._build import get_ext
from test_kernel_edges_gpu import BF16_TOL, FP8_TOL, _close_all, gpu_test
from test_paged_prefill_gpu import _DECODE_PAIRS, HKV, _prefill_case

# (n, prefix), G = 4: S = 31, 32, 33 around the first kv tile with the causal
# diagonal across the tile edge; a sequence with no new tokens; a run that
# ends at the 4-wave round (128 rows); several rounds per wave
_PAIRS = ((1, 0), (5, 0), (8, 23), (8, 24), (8, 25), (0, 40), (3, 126),
          (8, 121), (5, 300), (2, 1000))


def _trim(G):
    return tuple((min(n, 32 // G), p) for n, p in _PAIRS)


_TILE_CASES = [(D, 4, _PAIRS, bs, fp8) for D in (64, 128) for bs in (16, 32)
               for fp8 in (False, True)]
_BLOCK_CASES = [(128, 4, _PAIRS, bs) for bs in (8, 24, 48)]
_GQA_CASES = [(D, G, _trim(G)) for D in (64, 128) for G in (1, 2, 3, 5, 8)]
_PEAKED_CASES = [(D, 4, _PAIRS, 16, fp8, 6.0) for D in (64, 128)
                 for fp8 in (False, True)]
_ROW_PAIRS = tuple((8, p) for _, p in _PAIRS)
_DECODE_CASES = [(D, 4, _DECODE_PAIRS, 16, fp8) for D in (64, 128)
                 for fp8 in (False, True)]


def _ids(cases):
    return ["-".join(str(x) for x in (c[:2] + c[3:])) for c in cases]


def _packed(c, q, cu, lens, max_q_len, splits=0):
    return get_ext(required=True).paged_decode_packed(
        q.cuda(), c.kc.cuda(), c.vc.cuda(),
        c.bt.repeat_interleave(len(lens) // len(c.lens), 0).cuda(), cu.cuda(),
        lens.cuda(), c.block_size, c.sc, max_q_len, splits=splits)


def _run(*case, splits=0):
    c = _prefill_case(*case)
    atol, rtol = FP8_TOL if c.fp8 else BF16_TOL
    if splits:
        out = _packed(c, c.q, c.cu, c.lens, c.max_n, splits)
    else:  # the public op: the rule's splits
        out = F.paged_decode_packed(c.q.cuda(), c.kc.cuda(), c.vc.cuda(),
                                    c.bt.cuda(), c.cu.cuda(), c.lens.cuda(),
                                    c.block_size, scale=c.scale,
                                    max_q_len=c.max_n)
    assert out.shape == c.q.shape and out.dtype == torch.bfloat16
    _close_all(out, c.want, atol, rtol,
               what=f"paged_decode_packed{case} splits={splits}")


@gpu_test
@pytest.mark.parametrize("case", _TILE_CASES + _BLOCK_CASES,
                         ids=_ids(_TILE_CASES + _BLOCK_CASES))
def test_tile_mask_and_block_edges(case):
    _run(*case)


@gpu_test
@pytest.mark.parametrize("case", _GQA_CASES, ids=_ids(_GQA_CASES))
def test_gqa_packing(case):
    _run(*case)


@gpu_test
@pytest.mark.parametrize("splits", (1, 2, 4, 8, 0))
def test_splits(splits):
    _run(128, 4, _PAIRS, splits=splits)


@gpu_test
@pytest.mark.parametrize("case", _PEAKED_CASES, ids=_ids(_PEAKED_CASES))
def test_peaked_softmax(case):
    _run(*case)


@gpu_test
@pytest.mark.parametrize("D", (64, 128))
def test_rows_do_not_see_each_other(D):
    """A row's output is the same bits whether it shares the tile with the 7
    other rows of its run or is a sequence of its own (n = 1, seq_len = its
    position + 1) over the same cache."""
    c = _prefill_case(D, 4, _ROW_PAIRS)
    R = c.q.shape[0]
    together = _packed(c, c.q, c.cu, c.lens, 8, splits=1)
    pos = torch.cat([torch.arange(p, p + 8) for _, p in _ROW_PAIRS])
    alone = _packed(c, c.q, torch.arange(R + 1, dtype=torch.int32),
                    (pos + 1).int(), 1, splits=1)
    assert torch.equal(together, alone)
    _close_all(together, c.want, *BF16_TOL, what=f"row case D={D}")


@gpu_test
@pytest.mark.parametrize("splits", (1, 0))
def test_loose_and_tight_max_q_len_agree(splits):
    """Runs of 3 and 5 at G = 4: max_q_len = 5 is tight, 8 the loosest legal."""
    c = _prefill_case(128, 4, ((3, 126), (5, 300)))
    tight = _packed(c, c.q, c.cu, c.lens, c.max_n, splits)
    assert torch.equal(tight, _packed(c, c.q, c.cu, c.lens, 8, splits))
    _close_all(tight, c.want, *BF16_TOL, what=f"max_q_len case splits={splits}")


@gpu_test
@pytest.mark.parametrize("splits", (1, 2))
def test_rows_at_negative_positions_are_zero(splits):
    """seq_len 5 under a run of 8 (over the cache of an (8, 24) case): queries
    0..2 sit at positions -3..-1 and return zeros, the rest see kv <= t - 3."""
    c = _prefill_case(64, 4, ((8, 24),))
    lens = torch.tensor([5], dtype=torch.int32)
    want = ref.paged_prefill_ref(c.q.double(), c.kc.float().double(),
                                 c.vc.float().double(), c.bt, c.cu, lens,
                                 c.block_size, c.sc)
    out = _packed(c, c.q, c.cu, lens, 8, splits)
    assert (out[:3] == 0).all() and (want[:3] == 0).all()
    _close_all(out, want, *BF16_TOL, what=f"negative positions splits={splits}")


@gpu_test
@pytest.mark.parametrize("case", _DECODE_CASES, ids=_ids(_DECODE_CASES))
def test_single_token_rows_agree_with_paged_decode(case):
    c = _prefill_case(*case)
    atol, rtol = FP8_TOL if c.fp8 else BF16_TOL
    _run(*case)
    dec = F.paged_decode(c.q.cuda(), c.kc.cuda(), c.vc.cuda(), c.bt.cuda(),
                         c.lens.cuda(), block_size=c.block_size)
    _close_all(dec, c.want, atol, rtol, what=f"paged_decode{case}")


@gpu_test
def test_bad_arguments_raise_before_launch():
    case = (64, 4, ((3, 5), (8, 0)))
    c = _prefill_case(*case)
    q, kc, vc = c.q.cuda(), c.kc.cuda(), c.vc.cuda()
    bt, cu, lens = c.bt.cuda(), c.cu.cuda(), c.lens.cuda()
    bs, (R, Hq), nb = c.block_size, q.shape[:2], kc.shape[0]

    def call(q=q, kc=kc, vc=vc, bt=bt, **kw):
        return F.paged_decode_packed(q, kc, vc, bt, cu, lens, bs, **kw)

    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")  # noqa: E731
    with pytest.raises(ValueError, match="32"):
        call()  # max_q_len = R = 11, G = 4
    with pytest.raises(ValueError, match="32"):
        call(max_q_len=9)
    with pytest.raises(RuntimeError, match="head_dim"):
        call(q=z(R, Hq, 96), kc=z(nb, HKV, bs, 96), vc=z(nb, HKV, bs, 96),
             max_q_len=8)
    with pytest.raises(RuntimeError, match="Hq % Hkv"):
        call(q=z(R, 3, 64), max_q_len=8)
    with pytest.raises(RuntimeError, match="device"):
        call(bt=c.bt, max_q_len=8)
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        call(vc=vc.to(torch.float8_e4m3fn), max_q_len=8)
    empty = F.paged_decode_packed(q[:0], kc, vc, bt, torch.zeros_like(cu),
                                  lens, bs)
    assert empty.shape == (0, Hq, 64)
    torch.cuda.synchronize()
    _run(*case)
