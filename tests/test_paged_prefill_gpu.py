"""Paged prefill attention (csrc/attention_prefill_paged.hip) on the MI355X,
held to the strict comparator of test_kernel_edges_gpu.py: every output is
compared with the fp64 reference computed from the same bf16 /
fp8-dequantised values, every element finite and within atol + rtol*|want|
(BF16_TOL for a bf16 cache, FP8_TOL for an fp8 one), no share excused.

A case is a ragged batch of (n_b, prefix) pairs: n_b new tokens after
`prefix` cached ones, so seq_lens[b] = prefix + n_b.  Everything the kernel
has no business reading is NaN, as in `_decode_case`: cache rows past S_b in
a sequence's last block, every block no sequence owns, and the block that
the unused table slots name.  A finite, correct output proves none of it was
read.  Hkv = 2 and shuffled block tables throughout; fp8 caches hold
amplitude 0.5 like the decode cases.

The cases are module-level lists: test_paged_prefill.py walks all of them on
the CPU for the comparator floor.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import modal_examples_amd.ops.functional as F
import modal_examples_amd.ops.reference as ref
from test_kernel_edges_gpu import (BF16_TOL, FP8_TOL, _close_all, _gen,
                                   _randn, gpu_test)

HKV = 2


@functools.lru_cache(maxsize=None)
def _prefill_case(D, G, pairs, block_size=16, fp8=False, q_gain=1.0,
                  scale=None):
    """Inputs (CPU) and the fp64 reference of one paged_prefill call."""
    g = _gen(1000 * D + 100 * G + 7 * block_size + sum(n + 3 * p
                                                       for n, p in pairs))
    nan = float("nan")
    amp = 0.5 if fp8 else 1.0
    B = len(pairs)
    lens = [n + p for n, p in pairs]
    cu = [0]
    for n, _ in pairs:
        cu.append(cu[-1] + n)
    q = (_randn(g, cu[-1], HKV * G, D) * q_gain).to(torch.bfloat16)
    need = [(s + block_size - 1) // block_size for s in lens]
    nblocks, max_blocks = sum(need) + 5, max(need) + 2
    perm = torch.randperm(nblocks, generator=g)
    kc = _randn(g, nblocks, HKV, block_size, D) * amp
    vc = _randn(g, nblocks, HKV, block_size, D) * amp
    kc[perm[sum(need):]] = nan
    vc[perm[sum(need):]] = nan
    bt = torch.full((B, max_blocks), int(perm[sum(need)]), dtype=torch.int32)
    at = 0
    for b, s in enumerate(lens):
        bt[b, : need[b]] = perm[at: at + need[b]].int()
        at += need[b]
        if s % block_size:  # rows past S_b in the last block
            last = int(bt[b, need[b] - 1])
            kc[last, :, s % block_size:] = nan
            vc[last, :, s % block_size:] = nan
    cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kc, vc = kc.to(cdt), vc.to(cdt)
    assert torch.isnan(kc.float()).any()
    cu_t = torch.tensor(cu, dtype=torch.int32)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    want = ref.paged_prefill_ref(q.double(), kc.float().double(),
                                 vc.float().double(), bt, cu_t, lens_t,
                                 block_size, sc)
    assert torch.isfinite(want).all()
    return SimpleNamespace(q=q, kc=kc, vc=vc, bt=bt, cu=cu_t, lens=lens_t,
                           block_size=block_size, scale=scale, sc=sc, fp8=fp8,
                           pairs=pairs, max_n=max(n for n, _ in pairs),
                           want=want)


def _run_prefill(*case, max_q_len="tight"):
    c = _prefill_case(*case)
    atol, rtol = FP8_TOL if c.fp8 else BF16_TOL
    mq = {"tight": c.max_n, "loose": None}[max_q_len]
    out = F.paged_prefill(c.q.cuda(), c.kc.cuda(), c.vc.cuda(), c.bt.cuda(),
                          c.cu.cuda(), c.lens.cuda(), c.block_size,
                          scale=c.scale, max_q_len=mq)
    assert out.shape == c.q.shape and out.dtype == torch.bfloat16
    _close_all(out, c.want, atol, rtol, what=f"paged_prefill{case}")
    return out


# around the 32-query wave, the 128-query workgroup and the 32- and 64-row
# KV tiles; (0, 40) is a sequence with no new tokens in the middle
_EDGE_PAIRS = ((1, 0), (31, 1), (32, 15), (33, 16), (0, 40), (127, 33),
               (128, 63), (129, 65), (160, 0))
_TILE_CASES = [(D, 4, _EDGE_PAIRS, bs, fp8) for D in (64, 128)
               for bs in (16, 32) for fp8 in (False, True)]
# (5, 300): a short chunk far into a long prefix — most of its tile's queries
# are dead and many KV tiles are unmasked
_GQA_PAIRS = ((33, 16), (5, 300), (129, 65))
_GQA_CASES = [(D, G, _GQA_PAIRS) for D in (64, 128) for G in (1, 2, 3, 5, 8)]
# 8: several blocks per KV tile; 24: blocks and tiles drift against each
# other; 48: a block longer than either KV tile
_BLOCK_CASES = [(D, 2, _GQA_PAIRS, bs) for D in (64, 128) for bs in (8, 24, 48)]
# q scaled by 6: the running maxima move and defer-max has to rescale
_PEAKED_CASES = [(D, 2, _GQA_PAIRS, 16, fp8, 6.0) for D in (64, 128)
                 for fp8 in (False, True)]
_SCALE_CASES = [(D, 2, _GQA_PAIRS, 16, False, 1.0, 0.3) for D in (64, 128)]
_MAXQ_CASE = (128, 4, ((3, 70), (130, 5), (40, 0)))
# n_b = 1 everywhere: the decode kernel's job, on both sides of a block edge
_DECODE_PAIRS = ((1, 0), (1, 15), (1, 16), (1, 99), (1, 300))
_DECODE_CASES = [(D, 4, _DECODE_PAIRS, 16, fp8) for D in (64, 128)
                 for fp8 in (False, True)]
ALL_CASES = (_TILE_CASES + _GQA_CASES + _BLOCK_CASES + _PEAKED_CASES
             + _SCALE_CASES + [_MAXQ_CASE] + _DECODE_CASES)


def _ids(cases):
    return ["-".join(str(x) for x in (c[:2] + c[3:])) for c in cases]


@gpu_test
@pytest.mark.parametrize("case", _TILE_CASES, ids=_ids(_TILE_CASES))
def test_tile_edges(case):
    out = _run_prefill(*case)
    assert out.shape[0] == sum(n for n, _ in _EDGE_PAIRS)


@gpu_test
@pytest.mark.parametrize("case", _GQA_CASES, ids=_ids(_GQA_CASES))
def test_gqa_groups(case):
    _run_prefill(*case)


@gpu_test
@pytest.mark.parametrize("case", _BLOCK_CASES, ids=_ids(_BLOCK_CASES))
def test_block_sizes(case):
    _run_prefill(*case)


@gpu_test
@pytest.mark.parametrize("case", _PEAKED_CASES, ids=_ids(_PEAKED_CASES))
def test_peaked_softmax(case):
    _run_prefill(*case)


@gpu_test
@pytest.mark.parametrize("case", _SCALE_CASES, ids=_ids(_SCALE_CASES))
def test_explicit_scale(case):
    _run_prefill(*case)


@gpu_test
def test_loose_and_tight_max_q_len_agree():
    """max_q_len only sizes the grid: T (the default) launches idle tiles
    that exit at once, the exact maximum launches none; same output."""
    tight = _run_prefill(*_MAXQ_CASE, max_q_len="tight")
    loose = _run_prefill(*_MAXQ_CASE, max_q_len="loose")
    assert torch.equal(tight, loose)


@gpu_test
@pytest.mark.parametrize("case", _DECODE_CASES, ids=_ids(_DECODE_CASES))
def test_single_token_rows_agree_with_paged_decode(case):
    """n_b = 1 is a decode step: both kernels sit within the same bound of
    the same reference."""
    c = _prefill_case(*case)
    atol, rtol = FP8_TOL if c.fp8 else BF16_TOL
    _run_prefill(*case)
    dec = F.paged_decode(c.q.cuda(), c.kc.cuda(), c.vc.cuda(), c.bt.cuda(),
                         c.lens.cuda(), block_size=c.block_size)
    _close_all(dec, c.want, atol, rtol, what=f"paged_decode{case}")


@gpu_test
def test_empty_batch_returns_empty():
    c = _prefill_case(64, 2, ((3, 5),))
    out = F.paged_prefill(c.q[:0].cuda(), c.kc.cuda(), c.vc.cuda(),
                          c.bt.cuda(), torch.zeros(2, dtype=torch.int32).cuda(),
                          c.lens.cuda(), c.block_size)
    assert out.shape == (0, 4, 64)


@gpu_test
def test_bad_arguments_raise_before_launch():
    """Each bad argument raises on the host; a valid call afterwards is
    still right."""
    from modal_examples_amd.ops._build import get_ext

    ext = get_ext(required=True)
    case = (64, 2, ((3, 5), (9, 0)))
    c = _prefill_case(*case)
    q, kc, vc = c.q.cuda(), c.kc.cuda(), c.vc.cuda()
    bt, cu, lens = c.bt.cuda(), c.cu.cuda(), c.lens.cuda()
    bs = c.block_size

    def call(q=q, kc=kc, vc=vc, bt=bt, cu=cu, lens=lens, bs=bs):
        return F.paged_prefill(q, kc, vc, bt, cu, lens, bs)

    T, Hq = q.shape[0], q.shape[1]
    nb = kc.shape[0]
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")  # noqa: E731
    with pytest.raises(RuntimeError, match="head_dim"):
        call(q=z(T, Hq, 80), kc=z(nb, HKV, bs, 80), vc=z(nb, HKV, bs, 80))
    with pytest.raises(RuntimeError, match="Hq % Hkv"):
        call(q=z(T, 3, 64))
    with pytest.raises(RuntimeError, match="dtype mismatch"):
        call(vc=vc.to(torch.float8_e4m3fn))
    # F routes an fp32 q to the reference, so the binding is asked directly
    with pytest.raises(RuntimeError, match="bf16"):
        ext.paged_prefill(q.float(), kc, vc, bt, cu, lens, bs, 0.125, T)
    with pytest.raises(RuntimeError, match="cu_q"):
        call(cu=cu[:-1])
    with pytest.raises(ValueError, match="block_table"):
        call(bt=None)
    with pytest.raises(RuntimeError, match="block_size"):
        call(bs=0)
    with pytest.raises(RuntimeError, match="max_q_len"):
        F.paged_prefill(q, kc, vc, bt, cu, lens, bs, max_q_len=0)
    torch.cuda.synchronize()
    _run_prefill(*case)
