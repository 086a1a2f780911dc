"""Edge and dispatch cases of the decode, sampling, norm, elementwise and
3x3 convolution kernels, each against a float64 reference of the same
operation.

`test_kernels_gpu.py` compares every kernel with a reference at one friendly
shape and excuses 0.1 % of the elements.  This file goes where kernels break:
every GQA instantiation of the paged decode, empty splits, lengths around the
prefetch depth, block tables with fp8 and ragged lengths, the vocabulary split
of the sampler, the split statistics of GroupNorm, offset activations, ragged
tails, and for the convolution the channel, output-channel and spatial tails
of its 64 x 8 x 32 tile, the XCD renumbering, the fused upsample, residual and
GroupNorm, the 4-rows-per-wave variant and the bindings' argument checks.
Nothing is excused: `_close_all` wants every element finite and within
`atol + rtol*|want|`, and the integer cases of the plain convolution, whose
result no rounding touches, want every element equal (`_exact`).

GPU tests carry `pytest.mark.gpu` and the `requires_gpu` skip, one by one and
not through a module-level `pytestmark`, because the tests of the sampler host
model and of the comparator floor at the end of each section are plain CPU
tests: they have to stay unmarked to run with the CPU suite.

Figures this file relies on (all measured on the CPU by the unmarked tests
below, which print them and assert the stated relation):

* Comparator floor, `max |bf16(f32 reference) - f64 reference| / (atol +
  rtol*|ref|)`, over every decode and norm case here: 0.164 of the bound
  for bf16 at 2e-2/2e-2 (the half-ulp of bf16, up to 2^-8 relative, over
  rtol, reached by the norms where |ref| is a few units; the decode cases
  reach 0.113) and 0.042 for the fp8-cache cases at 3e-2/3e-2.  Both
  tolerances sit more than the 4x above the floor that fast exp and
  summation order are given, so neither atol is raised.  The fused
  GroupNorm+conv, whose f32 model rounds the MFMA operands to bf16, has a
  floor of 0.46 at 2e-2/2e-2 and 0.183 at the project's conv bound of
  5e-2/5e-2; it is held to the latter.  The GroupNorm edge cases (K = 65,
  C = 24 in 3 groups, upsample, residual, two offset images) stay below
  that: 0.167, 0.111, 0.150, 0.165.
* Plain convolution at ROUND_TOL (1e-3, 2^-7), which is derived and not
  measured: the f32 model rounded to bf16 sits at 0.482 of the bound at
  most over the real-valued cases (below the 0.5 that one rounding of 2^-8
  relative can take), the f32 model's own summation error at 3.3e-4 of it.
* Exact convolution cases: largest |want| per group is 118 (channel
  tails), 62 (output-channel tails), 65 and 73 (spatial edges of the 8-row
  and the 16-row tile), 73 (swizzle), 124 (C = 320 at a weight density of
  1/4), 76 (upsample), 75 (residual); the condition is 256, up to which
  every integer is a bf16 value.
* Sampler: |float32 numpy Gumbel - float64 Gumbel| is 3.7e-7 at most for
  Gumbel values below 7; a x1000 margin for the hardware fast log near
  u -> 1 gives DELTA = 1e-3.
* Share of draws whose float64 top-two gap is below DELTA (rows = 8,
  V in {1000, 4099}, logits 2*randn, seeds 1..512): 11 of 8192, 0.13 %;
  the cap is 1 %.
* Host-model chi-square of the V = 16 distribution case (4096 rows,
  seed 1234, T = 1): 12.38; the threshold is 56 (1e-6 quantile, 15 d.o.f.).

Out of scope: rows whose start is not 16-byte aligned (LayerNorm with
D % 8 != 0, GroupNorm with HW % 8 != 0).  Whether the kernels' bf16x8 loads
may be misaligned is to be settled by reading the code, not by a run.
"""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import modal_examples_amd.ops.functional as F

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def gpu_test(fn):
    return pytest.mark.gpu(requires_gpu(fn))


BF16_TOL = (2e-2, 2e-2)   # the project's bound for bf16 in / bf16 out
FP8_TOL = (3e-2, 3e-2)    # ... and for an fp8 KV cache
CONV_TOL = (5e-2, 5e-2)   # ... and for the bf16 MFMA convolution
# one bf16 rounding of an f32 result: half an ulp is at most 2^-8 relative
# (8 significand bits); 2x margin
ROUND_TOL = (1e-3, 2.0 ** -7)


# ===================================================================== 1.
# strict comparator

def _err_ratio(got, want64, atol, rtol):
    got = got.detach().double().cpu()
    want = want64.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want).abs() / (atol + rtol * want.abs())


def _close_all(got, want64, atol=BF16_TOL[0], rtol=BF16_TOL[1], what=""):
    """Every element finite and within atol + rtol*|want|; no excused share.
    Returns the worst error as a fraction of the bound."""
    g = got.detach().double().cpu()
    bad = ~torch.isfinite(g)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} non-finite outputs, first at "
        f"{tuple(bad.nonzero()[0].tolist())}")
    ratio = _err_ratio(got, want64, atol, rtol)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: worst error {worst:.4f} of the bound")
    if worst > 1.0:
        idx = tuple(np.unravel_index(int(ratio.argmax()), ratio.shape))
        raise AssertionError(
            f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements "
            f"outside atol={atol} rtol={rtol}; worst {worst:.3f}x the bound "
            f"at {idx}: got {float(g[idx])}, want {float(want64.cpu()[idx])}")
    return worst


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ===================================================================== 2.
# paged decode

HKV = 2
NPART = {64: 32, 128: 16}  # softmax partials per workgroup = prefetch stride


def _decode_ref(q, kc, vc, bt, lens, block_size, scale, dtype):
    """softmax(q k^T * scale) v over rows [:len], in `dtype`, from the same
    bf16 / fp8-dequantised values the kernel reads.  len 0 gives zeros."""
    B, Hq, D = q.shape
    Hkv = kc.shape[1]
    G = Hq // Hkv
    kf, vf = kc.float().to(dtype), vc.float().to(dtype)
    out = torch.zeros(B, Hq, D, dtype=dtype)
    for b in range(B):
        S = int(lens[b])
        if S == 0:
            continue
        if bt is None:
            k, v = kf[b, :, :S], vf[b, :, :S]
        else:
            idx = bt[b, : (S + block_size - 1) // block_size].long()
            k = kf[idx].permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :S]
            v = vf[idx].permute(1, 0, 2, 3).reshape(Hkv, -1, D)[:, :S]
        qg = q[b].float().to(dtype).view(Hkv, G, D)  # head h = hkv*G + g
        p = torch.softmax(torch.einsum("hgd,hsd->hgs", qg, k) * scale, -1)
        out[b] = torch.einsum("hgs,hsd->hgd", p, v).reshape(Hq, D)
    return out


@functools.lru_cache(maxsize=None)
def _decode_case(D, G, S, lens, block_size=0, fp8=False, q_gain=1.0,
                 scale=None):
    """Inputs (CPU) and references for one decode call.  Everything the
    kernel has no business reading is NaN: rows at index >= len, every cache
    block no sequence needs, and the block that the unused table slots name
    (a valid index).  A finite, correct output proves none of it was read."""
    B = len(lens)
    g = _gen(1000 * D + 100 * G + S + 7 * block_size + sum(lens))
    nan = float("nan")
    amp = 0.5 if fp8 else 1.0
    q = (_randn(g, B, HKV * G, D) * q_gain).to(torch.bfloat16)
    if block_size == 0:
        kc, vc = _randn(g, B, HKV, S, D) * amp, _randn(g, B, HKV, S, D) * amp
        for b, n in enumerate(lens):
            kc[b, :, n:] = nan
            vc[b, :, n:] = nan
        bt = None
    else:
        need = [(n + block_size - 1) // block_size for n in lens]
        nblocks, max_blocks = sum(need) + 5, max(need) + 2
        perm = torch.randperm(nblocks, generator=g)
        kc = _randn(g, nblocks, HKV, block_size, D) * amp
        vc = _randn(g, nblocks, HKV, block_size, D) * amp
        kc[perm[sum(need):]] = nan
        vc[perm[sum(need):]] = nan
        bt = torch.full((B, max_blocks), int(perm[sum(need)]), dtype=torch.int32)
        at = 0
        for b, n in enumerate(lens):
            bt[b, : need[b]] = perm[at: at + need[b]].int()
            at += need[b]
            if n % block_size:  # rows past len in the last block
                last = int(bt[b, need[b] - 1])
                kc[last, :, n % block_size:] = nan
                vc[last, :, n % block_size:] = nan
    cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    kc, vc = kc.to(cdt), vc.to(cdt)
    assert torch.isnan(kc.float()).any() or all(n == S for n in lens)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    sc = scale if scale is not None else 1.0 / math.sqrt(D)
    args = (q, kc, vc, bt, lens_t, block_size, sc)
    want = _decode_ref(*args, torch.float64)
    assert torch.isfinite(want).all()
    return SimpleNamespace(q=q, kc=kc, vc=vc, bt=bt, lens=lens_t,
                           block_size=block_size, scale=scale, fp8=fp8,
                           want=want, want32=_decode_ref(*args, torch.float32))


def _run_decode(*case):
    c = _decode_case(*case)
    atol, rtol = FP8_TOL if c.fp8 else BF16_TOL
    out = F.paged_decode(c.q.cuda(), c.kc.cuda(), c.vc.cuda(),
                         c.bt.cuda() if c.bt is not None else None,
                         c.lens.cuda(), block_size=c.block_size, scale=c.scale)
    _close_all(out, c.want, atol, rtol, what=f"decode{case}")
    for b in (c.lens == 0).nonzero().flatten().tolist():
        assert (out[b].float() == 0).all(), "len 0 must give exact zeros"


# (S, lens): S = 160 gives two splits and the merge kernel, S = 96 one split
# and the direct write
_GQA_CACHES = [(160, (160, 37)), (96, (96, 1))]
_GQA_CASES = [(D, G, S, lens) for D in (64, 128) for G in (1, 2, 3, 5, 8)
              for S, lens in _GQA_CACHES]


def _edge_lens(D, S):
    n = NPART[D]
    return (0, 1, n - 1, n, n + 1, 2 * n + 1, S)


_EDGE_CASES = [(D, 4, S, _edge_lens(D, S)) for D in (64, 128) for S in (96, 160)]
# capacity 4096 at B*Hkv = 2 gives 32 splits; these lengths leave 27 of them
# empty, and all but the first two almost empty
_SHORT_CASES = [(128, 4, 4096, (5,)), (128, 4, 4096, (129,))]
# block tables: 7-block tables of 16 rows stay one split, of 32 rows take two
_PAGED_LENS = (45, 7, 83)
_PAGED_CASES = [(D, G, 0, _PAGED_LENS, bs, fp8) for D in (64, 128)
                for G in (1, 4, 8) for bs in (16, 32) for fp8 in (False, True)]
# q scaled by 6: scores ~ N(0, 36), so the maxima of the partials and of the
# two splits differ by tens and both merges have to re-align them
_PEAKED_CASE = (128, 4, 160, (160, 37), 0, False, 6.0)
_SCALE_CASE = (64, 2, 160, (160, 37), 0, False, 1.0, 0.3)
_DECODE_CASES = (_GQA_CASES + _EDGE_CASES + _SHORT_CASES + _PAGED_CASES
                 + [_PEAKED_CASE, _SCALE_CASE])


@gpu_test
@pytest.mark.parametrize("case", _GQA_CASES, ids=str)
def test_decode_gqa_sweep(case):
    """Every GT instantiation (1, 2, 4 with a dead group at G=3, 8 at G=5
    and at the full G=8), split and unsplit."""
    _run_decode(*case)


@gpu_test
@pytest.mark.parametrize("case", _EDGE_CASES, ids=str)
def test_decode_length_edges(case):
    """len 0, 1 and the lengths around NPART and 2*NPART, where the depth-2
    prefetch has nothing, one row or two rows in flight."""
    _run_decode(*case)


@gpu_test
@pytest.mark.parametrize("case", _SHORT_CASES, ids=str)
def test_decode_short_sequence_in_large_cache(case):
    """splits follows the cache capacity, so most splits are empty and
    hand the merge (m=-1e30, l=0) partials."""
    _run_decode(*case)


@gpu_test
@pytest.mark.parametrize("case", _PAGED_CASES, ids=str)
def test_decode_paged_ragged(case):
    """Permuted block table, lengths that are no multiple of the block,
    bf16 and fp8 caches."""
    _run_decode(*case)


@gpu_test
def test_decode_peaked_softmax():
    _run_decode(*_PEAKED_CASE)


@gpu_test
def test_decode_explicit_scale():
    _run_decode(*_SCALE_CASE)


# ===================================================================== 3.
# sampler

DELTA = 1e-3
_M32 = np.uint64(0xFFFFFFFF)


def _hash3(a, b, c):
    """The kernel's hash3 on uint32 values, kept in uint64 and masked."""
    a, b, c = (np.asarray(x, dtype=np.uint64) for x in (a, b, c))
    h = ((a * np.uint64(0x9E3779B1)) ^ (b * np.uint64(0x85EBCA77))
         ^ (c * np.uint64(0xC2B2AE3D))) & _M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & _M32
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & _M32
    h ^= h >> np.uint64(15)
    return h


def _uniform_f32(rows, V, seed):
    """uf exactly as the kernel forms it, float32 [rows, V]."""
    seed &= (1 << 64) - 1  # the binding's int64 -> unsigned long long
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    row = np.arange(rows, dtype=np.uint64)[:, None]
    u = _hash3(lo, np.uint64(hi) ^ row, np.arange(V, dtype=np.uint64)[None, :])
    return ((u >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
            + np.float32(1e-10))


def gumbel_scores(logits, temperature, seed):
    """float64 scores logits/T + Gumbel(seed, row, i) of the sampling kernel."""
    lg = np.asarray(logits, dtype=np.float32)
    uf = _uniform_f32(lg.shape[0], lg.shape[1], seed)
    inv_t = np.float32(1.0) / np.float32(temperature)  # the launcher's f32
    return lg.astype(np.float64) * np.float64(inv_t) - np.log(-np.log(uf.astype(np.float64)))


def gumbel_expected(logits, temperature, seed):
    """The token the kernel must pick for each row, near-ties aside."""
    return gumbel_scores(logits, temperature, seed).argmax(-1)


def _chi2_logits():
    return np.linspace(-1.5, 1.5, 16, dtype=np.float32) * np.float32(1.25)


CHI2_ROWS, CHI2_SEED, CHI2_MAX = 4096, 1234, 56.0


def _chi2(tokens):
    lg = _chi2_logits().astype(np.float64)
    p = np.exp(lg - lg.max())
    want = CHI2_ROWS * p / p.sum()
    got = np.bincount(np.asarray(tokens, dtype=np.int64), minlength=16)
    assert got.sum() == CHI2_ROWS and len(got) == 16
    return float(((got - want) ** 2 / want).sum())


def _check_sample(logits, temperature, seed):
    """F.sample against the host model on one call.  Returns (excused, rows):
    a pick may differ from the model's only where the model scores it within
    DELTA of its best."""
    lg = logits.numpy()
    scores = gumbel_scores(lg, temperature, seed)
    tok = F.sample(logits.cuda(), temperature, seed=seed).cpu().numpy().astype(np.int64)
    assert tok.shape == (lg.shape[0],)
    assert ((tok >= 0) & (tok < lg.shape[1])).all(), tok
    picked = scores[np.arange(len(tok)), tok]
    gap = scores.max(-1) - picked
    assert np.isfinite(picked).all(), "sampled a masked (-inf) token"
    assert (gap <= DELTA).all(), (
        f"rows {np.nonzero(gap > DELTA)[0][:8]} picked a token scoring "
        f"{gap.max():.4g} below the model's best (V={lg.shape[1]} "
        f"T={temperature} seed={seed})")
    return int((tok != scores.argmax(-1)).sum()), len(tok)


_SEEDS = (0, 1, 2 ** 32 + 3, -12345)
_TEMPS = (0.7, 1.0, 2.5)


@gpu_test
@pytest.mark.parametrize("V", [1, 255, 1025, 4099, 32003])
def test_sample_matches_host_model(V):
    """Exact-token agreement with the host model.  rows 1 and 5 split the
    vocabulary (2 chunks at 1025, 8 at 4099 with a short last one, 32 at
    32003); rows = 600 does not.  Every temperature meets every seed at the
    small row counts; at rows = 600 each seed and each temperature is used."""
    g = _gen(V)
    excused = total = 0
    for rows in (1, 5):
        logits = 2.0 * _randn(g, rows, V)
        for t in _TEMPS:
            for seed in _SEEDS:
                e, n = _check_sample(logits, t, seed)
                excused, total = excused + e, total + n
    logits = 2.0 * _randn(g, 600, V)
    for j, seed in enumerate(_SEEDS):
        e, n = _check_sample(logits, _TEMPS[j % 3], seed)
        excused, total = excused + e, total + n
    print(f"V={V}: {excused} of {total} picks excused as near-ties")
    assert excused <= 0.01 * total


@gpu_test
def test_sample_seed_zero_samples():
    """seed 0 is a seed like any other: with T > 0 the kernel hashes with 0
    and does not fall back to the argmax."""
    flat = torch.zeros(64, 1000)
    tok = F.sample(flat.cuda(), 1.0, seed=0).cpu().numpy()
    assert (tok == gumbel_expected(flat.numpy(), 1.0, 0)).all()
    assert (tok != 0).any(), "argmax of a flat row: seed 0 was taken as greedy"
    assert len(set(tok.tolist())) > 32


@gpu_test
def test_sample_top_p_masked_rows():
    """Rows as the engine's nucleus filter leaves them: a few kept tokens,
    everything else -inf, whole split chunks masked."""
    g = _gen(77)
    excused = total = 0
    for V, rows in ((4099, 5), (32003, 1), (4099, 600)):
        logits = torch.full((rows, V), float("-inf"))
        for r in range(rows):
            # kept tokens sit in the second 513-wide chunk (the first two
            # 1001-wide ones at V = 32003) and, in odd rows, in the last; the
            # first token of every chunk, a split's initial pick, is masked
            keep = torch.randint(520, 1020, (3 + r % 5,), generator=g)
            if r % 2:
                keep = torch.cat([keep, torch.tensor([V - 1 - r % 3])])
            logits[r, keep] = 2.0 * _randn(g, len(keep))
        for seed in _SEEDS:
            e, n = _check_sample(logits, 0.7 if seed else 1.0, seed)
            excused, total = excused + e, total + n
    print(f"masked rows: {excused} of {total} picks excused as near-ties")
    assert excused <= 0.01 * total


def _greedy_rows(V=4099):
    """Rows for T = 0 at V = 4099: 8 chunks of 513 below 512 rows, one
    thread per 256 and one wave per 64 inside a chunk."""
    g = _gen(5)
    rows = []

    def base():
        return _randn(g, V).clamp_(max=3.0)

    for dup in ((512, 513),      # last of chunk 0, first of chunk 1
                (600, 3000),     # two chunks apart
                (513 + 63, 513 + 64),    # neighbouring waves of one chunk
                (5, 5 + 256),    # the same thread, one stride apart
                (0, V - 1)):
        r = base()
        r[list(dup)] = 7.0
        rows.append(r)
    rows.append(base() - 100.0)                      # all negative
    r = -base().abs() - 1.0                          # zeros of both signs
    r[3], r[3000] = -0.0, 0.0
    rows.append(r)
    r = -base().abs() - 1.0
    r[700], r[100] = -0.0, 0.0
    rows.append(r)
    r = base()                                       # -inf, chunk starts too
    r[torch.rand(V, generator=g) < 0.5] = float("-inf")
    r[[0, 513, 1026, 4098]] = float("-inf")
    rows.append(r)
    r = torch.full((V,), float("-inf"))
    r[[2051, 2052]] = -3.0
    rows.append(r)
    return torch.stack(rows)


@gpu_test
def test_sample_greedy_first_index():
    """T = 0 is numpy's argmax: the first index among equal maxima, with
    -0.0 equal to +0.0, whatever split, wave or thread holds them."""
    x = _greedy_rows()
    want = x.numpy().argmax(-1)
    assert want[0] == 512 and want[6] == 3 and want[7] == 100
    for rows in (x[:5], x[5:], x.repeat(52, 1)):  # 8 splits twice, then none
        got = F.sample(rows.cuda(), temperature=0.0, seed=9).cpu().numpy()
        exp = rows.numpy().argmax(-1)
        assert (got == exp).all(), (np.nonzero(got != exp)[0], got, exp)


@gpu_test
def test_sample_distribution_chi_square():
    logits = torch.from_numpy(_chi2_logits()).repeat(CHI2_ROWS, 1)
    tok = F.sample(logits.cuda(), 1.0, seed=CHI2_SEED).cpu().numpy()
    stat = _chi2(tok)
    print(f"chi-square on GPU {stat:.2f}")
    assert stat <= CHI2_MAX


# ---- the sampler's CPU conditions (unmarked: they need no GPU)

def test_host_hash_known_answers():
    """The numpy hash against a scalar big-integer version of the same mix."""
    def scalar(a, b, c):
        m = 0xFFFFFFFF
        h = ((a * 0x9E3779B1) ^ (b * 0x85EBCA77) ^ (c * 0xC2B2AE3D)) & m
        h ^= h >> 15
        h = h * 0x2C1B3C6D & m
        h ^= h >> 12
        h = h * 0x297A2D39 & m
        return h ^ (h >> 15)

    assert scalar(0, 0, 0) == 0
    for seed in _SEEDS:
        s = seed & (1 << 64) - 1
        uf = _uniform_f32(7, 300, seed)
        for row, i in ((0, 0), (3, 17), (6, 299)):
            u = scalar(s & 0xFFFFFFFF, (s >> 32) ^ row, i)
            assert uf[row, i] == np.float32(u >> 8) * np.float32(2.0 ** -24) + np.float32(1e-10)
    assert 1e-10 <= uf.min() and uf.max() < 1.0
    # seed 0 is no special value of the model either
    assert (gumbel_expected(np.zeros((64, 1000), np.float32), 1.0, 0) != 0).any()


def test_host_gumbel_precision_sets_delta():
    """DELTA is 1000x the float32-vs-float64 Gumbel difference below 7."""
    uf = _uniform_f32(64, 32003, 3)
    g64 = -np.log(-np.log(uf.astype(np.float64)))
    g32 = -np.log(-np.log(uf))
    assert g32.dtype == np.float32
    diff = np.abs(g32.astype(np.float64) - g64)[g64 < 7.0].max()
    print(f"float32 vs float64 Gumbel below 7: {diff:.3g}")
    assert 1000.0 * diff <= DELTA


def test_host_near_tie_share():
    """Draws the GPU check may excuse are rare: top-two gap below DELTA in
    at most 1 % of them."""
    near = total = 0
    for V in (1000, 4099):
        lg = (2.0 * _randn(_gen(V), 8, V)).numpy()
        for seed in range(1, 513):
            top2 = np.partition(gumbel_scores(lg, 1.0, seed), -2, axis=-1)[:, -2:]
            near += int(((top2[:, 1] - top2[:, 0]) < DELTA).sum())
            total += 8
    print(f"near-tie share {near}/{total} = {near / total:.5f}")
    assert near <= 0.01 * total


def test_host_chi_square_precheck():
    """The seed of the distribution test is picked so that the host model
    itself is under the threshold the GPU has to meet."""
    lg = np.tile(_chi2_logits(), (CHI2_ROWS, 1))
    stat = _chi2(gumbel_expected(lg, 1.0, CHI2_SEED))
    print(f"chi-square of the host model {stat:.2f}")
    assert stat <= CHI2_MAX


# ===================================================================== 4.
# norms

def _silu(y):
    return y * torch.sigmoid(y)


def _gn_ref(x, gamma, beta, groups, do_silu, dtype):
    y = torch.nn.functional.group_norm(x.to(dtype), groups, gamma.to(dtype),
                                       beta.to(dtype), 1e-5)
    return _silu(y) if do_silu else y


def _ln_ref(x, gamma, beta, dtype):
    return torch.nn.functional.layer_norm(x.to(dtype), (x.shape[-1],),
                                          gamma.to(dtype), beta.to(dtype), 1e-5)


def _rms_ref(x, gamma, dtype):
    xf = x.to(dtype)
    return xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6) * gamma.to(dtype)


# (N, C, G, H, W): HW = 2304 splits in two even halves of 1152; HW = 2312
# rounds `per` up to 1160 and leaves a last slice of 1152
_GN_SHAPES = [(1, 64, 32, 48, 48), (2, 32, 8, 34, 68)]
_ROW_SHAPES = [(rows, D) for rows in (1, 5, 7) for D in (8, 64, 520, 4096)]
_OFFSETS = (0.0, 32.0)


@functools.lru_cache(maxsize=None)
def _gn_case(shape, offset=0.0):
    N, C, G, H, W = shape
    g = _gen(C * H + W + int(offset))
    x = (_randn(g, N, C, H, W) + offset).to(torch.bfloat16)
    return x, _randn(g, C), _randn(g, C)


@functools.lru_cache(maxsize=None)
def _row_case(rows, D, offset=0.0):
    g = _gen(rows * 10000 + D + int(offset))
    x = (_randn(g, rows, D) + offset).to(torch.bfloat16)
    return x, _randn(g, D), _randn(g, D)


@gpu_test
@pytest.mark.parametrize("offset", _OFFSETS)
@pytest.mark.parametrize("do_silu", [True, False])
@pytest.mark.parametrize("shape", _GN_SHAPES, ids=str)
def test_groupnorm_split_path(shape, do_silu, offset):
    """HW >= 2048: per-slice partial sums joined by atomicAdd.  offset 32 is
    the activation with a mean far from zero, where E[x^2] - mean^2 in f32
    loses digits."""
    x, gamma, beta = _gn_case(shape, offset)
    got = F.groupnorm_silu(x.cuda(), gamma.cuda(), beta.cuda(), shape[2],
                           do_silu=do_silu)
    _close_all(got, _gn_ref(x, gamma, beta, shape[2], do_silu, torch.float64),
               what=f"groupnorm{shape} silu={do_silu} offset={offset}")


@gpu_test
def test_groupnorm_unsplit_offset():
    shape = (2, 64, 32, 32, 32)  # HW = 1024: split stays 1
    x, gamma, beta = _gn_case(shape, 32.0)
    got = F.groupnorm_silu(x.cuda(), gamma.cuda(), beta.cuda(), 32)
    _close_all(got, _gn_ref(x, gamma, beta, 32, True, torch.float64),
               what="groupnorm unsplit offset=32")


def _up2(t):
    return torch.nn.functional.interpolate(t, scale_factor=2.0, mode="nearest")


@functools.lru_cache(maxsize=None)
def _conv_gn_case(shape, K=32, upsample=False, residual=False, offsets=None):
    """Inputs (CPU) and references of one fused GroupNorm+SiLU+conv call.
    `offsets` shifts image n by offsets[n], so that every image needs its own
    statistics.  beta is of order one: zero padding applied before the
    activation instead of after it would put silu(beta) != 0 on the border."""
    N, C, G, H, W = shape
    x, gamma, beta = _gn_case(shape)
    if offsets is not None:
        x = (x.float() + torch.tensor(offsets).view(N, 1, 1, 1)).bfloat16()
    g = _gen(K + C)
    w = (_randn(g, K, C, 3, 3) / math.sqrt(C * 9)).to(torch.bfloat16)
    bias = _randn(g, K)
    gamma = gamma.abs() + 0.5
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    res = _randn(g, N, K, Ho, Wo).to(torch.bfloat16) if residual else None

    def conv(h, dtype):
        y = torch.nn.functional.conv2d(_up2(h) if upsample else h, w.to(dtype),
                                       bias.to(dtype), padding=1)
        return y if res is None else y + res.to(dtype)

    want = conv(_gn_ref(x, gamma, beta, G, True, torch.float64), torch.float64)
    # f32 model of the kernel's number formats: bf16 operands into the MFMA
    h32 = _gn_ref(x, gamma, beta, G, True, torch.float32).bfloat16().float()
    return SimpleNamespace(x=x, w=w, bias=bias, gamma=gamma, beta=beta, res=res,
                           K=K, groups=G, upsample=upsample, want=want,
                           want32=conv(h32, torch.float32))


# (shape = (N, C, G, H, W) of the source, K, upsample, residual, offsets);
# HW stays a multiple of 8 (see "Out of scope" above)
_CONV_GN_EDGE_CASES = [
    ((1, 32, 8, 16, 24), 65),                     # a second k-tile of one row
    # C16 = 32: eight padded scale/shift entries per image; two images with
    # different means
    ((2, 24, 3, 16, 24), 32, False, False, (-2.0, 3.0)),
    ((1, 32, 8, 7, 24), 32, True),                # odd source, 14 x 48 output
    ((2, 24, 3, 7, 24), 65, True, True, (-2.0, 3.0)),   # all of it at once
]
_CONV_GN_CASES = [(s,) for s in _GN_SHAPES] + _CONV_GN_EDGE_CASES


def _run_conv_gn(case):
    c = _conv_gn_case(*case)
    wr = F.repack_conv3x3_weight(c.w.cuda())
    got = F.conv3x3_gn(c.x.cuda(), wr, c.bias.cuda(), c.K, c.gamma.cuda(),
                       c.beta.cuda(), groups=c.groups, raw_weight=c.w.cuda(),
                       residual=c.res.cuda() if c.res is not None else None,
                       upsample=c.upsample)
    _close_all(got, c.want, *CONV_TOL, what=f"conv3x3_gn{case}")


@gpu_test
@pytest.mark.parametrize("shape", _GN_SHAPES, ids=str)
def test_conv3x3_gn_split_stats(shape):
    """The fused GroupNorm+SiLU+conv takes its statistics from the same split
    partial kernel.  Bound: the project's 5e-2/5e-2 for the bf16 MFMA conv,
    with no excused share.  Each of the 9*C products carries a bf16 rounding
    of the normalised activation and the output one more; an f32 model with
    those roundings sits at 0.18 of this bound (CPU floor test), at 0.46 of
    2e-2/2e-2, which would leave the kernel too little room."""
    _run_conv_gn((shape,))


@gpu_test
@pytest.mark.parametrize("case", _CONV_GN_EDGE_CASES, ids=str)
def test_conv3x3_gn_edges(case):
    """K past a 64-channel block, C = 24 in three groups (padded scale and
    shift), an odd upsampled source, upsample plus residual, and two images
    whose means differ by 5, at the same bound as above."""
    _run_conv_gn(case)


@gpu_test
@pytest.mark.parametrize("offset", _OFFSETS)
@pytest.mark.parametrize("rows,D", _ROW_SHAPES)
def test_layernorm_shapes(rows, D, offset):
    """Rows no multiple of the 4-row block; D below, at and past the
    512-element wave stride."""
    x, gamma, beta = _row_case(rows, D, offset)
    got = F.layernorm(x.cuda(), gamma.cuda(), beta.cuda())
    _close_all(got, _ln_ref(x, gamma, beta, torch.float64),
               what=f"layernorm {rows}x{D} offset={offset}")


@gpu_test
@pytest.mark.parametrize("offset", _OFFSETS)
@pytest.mark.parametrize("rows,D", _ROW_SHAPES)
def test_rmsnorm_shapes(rows, D, offset):
    x, gamma, _ = _row_case(rows, D, offset)
    got = F.rmsnorm(x.cuda(), gamma.cuda())
    _close_all(got, _rms_ref(x, gamma, torch.float64),
               what=f"rmsnorm {rows}x{D} offset={offset}")


def test_comparator_floor():
    """What the number formats alone cost: the f32 reference rounded to bf16
    against the f64 reference, as a fraction of the bound, over every decode,
    norm and fused-conv case of this file.  The tolerances must sit at least
    4x above it, which leaves the kernels' fast exp and summation order
    their room.  The plain convolution is held to ROUND_TOL instead, where
    the rounding alone may take half of the bound: there the floor has to
    stay at or below 0.5 plus the f32 model's own summation error (measured:
    0.482 and 3.3e-4)."""
    def floor(want32, want64, tol):
        return float(_err_ratio(want32.bfloat16(), want64, *tol).max())

    bf16 = fp8 = conv = 0.0
    for case in _CONV_GN_EDGE_CASES:
        c = _conv_gn_case(*case)
        f = floor(c.want32, c.want, CONV_TOL)
        print(f"fused conv {case}: floor {f:.4f} of the bound")
        conv = max(conv, f)
    # plain conv at ROUND_TOL: the bf16 rounding of the f32 result may take
    # half of the bound (2^-8 over an rtol of 2^-7), beyond what the f32
    # model's own summation error, measured here, already takes
    plain = plain_sum = 0.0
    for case in _CONV_REAL_CASES:
        c = _conv_real_case(*case)
        f = floor(c.want32, c.want, ROUND_TOL)
        s = float(_err_ratio(c.want32, c.want, *ROUND_TOL).max())
        print(f"plain conv {case}: floor {f:.4f}, f32 summation {s:.2e} "
              "of the bound")
        assert f <= 0.5 + s
        plain, plain_sum = max(plain, f), max(plain_sum, s)
    print(f"comparator floor: plain conv {plain:.4f} of ROUND_TOL, "
          f"f32 summation {plain_sum:.2e}")
    for case in _DECODE_CASES:
        c = _decode_case(*case)
        if c.fp8:
            fp8 = max(fp8, floor(c.want32, c.want, FP8_TOL))
        else:
            bf16 = max(bf16, floor(c.want32, c.want, BF16_TOL))
    for shape in _GN_SHAPES:
        for offset in _OFFSETS:
            x, gamma, beta = _gn_case(shape, offset)
            for silu in (True, False):
                bf16 = max(bf16, floor(
                    _gn_ref(x, gamma, beta, shape[2], silu, torch.float32),
                    _gn_ref(x, gamma, beta, shape[2], silu, torch.float64),
                    BF16_TOL))
        c = _conv_gn_case(shape)
        conv = max(conv, floor(c.want32, c.want, CONV_TOL))
    for rows, D in _ROW_SHAPES:
        for offset in _OFFSETS:
            x, gamma, beta = _row_case(rows, D, offset)
            bf16 = max(bf16, floor(_ln_ref(x, gamma, beta, torch.float32),
                                   _ln_ref(x, gamma, beta, torch.float64),
                                   BF16_TOL))
            bf16 = max(bf16, floor(_rms_ref(x, gamma, torch.float32),
                                   _rms_ref(x, gamma, torch.float64), BF16_TOL))
    print(f"comparator floor: bf16 {bf16:.4f}, fp8 cache {fp8:.4f}, "
          f"fused conv {conv:.4f} of the bound")
    assert 4.0 * max(bf16, fp8, conv) <= 1.0


# ===================================================================== 5.
# RoPE, elementwise, softmax, AdamW

def _rope_ref64(x, cos, sin, pos):
    """x [B,H,S,D]; pos [B,S] long; rotate-half, float64."""
    D = x.shape[-1]
    c = cos.double()[pos][:, None]  # [B,1,S,D/2]
    s = sin.double()[pos][:, None]
    x1, x2 = x.double()[..., : D // 2], x.double()[..., D // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


@gpu_test
@pytest.mark.parametrize("D", [64, 128])
def test_rope_per_sequence_positions_in_place(D):
    """[B*S] positions that differ per batch row, rotating the q slice of a
    fused [B,S,3,H,D] projection in place through its transposed view: q is
    the reference, k and v keep their bits."""
    B, H, S = 3, 2, 5
    qkv = _randn(_gen(D), B, S, 3, H, D).to(torch.bfloat16)
    cos, sin = F.rope_tables(128, D)
    pos = (torch.tensor([0, 7, 100])[:, None] + torch.arange(S)[None, :])
    want = _rope_ref64(qkv[:, :, 0].transpose(1, 2), cos, sin, pos)
    dev = qkv.cuda()
    qview = dev[:, :, 0].transpose(1, 2)
    assert not qview.is_contiguous()
    out = F.rope(qview, cos.cuda(), sin.cuda(),
                 positions=pos.reshape(-1).int().cuda(), inplace=True)
    assert out.data_ptr() == qview.data_ptr()
    _close_all(dev[:, :, 0].transpose(1, 2), want, *ROUND_TOL, what=f"rope D={D}")
    back = dev.cpu()
    assert torch.equal(back[:, :, 1:].view(torch.int16),
                       qkv[:, :, 1:].view(torch.int16)), "k or v changed"


@gpu_test
def test_rope_grid_stride_rows():
    """More than 16384 rows: the grid is capped at 4096 blocks of 4 rows and
    every wave walks several rows."""
    B, H, S, D = 1, 8, 2304, 64
    x = _randn(_gen(3), B, H, S, D).to(torch.bfloat16)
    cos, sin = F.rope_tables(S, D)
    want = _rope_ref64(x, cos, sin, torch.arange(S)[None, :])
    _close_all(F.rope(x.cuda(), cos.cuda(), sin.cuda()), want, *ROUND_TOL,
               what="rope grid-stride")


def _gelu_tanh(a):
    return torch.nn.functional.gelu(a, approximate="tanh")


@gpu_test
@pytest.mark.parametrize("n", [5, 8 * 1000 + 3])
def test_elementwise_tails(n):
    """n below one vector and n = 8k + 3: the scalar tail after the bf16x8
    body, in every elementwise kernel."""
    g = _gen(n)
    a, b, c = (_randn(g, n).to(torch.bfloat16) for _ in range(3))
    ad, bd, cd = a.double(), b.double(), c.double()
    ac, bc, cc = a.cuda(), b.cuda(), c.cuda()
    _close_all(F.silu_mul(ac, bc), _silu(ad) * bd, *ROUND_TOL, what="silu_mul")
    _close_all(F.geglu(ac, bc), _gelu_tanh(ad) * bd, *ROUND_TOL, what="geglu")
    _close_all(F.add_residual(ac, bc), ad + bd, *ROUND_TOL, what="add_residual")
    _close_all(F.cfg_euler(ac, bc, cc, 7.5, -0.3),
               ad - 0.3 * (cd + 7.5 * (bd - cd)), *ROUND_TOL, what="cfg_euler")
    _close_all(F.cfg_euler(ac, bc, None, 0.0, -0.3), ad - 0.3 * bd, *ROUND_TOL,
               what="cfg_euler no uncond")


@gpu_test
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("rows,inner", [(1, 8), (3, 24)])
def test_glu_fused_small(rows, inner, gelu):
    src = _randn(_gen(rows + inner), rows, 2 * inner).to(torch.bfloat16)
    a, b = src[:, :inner].double(), src[:, inner:].double()
    want = (_gelu_tanh(a) if gelu else _silu(a)) * b
    _close_all(F.glu_fused(src.cuda(), gelu=gelu), want, *ROUND_TOL,
               what=f"glu_fused {rows}x{inner}")


@gpu_test
def test_adamw_bf16_ragged():
    """bf16 parameters at n = 4099 against a float64 AdamW step."""
    n, lr, b1, b2, eps, wd = 4099, 1e-2, 0.9, 0.999, 1e-8, 0.01
    g = _gen(14)
    p = _randn(g, n).to(torch.bfloat16)
    gr = _randn(g, n).to(torch.bfloat16)
    m, v = _randn(g, n) * 0.1, _randn(g, n).abs() * 0.1
    pd, gd = p.double(), gr.double()
    m2 = b1 * m.double() + (1 - b1) * gd
    v2 = b2 * v.double() + (1 - b2) * gd * gd
    step = 3
    upd = (m2 / (1 - b1 ** step)) / ((v2 / (1 - b2 ** step)).sqrt() + eps)
    want = pd - lr * (upd + wd * pd)
    pc, mc, vc = p.cuda(), m.cuda(), v.cuda()
    F.adamw_step(pc, gr.cuda(), mc, vc, lr=lr, step=step)
    _close_all(pc, want, *ROUND_TOL, what="adamw p")
    # f32 moments; the kernel forms 1 - beta2 in f32, where 2^-25 of
    # rounding in 0.999f is 3e-5 of the 1e-3 that is left
    _close_all(mc, m2, 1e-7, 1e-5, what="adamw m")
    _close_all(vc, v2, 1e-7, 1e-4, what="adamw v")


@gpu_test
@pytest.mark.parametrize("V", [1, 255, 257])
def test_softmax_edge_rows(V):
    """Against torch.softmax in float64 at the project's 1e-6 / 1e-4: V
    below and past the 256-thread block, a row with -inf, a row near +-1e4
    and a constant row."""
    g = _gen(V)
    x = _randn(g, 5, V)
    if V > 1:
        x[1, torch.rand(V, generator=g) < 0.3] = float("-inf")
        x[1, V // 2] = 0.5
    x[2] = _randn(g, V) + torch.where(torch.arange(V) % 3 == 0, 1e4, -1e4)
    x[3] = 3.0
    x[4] = _randn(g, V) - 1e4
    want = torch.softmax(x.double(), -1)
    assert torch.isfinite(want).all()
    _close_all(F.softmax(x.cuda()), want, 1e-6, 1e-4, what=f"softmax V={V}")


# ===================================================================== 6.
# 3x3 convolution
#
# The tile is 64 output channels x 8 rows x 32 columns (16 rows in the
# 4-rows-per-wave variant), the input channels go in 16-channel chunks of two
# octets, and the workgroups of one image are renumbered across the 8 XCDs.

def _exact(got, want64, what=""):
    """Every element equal to the float64 reference; nothing excused."""
    g = got.detach().float().cpu()
    w = want64.float()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if torch.equal(g, w):
        return
    diff = g != w  # true for NaN as well
    n, k, y, x = diff.nonzero()[0].tolist()
    raise AssertionError(
        f"{what}: {int(diff.sum())} of {diff.numel()} elements differ, first "
        f"at (n={n}, k={k}, y={y}, x={x}): got {float(g[n, k, y, x])}, want "
        f"{float(w[n, k, y, x])}")


@functools.lru_cache(maxsize=None)
def _conv_exact_case(N, C, K, H, W, upsample=False, residual=False):
    """Small-integer operands (CPU): x in [-2, 2], w in {-1, 0, 1}, bias and
    residual in [-8, 8].  Every product and every f32 partial sum is an
    integer far below 2^24, so the order of the MFMA sums does not matter,
    and while |want| <= 256 the final bf16 rounding is the identity: kernel
    and reference agree in every element or the kernel is wrong.  Past
    C = 80 only 80/C of the weights are non-zero, which keeps |want| there.
    H, W are the source's; the output is twice that with upsample."""
    g = _gen(((((N * 401 + C) * 401 + K) * 401 + H) * 401 + W) * 4
             + 2 * upsample + residual)
    x = torch.randint(-2, 3, (N, C, H, W), generator=g).to(torch.bfloat16)
    w = torch.randint(-1, 2, (K, C, 3, 3), generator=g).float()
    if C > 80:
        w *= torch.rand(K, C, 3, 3, generator=g) < 80.0 / C
    w = w.to(torch.bfloat16)
    bias = torch.randint(-8, 9, (K,), generator=g).float()
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    res = (torch.randint(-8, 9, (N, K, Ho, Wo), generator=g).to(torch.bfloat16)
           if residual else None)
    xin = _up2(x.double()) if upsample else x.double()
    want = torch.nn.functional.conv2d(xin, w.double(), bias.double(), padding=1)
    if res is not None:
        want = want + res.double()
    return SimpleNamespace(x=x, w=w, bias=bias, res=res, K=K,
                           upsample=upsample, want=want)


_CONV_WS = (1, 2, 31, 32, 33, 64, 65)
_CONV_C_TAILS = [(2, C, 8, 9, 33) for C in (1, 3, 4, 8, 9, 16, 17, 24, 40, 80)]
_CONV_K_TAILS = [(1, 16, K, 9, 33) for K in (1, 3, 31, 32, 33, 64, 65, 96, 129)]
# all padding, one short of, at and one past a tile, seams both ways; every
# one a single launch, those of one tile per k-tile fewer than 8 workgroups
_CONV_SPATIAL = [(1, 16, 8, H, W) for H in (1, 2, 7, 8, 9, 16, 17)
                 for W in _CONV_WS]
# the same edges of the 16-row tile of the 4-rows-per-wave variant
_CONV_SPATIAL_RPW4 = [(1, 16, 8, H, W) for H in (15, 16, 17, 32, 33)
                      for W in _CONV_WS]
# nwg = npix * nk from 9 to 15: every remainder of the XCD renumbering but 0
_CONV_SWIZZLE = [(3, 16, 64 * c, 8 * a, 32 * b) for a, b, c in
                 ((3, 3, 1), (5, 2, 1), (11, 1, 1), (3, 2, 2), (13, 1, 1),
                  (7, 2, 1), (5, 1, 3))]
_CONV_DEEP = [(1, 320, 64, 16, 32)]
# odd sources; x0 - 1 and x0 of the second tile column share a source column
_CONV_UP = [(2, 24, 40, 5, 17, True, r) for r in (False, True)] + \
           [(1, 16, 8, 9, 33, True, r) for r in (False, True)]
_CONV_RES = [(2, 17, 65, 9, 33, False, True)]
_CONV_EXACT_GROUPS = {
    "channel tails": _CONV_C_TAILS, "output-channel tails": _CONV_K_TAILS,
    "spatial edges": _CONV_SPATIAL, "spatial edges, 16-row tile":
    _CONV_SPATIAL_RPW4, "swizzle": _CONV_SWIZZLE, "deep C": _CONV_DEEP,
    "upsample": _CONV_UP, "residual": _CONV_RES}
_LEAK_CASE = (2, 3, 8, 9, 33)
_LAYOUT_CASE = _CONV_RES[0]
# the valid arguments that the rejection test spoils one at a time; HW is a
# multiple of 8 so that they are valid for the GroupNorm entry as well
_ARG_CASE = (2, 17, 65, 8, 33, False, True)


def _conv_exact_out(case, x=None, res=None):
    """F.conv3x3 on an exact case; x and res may be given in another layout."""
    c = _conv_exact_case(*case)
    wd = c.w.cuda()
    if res is None and c.res is not None:
        res = c.res.cuda()
    return F.conv3x3(c.x.cuda() if x is None else x,
                     F.repack_conv3x3_weight(wd), c.bias.cuda(), c.K,
                     residual=res, raw_weight=wd, upsample=c.upsample)


def _run_conv_exact(case):
    _exact(_conv_exact_out(case), _conv_exact_case(*case).want,
           what=f"conv3x3{case}")


@gpu_test
@pytest.mark.parametrize("case", _CONV_C_TAILS, ids=str)
def test_conv3x3_exact_channel_tails(case):
    """C = 1, 3, 4: a partial first octet; 9: one channel in the second
    octet; 17: one channel in a second chunk; 24: a second chunk with an
    empty second octet; 80: five chunks, so the prefetch loop has iterations
    that are neither its first nor its last."""
    _run_conv_exact(case)


@gpu_test
@pytest.mark.parametrize("case", _CONV_K_TAILS, ids=str)
def test_conv3x3_exact_output_channel_tails(case):
    """The k < K store mask inside a 32-channel fragment, the tail of a
    64-channel block, and a third k-tile."""
    _run_conv_exact(case)


@gpu_test
@pytest.mark.parametrize("case", _CONV_SPATIAL + _CONV_SPATIAL_RPW4, ids=str)
def test_conv3x3_exact_spatial_edges(case):
    _run_conv_exact(case)


@gpu_test
@pytest.mark.parametrize("case", _CONV_SWIZZLE, ids=str)
def test_conv3x3_exact_xcd_swizzle(case):
    """Workgroup counts 9 to 15 per image, over pixel tiles and k-tiles, in
    three images (blockIdx.y)."""
    _run_conv_exact(case)


@gpu_test
@pytest.mark.parametrize("case", _CONV_DEEP + _CONV_UP + _CONV_RES, ids=str)
def test_conv3x3_exact_deep_upsample_residual(case):
    _run_conv_exact(case)


@gpu_test
def test_conv3x3_masked_channels_do_not_leak():
    """C = 3 of a 16-channel chunk: the 13 padded channels of image 0 are, in
    memory, the channels of image 1, here NaN.  Their weights are zero, but
    NaN * 0 is NaN: image 0 stays exact only if those loads are masked."""
    c = _conv_exact_case(*_LEAK_CASE)
    x = c.x.clone()
    x[1] = float("nan")
    out = _conv_exact_out(_LEAK_CASE, x=x.cuda())
    _exact(out[:1], c.want[:1], what="image 0 beside a NaN image")
    assert torch.isnan(out[1]).all(), "image 1 is NaN in every input"


@gpu_test
def test_conv3x3_layout_dispatch():
    """Contiguous, channels_last and a channel slice of a wider tensor give
    the same bits, as does a residual that is a slice."""
    N, C, K, H, W = _LAYOUT_CASE[:5]
    c = _conv_exact_case(*_LAYOUT_CASE)
    xd, rd = c.x.cuda(), c.res.cuda()
    big = torch.full((N, C + 3, H, W), float("nan"), dtype=torch.bfloat16,
                     device="cuda")
    big[:, 1:1 + C] = xd
    rbig = torch.full((N, K, H, W + 2), float("nan"), dtype=torch.bfloat16,
                      device="cuda")
    rbig[..., 1:1 + W] = rd
    cl = xd.to(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and not big[:, 1:1 + C].is_contiguous()
    assert not rbig[..., 1:1 + W].is_contiguous()
    for what, x, r in (("contiguous", xd, rd), ("channels_last", cl, rd),
                       ("channel slice", big[:, 1:1 + C], rd),
                       ("residual slice", xd, rbig[..., 1:1 + W])):
        _exact(_conv_exact_out(_LAYOUT_CASE, x=x, res=r), c.want, what=what)


@functools.lru_cache(maxsize=None)
def _conv_real_case(N, C, K, H, W, upsample=False, residual=False):
    """Random bf16 x and w / sqrt(9C), f32 bias: outputs of about unit
    variance, against float64 and an f32 model of the same bf16 operands."""
    g = _gen(((((N * 401 + C) * 401 + K) * 401 + H) * 401 + W) * 4
             + 2 * upsample + residual + 1_000_000_007)
    x = _randn(g, N, C, H, W).to(torch.bfloat16)
    w = (_randn(g, K, C, 3, 3) / math.sqrt(9 * C)).to(torch.bfloat16)
    bias = _randn(g, K)
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    res = _randn(g, N, K, Ho, Wo).to(torch.bfloat16) if residual else None

    def conv(dtype):
        xin = _up2(x.to(dtype)) if upsample else x.to(dtype)
        y = torch.nn.functional.conv2d(xin, w.to(dtype), bias.to(dtype),
                                       padding=1)
        return y if res is None else y + res.to(dtype)

    return SimpleNamespace(x=x, w=w, bias=bias, res=res, K=K,
                           upsample=upsample, want=conv(torch.float64),
                           want32=conv(torch.float32))


_CONV_REAL_CASES = [(2, 64, 64, 16, 32), (1, 96, 64, 19, 45),
                    (2, 4, 320, 16, 32), (1, 128, 3, 24, 32),
                    (2, 32, 48, 12, 16, False, True),
                    (2, 32, 48, 12, 16, True, False),
                    (2, 32, 48, 12, 16, True, True)]


@gpu_test
@pytest.mark.parametrize("case", _CONV_REAL_CASES, ids=str)
def test_conv3x3_real_valued(case):
    """ROUND_TOL is derived, not measured: against the float64 reference of
    the same bf16 operands the kernel may differ by the order of its f32
    sums, absolute and far below atol (the f32 model's own is 3.3e-4 of the
    bound, CPU floor test), and by the one bf16 rounding of its result, at
    most 2^-8 relative, half of rtol."""
    c = _conv_real_case(*case)
    wd = c.w.cuda()
    got = F.conv3x3(c.x.cuda(), F.repack_conv3x3_weight(wd), c.bias.cuda(),
                    c.K, residual=c.res.cuda() if c.res is not None else None,
                    raw_weight=wd, upsample=c.upsample)
    _close_all(got, c.want, *ROUND_TOL, what=f"conv3x3 real{case}")


# ---- argument checks of the two bindings

def _conv_bad_arguments(gn):
    """(match, changed arguments) for every argument the bindings reject."""
    c = _conv_exact_case(*_ARG_CASE)               # C = 17, K = 65
    x, bias, res = c.x.cuda(), c.bias.cuda(), c.res.cuda()
    wr = F.repack_conv3x3_weight(c.w.cuda())       # [9, 128, 32]
    vec = torch.ones(17, device="cuda")
    good = dict(x=x, wr=wr, bias=bias, residual=res, K=65, upsample=False,
                gamma=vec, beta=vec, groups=1, eps=1e-5)
    wide = torch.ones(2 * 65, device="cuda")
    bad = [
        ("bias must be on GPU", dict(bias=bias.cpu())),
        ("bias must be fp32", dict(bias=bias.double())),
        ("bias must be contiguous", dict(bias=wide[::2])),
        ("bias must have K", dict(bias=bias[:64])),
        ("bias must have K", dict(bias=wide)),
        ("K must be at least 1", dict(K=0, bias=bias[:0], residual=None)),
        ("wr must be", dict(wr=wr[:8].contiguous())),
        ("wr must be", dict(wr=wr[0])),
        ("Kpad % 64", dict(wr=wr[:, :96].contiguous())),
        ("C16 % 16", dict(wr=wr[:, :, :24].contiguous())),
        ("weight pack smaller", dict(wr=wr[:, :64].contiguous())),
        ("weight pack smaller", dict(wr=wr[:, :, :16].contiguous())),
        ("x must be NCHW", dict(x=x[0], residual=None)),
        ("residual shape", dict(residual=res[:, :, :-1].contiguous())),
        ("residual shape", dict(residual=res[:1])),
    ]
    if gn:
        wide = torch.ones(34, device="cuda")
        for name in ("gamma", "beta"):
            bad += [
                (f"{name} must be on GPU", {name: vec.cpu()}),
                (f"{name} must be fp32", {name: vec.double()}),
                (f"{name} must be contiguous", {name: wide[::2]}),
                (f"{name} must have C", {name: vec[:16]}),
            ]
        bad += [("groups", dict(groups=0)), ("groups", dict(groups=-1)),
                ("groups", dict(groups=4)), ("groups", dict(groups=34))]
    return good, bad


@gpu_test
@pytest.mark.parametrize("gn", [False, True], ids=["conv3x3", "conv3x3_gn"])
def test_conv3x3_bindings_reject_bad_arguments(gn):
    """Each bad argument raises on the host, naming the argument, before
    anything is launched; a valid call afterwards is exact."""
    from modal_examples_amd.ops._build import get_ext

    ext = get_ext(required=True)
    names = ["x", "wr", "bias", "residual", "K", "upsample"]
    if gn:
        names += ["gamma", "beta", "groups", "eps"]
    entry = ext.conv3x3_gn if gn else ext.conv3x3
    good, bad = _conv_bad_arguments(gn)
    for match, changed in bad:
        args = [changed.get(n, good[n]) for n in names]
        with pytest.raises(RuntimeError, match=match):
            entry(*args)
    torch.cuda.synchronize()
    if gn:
        _run_conv_gn(_CONV_GN_EDGE_CASES[-1])
    _run_conv_exact(_ARG_CASE)


# ---- the Conv3x3 module

@gpu_test
@pytest.mark.parametrize("case", [_CONV_C_TAILS[6], _CONV_RES[0], _CONV_UP[0]],
                         ids=["plain", "residual", "upsample"])
def test_conv3x3_module_follows_bias_update(case):
    """The module in eval mode, bf16, with integer parameters: exact, and
    exact again after an in-place bias update that leaves the weight alone
    (the repacked weight and the f32 bias are cached together)."""
    from modal_examples_amd.models.sdxl.layers import Conv3x3

    c = _conv_exact_case(*case)
    m = Conv3x3(case[1], case[2]).to(torch.bfloat16).cuda().eval()
    x = c.x.cuda()
    res = c.res.cuda() if c.res is not None else None
    with torch.no_grad():
        m.weight.copy_(c.w)
        m.bias.copy_(c.bias)
        assert m._use_kernel(x)
        _exact(m(x, residual=res, upsample=c.upsample), c.want, "module")
        m.bias.add_(1)
        want = c.want + 1
        assert torch.equal(want.bfloat16().double(), want)
        _exact(m(x, residual=res, upsample=c.upsample), want,
               "module after bias.add_(1)")


# ---- the 4-rows-per-wave variant, in a process of its own

_RPW4_CASES = (_CONV_SPATIAL_RPW4 + _CONV_C_TAILS + [_CONV_UP[1]])
_RPW4_GN_CASE = _CONV_GN_EDGE_CASES[-1]
_RPW4_TIMEOUT = 120.0


def _rpw_cases_main():
    """Runs the variant's cases and prints what they took."""
    import time

    torch.cuda.init()
    t0 = time.perf_counter()
    for case in _RPW4_CASES:
        _run_conv_exact(case)
    _run_conv_gn(_RPW4_GN_CASE)
    torch.cuda.synchronize()
    print(f"{len(_RPW4_CASES) + 1} conv cases with MODAL_AMD_CONV_RPW="
          f"{os.environ.get('MODAL_AMD_CONV_RPW')}: "
          f"{time.perf_counter() - t0:.2f} s")


@gpu_test
def test_conv3x3_four_rows_per_wave_variant():
    """MODAL_AMD_CONV_RPW=4 is read once per process, so the variant runs in
    one fresh child: the exact spatial cases around its 16-row tile, the
    channel tails, upsample plus residual, and one GroupNorm case.  Measured:
    the same 47 cases take 0.16 s in this process, and 0.16 s in the child,
    which takes 2.8 s in all with its start; the limit is 120 s, 40 times
    that, so that only a hang reaches it."""
    import subprocess
    import sys

    tests_dir = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MODAL_AMD_CONV_RPW="4")
    code = ("import sys; sys.path[:0] = [%r, %r]; "
            "import test_kernel_edges_gpu as t; t._rpw_cases_main()"
            % (os.path.dirname(tests_dir), tests_dir))
    r = subprocess.run([sys.executable, "-c", code], env=env,
                       timeout=_RPW4_TIMEOUT, capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (f"child exited with {r.returncode}\n"
                               f"{r.stdout[-4000:]}\n{r.stderr[-8000:]}")
    assert "MODAL_AMD_CONV_RPW=4" in r.stdout


# ---- the convolution's CPU condition (unmarked: it needs no GPU)

def test_conv3x3_exact_cases_are_exact_in_bf16():
    """The condition of every exact case above: the float64 reference is
    itself a bf16 value (an integer of magnitude at most 256), so that the
    kernel's final rounding cannot excuse anything."""
    for name, cases in _CONV_EXACT_GROUPS.items():
        top = 0.0
        for case in cases + ([_LEAK_CASE] if name == "channel tails" else []):
            want = _conv_exact_case(*case).want
            assert torch.equal(want.bfloat16().double(), want), (name, case)
            assert torch.equal(want, want.round())
            top = max(top, float(want.abs().max()))
        print(f"exact conv cases, {name}: largest |want| {top:.0f}")
        assert top <= 256
    for case in (_CONV_C_TAILS[6], _CONV_RES[0], _CONV_UP[0]):  # module test
        want = _conv_exact_case(*case).want + 1
        assert torch.equal(want.bfloat16().double(), want)
    want = _conv_exact_case(*_ARG_CASE).want
    assert torch.equal(want.bfloat16().double(), want)
