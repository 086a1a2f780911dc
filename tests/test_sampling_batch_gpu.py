"""Per-row filtered sampling (`F.sampling_cutoff`, `F.sample_batch`) against
float64 models, following the conventions of `test_kernel_edges_gpu.py`.

The kept set of a row is `{i : logit_i >= c_r}`.  The cutoff `c_r` is checked
against `ops.reference.sampling_cutoff_ref` (float64, itself checked below
against a plain per-row loop): exactly where only top-k is on (pure ordering),
and otherwise by a sandwich

    c_ref(p + CUT_DELTA, q (1 - CUT_DELTA)) <= c_gpu <= c_ref(p - CUT_DELTA, q (1 + CUT_DELTA))

with `c_gpu` an element of its row (or -inf).  Nothing is excused.  Tokens
are checked against a host model of the draw: Gumbel scores from the row's
own (seed, counter), masked to `logit >= c_gpu`; the pick must score within
`DELTA` of the best, and picks that differ from the model's arg-max (near-
ties) are capped at 1 % per test.

GPU tests are marked one by one; the host-model tests are unmarked and run
with the CPU suite.

Figures this file relies on (measured on the CPU by the unmarked tests below,
which print them and assert the stated relation):

* The kernel forms e_i = exp(logit_i * f32(1/T) - m) in float32 and sums
  trunc(e_i * 2^32) in 64-bit integers.  A numpy emulation of exactly that,
  against float64, over rows = 5 of every V and parameter set here: mass
  fractions (mass above a token / Z_K) differ by 1.35e-7 at most and e_i, the
  min-p quantity, by 9.4e-7 relative (where e_i >= 1e-3).  100x the larger
  is 9.4e-5; CUT_DELTA = 1e-4, below the 1e-3 the sandwich may use.
* Share of draws whose float64 top-two gap inside the reference's kept set
  is below DELTA (rows = 8, V in {1000, 4099}, the four filter sets, seeds
  1..64): 3 of 4096, 0.07 %; the cap is 1 %.
* Host-model chi-square of the V = 16 case with top_k = 4 (4096 rows under
  seed 1234, counters 0..4095, T = 1), against the distribution renormalised
  over the four largest: 1.00; the threshold is 30.7 (1e-6 quantile, 3 d.o.f.).
"""
import functools

import numpy as np
import pytest
import torch

import modal_examples_amd.ops.functional as F
from modal_examples_amd.ops import reference as ref
from test_kernel_edges_gpu import (DELTA, _chi2_logits, _gen, _hash3, _randn,
                                   gumbel_scores)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def gpu_test(fn):
    return pytest.mark.gpu(requires_gpu(fn))


CUT_DELTA = 1e-4
VOCABS = (1, 255, 1025, 4099, 32003)
# (top_k, top_p, min_p, temperature)
PARAM_SETS = ((0, .9, 0., 1.), (50, 1., 0., .7), (40, .8, .02, 1.),
              (0, 1., .05, 2.5))
SEEDS = (0, 1, 2 ** 32 + 3, -12345)
NEG_INF = float("-inf")


# ------------------------------------------------------------ host models

def _i64(seed):
    return int(seed) & (1 << 64) - 1


def row_scores(logits, temps, seeds, counters):
    """float64 scores logit * f32(1/T) + G(seed, counter, i) with a seed and
    a counter per row, the uniform formed in float32 as the kernel does."""
    lg = np.asarray(logits, dtype=np.float32)
    rows, V = lg.shape
    temps = np.broadcast_to(np.asarray(temps, dtype=np.float32), (rows,))
    seeds = [_i64(s) for s in np.broadcast_to(np.asarray(seeds, dtype=object), (rows,))]
    counters = np.broadcast_to(np.asarray(counters, dtype=np.int64), (rows,))
    lo = np.array([s & 0xFFFFFFFF for s in seeds], dtype=np.uint64)[:, None]
    hi = np.array([(s >> 32) ^ (int(c) & 0xFFFFFFFF)
                   for s, c in zip(seeds, counters)], dtype=np.uint64)[:, None]
    u = _hash3(lo, hi, np.arange(V, dtype=np.uint64)[None, :])
    uf = ((u >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
          + np.float32(1e-10))
    inv_t = (np.float32(1.0) / temps).astype(np.float64)[:, None]
    return lg.astype(np.float64) * inv_t - np.log(-np.log(uf.astype(np.float64)))


def _params(rows, k, p, q, T):
    return (torch.full((rows,), T, dtype=torch.float32),
            torch.full((rows,), k, dtype=torch.int32),
            torch.full((rows,), p, dtype=torch.float32),
            torch.full((rows,), q, dtype=torch.float32))


def cutoff_ref(logits, k, p, q, T):
    t, kk, pp, qq = _params(logits.shape[0], k, min(p, 1.0), q, T)
    return ref.sampling_cutoff_ref(logits, t, kk, pp, qq).numpy()


def cutoff_band(logits, k, p, q, T):
    """(lower, upper) reference cutoffs of the sandwich."""
    if p >= 1 and q <= 0:
        c = cutoff_ref(logits, k, p, q, T)
        return c, c
    p_lo, p_hi = (p, p) if p >= 1 else (p - CUT_DELTA, p + CUT_DELTA)
    return (cutoff_ref(logits, k, p_hi, q * (1 - CUT_DELTA), T),
            cutoff_ref(logits, k, p_lo, q * (1 + CUT_DELTA), T))


def cutoff_loop(row, k, p, q, T):
    """The specification, one row at a time in plain numpy float64."""
    x = np.asarray(row, dtype=np.float64)
    V = len(x)
    fin = x > NEG_INF
    if T <= 0 or not ((0 < k < V) or p < 1 or q > 0):
        return NEG_INF
    inv = np.float64(np.float32(T))
    c_k = NEG_INF
    if 0 < k < V:
        c_k = np.sort(x[fin])[::-1][min(k, fin.sum()) - 1]
    in_k = fin & (x >= c_k)
    e = np.where(fin, np.exp(x / inv - x.max() / inv), 0.0)
    kept = in_k.copy()
    if p < 1:
        z = e[in_k].sum()
        for i in np.nonzero(in_k)[0]:
            kept[i] = e[in_k & (x > x[i])].sum() <= np.float64(np.float32(p)) * z
    if q > 0:
        kept &= e >= np.float64(np.float32(q))
    return x[kept].min()


def _emulated_mass(x32, inv_t32):
    """The kernel's e_i and fixed-point mass in numpy: float32 multiply,
    subtract and exp, then trunc(e * 2^32) as an exact integer in float64."""
    s = (x32 * inv_t32).astype(np.float32)
    e = np.exp((s - s.max()).astype(np.float32)).astype(np.float32)
    return e, np.floor(e.astype(np.float64) * 4294967296.0)


# ------------------------------------------------------------ GPU checks

def _check_cutoff(logits, k, p, q, T, c_gpu):
    lg = logits.numpy()
    lo, hi = cutoff_band(logits, k, p, q, T)
    assert c_gpu.shape == lo.shape and c_gpu.dtype == np.float32
    in_row = (lg == c_gpu[:, None]).any(-1) | (c_gpu == NEG_INF)
    assert in_row.all(), f"cutoff not a row element: rows {np.nonzero(~in_row)[0][:8]}"
    bad = ~((lo <= c_gpu) & (c_gpu <= hi))
    assert not bad.any(), (
        f"rows {np.nonzero(bad)[0][:8]}: cutoff {c_gpu[bad][:4]} outside "
        f"[{lo[bad][:4]}, {hi[bad][:4]}] (k={k} p={p} q={q} T={T} V={lg.shape[1]})")
    if p >= 1 and q <= 0:
        assert (c_gpu == lo).all()  # top-k alone: exact


def _check_tokens(logits, temps, seeds, counters, c_gpu, tok):
    """Returns (excused, rows) as `_check_sample` of the edges file does."""
    lg = logits.numpy()
    rows = lg.shape[0]
    temps = np.broadcast_to(np.asarray(temps, dtype=np.float32), (rows,))
    tok = tok.astype(np.int64)
    assert tok.shape == (rows,) and ((tok >= 0) & (tok < lg.shape[1])).all(), tok
    live = temps > 0
    want_greedy = lg.argmax(-1)
    assert (tok[~live] == want_greedy[~live]).all()
    scores = row_scores(lg, np.where(live, temps, 1.0), seeds, counters)
    scores = np.where(lg >= c_gpu[:, None], scores, NEG_INF)
    picked = scores[np.arange(rows), tok]
    gap = (scores.max(-1) - picked)[live]
    assert np.isfinite(picked[live]).all(), "sampled a token outside the kept set"
    assert (gap <= DELTA).all(), f"pick scores {gap.max():.4g} below the model's best"
    return int((tok != scores.argmax(-1))[live].sum()), int(live.sum())


def _run(logits, k, p, q, T, seeds, counters):
    x = logits.cuda()
    c = F.sampling_cutoff(x, T, top_k=k, top_p=p, min_p=q).cpu().numpy()
    tok = F.sample_batch(x, T, top_k=k, top_p=p, min_p=q, seeds=seeds,
                         counters=counters).cpu().numpy()
    return c, tok


@gpu_test
@pytest.mark.parametrize("V", VOCABS)
def test_cutoff_and_token_match_host_models(V):
    """rows 1 and 5 split the vocabulary in the draw kernel, rows = 600 does
    not.  Every parameter set meets every row count."""
    g = _gen(1000 + V)
    excused = total = 0
    for rows in (1, 5):
        logits = 2.0 * _randn(g, rows, V)
        for j, (k, p, q, T) in enumerate(PARAM_SETS):
            seeds = torch.tensor([SEEDS[(j + r) % 4] for r in range(rows)])
            counters = torch.arange(rows) * 7 + j
            c, tok = _run(logits, k, p, q, T, seeds.cuda(), counters.cuda())
            _check_cutoff(logits, k, p, q, T, c)
            e, n = _check_tokens(logits, T, seeds.tolist(), counters.numpy(), c, tok)
            excused, total = excused + e, total + n
    logits = 2.0 * _randn(g, 600, V)
    for j, (k, p, q, T) in enumerate(PARAM_SETS):
        counters = torch.arange(600) % 13 + j
        c, tok = _run(logits, k, p, q, T, SEEDS[j], counters.cuda())
        _check_cutoff(logits, k, p, q, T, c)
        e, n = _check_tokens(logits, T, SEEDS[j], counters.numpy(), c, tok)
        excused, total = excused + e, total + n
    print(f"V={V}: {excused} of {total} picks excused as near-ties")
    assert excused <= 0.01 * total


@gpu_test
def test_mixed_rows_in_one_call():
    """Greedy, unfiltered and filtered rows side by side, each with its own
    parameters."""
    V, rows = 4099, 12
    logits = 2.0 * _randn(_gen(12), rows, V)
    sets = [(0, 1., 0., 0.), (0, 1., 0., 1.), (40, .8, .02, 1.), (0, .9, 0., 1.),
            (50, 1., 0., .7), (7, .5, 0., 0.)] * 2
    k, p, q, T = (torch.tensor(col) for col in zip(*sets))
    seeds = torch.arange(rows) * 1000003 - 5
    counters = torch.arange(rows) + 3
    x = logits.cuda()
    c = F.sampling_cutoff(x, T.cuda(), k.cuda(), p.cuda(), q.cuda()).cpu().numpy()
    tok = F.sample_batch(x, T.cuda(), k.cuda(), p.cuda(), q.cuda(),
                         seeds.cuda(), counters.cuda()).cpu().numpy()
    for r, (kk, pp, qq, tt) in enumerate(sets):
        if tt <= 0 or (kk == 0 and pp >= 1 and qq <= 0):
            assert c[r] == NEG_INF
        else:
            _check_cutoff(logits[r:r + 1], kk, pp, qq, tt, c[r:r + 1])
    excused, total = _check_tokens(logits, T.numpy(), seeds.tolist(),
                                   counters.numpy(), c, tok)
    assert excused == 0 and total == 8, (excused, total)


@gpu_test
@pytest.mark.parametrize("V", VOCABS)
def test_unfiltered_equals_sample(V):
    """With the filters off and counter = row, sample_batch IS sample."""
    g = _gen(2000 + V)
    for rows in (1, 5, 600):
        x = (2.0 * _randn(g, rows, V)).cuda()
        ctr = torch.arange(rows, device="cuda")
        for j, seed in enumerate(SEEDS):
            T = (0.7, 1.0, 2.5)[(j + rows) % 3]
            want = F.sample(x, T, seed=seed)
            got = F.sample_batch(x, T, seeds=seed, counters=ctr)
            assert torch.equal(got, want), (V, rows, seed)
            assert torch.equal(F.sample_batch(x, T, seeds=seed), want)
        assert torch.equal(F.sample_batch(x, 0.0), F.sample(x, 0.0, seed=3))


@gpu_test
@pytest.mark.parametrize("V", [4099, 32003])
def test_row_result_independent_of_batch(V):
    """A row's cutoff and, for equal (seed, counter), its token do not depend
    on the row's index, the batch around it or the launch."""
    g = _gen(3000 + V)
    row = 2.0 * _randn(g, 1, V)
    k, p, q, T = 40, .8, .02, 1.
    kw = dict(top_k=k, top_p=p, min_p=q)
    c1 = F.sampling_cutoff(row.cuda(), T, **kw).cpu()
    t1 = F.sample_batch(row.cuda(), T, seeds=5, counters=9, **kw).cpu()
    # top-p alone reads the whole row's mass
    cp1 = F.sampling_cutoff(row.cuda(), T, top_p=.9).cpu()
    rep = row.repeat(600, 1).cuda()
    assert (F.sampling_cutoff(rep, T, **kw).cpu() == c1).all()
    assert (F.sampling_cutoff(rep, T, top_p=.9).cpu() == cp1).all()
    assert (F.sample_batch(rep, T, seeds=5, counters=9, **kw).cpu() == t1).all()
    others = 2.0 * _randn(g, 37, V)
    spots = [3, 17, 36]
    perm = torch.randperm(37, generator=g)
    mixed = others[perm].clone()
    mixed[spots] = row
    seeds = torch.arange(37) + 100
    counters = torch.arange(37)
    seeds[spots], counters[spots] = 5, 9
    x = mixed.cuda()
    c = F.sampling_cutoff(x, T, **kw).cpu()
    t = F.sample_batch(x, T, seeds=seeds.cuda(), counters=counters.cuda(), **kw).cpu()
    assert (c[spots] == c1).all() and (t[spots] == t1).all()
    assert (F.sampling_cutoff(x, T, top_p=.9).cpu()[spots] == cp1).all()
    # two consecutive calls
    assert torch.equal(F.sampling_cutoff(x, T, **kw).cpu(), c)
    assert torch.equal(
        F.sample_batch(x, T, seeds=seeds.cuda(), counters=counters.cuda(), **kw).cpu(), t)


EV = 4099


def _cut(row, T=1.0, **kw):
    x = torch.as_tensor(row, dtype=torch.float32).reshape(1, -1).cuda()
    return float(F.sampling_cutoff(x, T, **kw).cpu()[0])


SPLIT_ROWS = 64  # below 512 rows the draw kernel splits V = 4099 into 8 chunks of 513


def _draws(row, n=600, T=1.0, seed=11, **kw):
    """n draws of one row: counters 0..n-1 under one seed.  They are taken
    twice: in calls of SPLIT_ROWS rows, where the draw kernel splits the
    vocabulary, and in one call of n rows, which at n >= 512 does not.  A
    draw depends on (seed, counter, row) alone, so the two must agree."""
    x = torch.as_tensor(row, dtype=torch.float32).reshape(1, -1).repeat(n, 1).cuda()
    ctr = torch.arange(n).cuda()
    parts = [F.sample_batch(x[a:a + SPLIT_ROWS], T, seeds=seed,
                            counters=ctr[a:a + SPLIT_ROWS], **kw)
             for a in range(0, n, SPLIT_ROWS)]
    split = torch.cat(parts).cpu().numpy()
    whole = F.sample_batch(x, T, seeds=seed, counters=ctr, **kw).cpu().numpy()
    assert (split == whole).all(), np.nonzero(split != whole)[0][:8]
    return split


def _base(seed):
    return _randn(_gen(seed), EV).clamp_(max=3.0)


@gpu_test
def test_edge_all_equal_keeps_everything():
    row = torch.full((EV,), 1.25)
    for kw in (dict(top_k=5), dict(top_p=.1), dict(min_p=.5), dict(min_p=1.),
               dict(top_k=40, top_p=.8, min_p=.02)):
        assert _cut(row, **kw) == 1.25, kw
    tok = _draws(row, top_k=5, top_p=.1)
    assert len(set(tok.tolist())) > 400  # draws from all 4099, not from 5


@gpu_test
def test_edge_filters_that_keep_only_the_argmax():
    row = _base(1)
    row[2600] = 4.5
    for kw in (dict(top_k=1), dict(top_p=1e-6), dict(min_p=1.)):
        assert _cut(row, **kw) == 4.5, kw
        for seed in SEEDS:
            assert (_draws(row, n=64, seed=seed, **kw) == 2600).all(), (kw, seed)


@gpu_test
def test_edge_top_k_off_values():
    row = _base(2)
    for k in (0, EV, EV + 5, 2 ** 31 - 1):
        assert _cut(row, top_k=k) == NEG_INF, k
    assert _cut(row, top_k=EV - 1) == float(row.sort().values[1])


@gpu_test
@pytest.mark.parametrize("dup", [(512, 513), (600, 3000)])
def test_edge_kth_value_duplicated(dup):
    """The k-th largest value sits twice in the row: at the last index of
    chunk 0 and the first of chunk 1 of the split draw (8 chunks of 513), or
    two chunks apart.  Both copies are kept, with the vocabulary split (calls
    of 64 rows) and unsplit (one call of 600): `_draws` takes both."""
    row = _base(3)
    row[[40, 1500, 4000]] = 7.0
    row[list(dup)] = 5.0
    assert _cut(row, top_k=4) == 5.0
    tok = _draws(row, T=2.0, top_k=4)
    assert set(tok.tolist()) == {40, 1500, 4000, *dup}


@gpu_test
def test_edge_two_valued_row():
    row = torch.full((EV,), -1.0)
    row[::2] = 1.0  # 2050 ones
    assert _cut(row, top_k=10) == 1.0
    assert _cut(row, top_k=2050) == 1.0
    assert _cut(row, top_k=2051) == -1.0
    assert _cut(row, top_p=.5) == 1.0      # the ones alone hold 88 % of the mass
    assert _cut(row, top_p=.95) == -1.0
    assert _cut(row, min_p=.5) == 1.0      # e^-2 = .135
    assert _cut(row, min_p=.1) == -1.0
    assert (_draws(row, n=256, top_p=.5) % 2 == 0).all()


@gpu_test
def test_edge_half_minus_inf():
    """top_k beyond the finite count keeps the finite tokens and nothing
    else: -inf is never kept by a filter and never sampled."""
    g = _gen(4)
    row = _base(4)
    dead = torch.rand(EV, generator=g) < 0.5
    dead[[0, 513, 1026, 4098]] = True
    row[dead] = NEG_INF
    nfin = int((~dead).sum())
    low = float(row[~dead].min())
    assert _cut(row, top_k=nfin + 100) == low
    assert _cut(row, top_k=EV - 1) == low
    assert _cut(row, top_k=nfin + 100, top_p=.999999, min_p=1e-30) >= low
    tok = _draws(row, T=3.0, top_k=nfin + 100)
    assert not dead.numpy()[tok].any()
    assert len(set(tok.tolist())) > 300
    c = _cut(row, top_p=.9, min_p=.01)
    want = cutoff_band(row.reshape(1, -1), 0, .9, .01, 1.0)
    assert want[0][0] <= c <= want[1][0] and c > NEG_INF


@gpu_test
def test_edge_three_finite_tokens():
    row = torch.full((EV,), NEG_INF)
    row[[4098, 513, 7]] = torch.tensor([2.0, 1.0, 0.0])  # e = 1, .368, .135
    assert _cut(row, top_k=2) == 1.0
    assert _cut(row, top_k=3) == 0.0 and _cut(row, top_k=900) == 0.0
    assert _cut(row, top_p=.5) == 2.0      # 1 > .5 * 1.503
    assert _cut(row, top_p=.7) == 1.0      # 1 <= 1.052 < 1.368
    assert _cut(row, top_p=.95) == 0.0
    assert _cut(row, min_p=.2) == 1.0
    assert _cut(row, top_k=2, top_p=.7) == 2.0  # renormalised over two: 1 > .958
    assert set(_draws(row, top_p=.7).tolist()) == {4098, 513}


@gpu_test
def test_edge_zeros_of_both_signs_at_the_cutoff():
    row = -_base(5).abs() - 1.0
    row[7], row[3], row[3000] = 2.0, -0.0, 0.0
    for k in (2, 3):
        assert _cut(row, top_k=k) == 0.0
        assert set(_draws(row, top_k=k).tolist()) == {7, 3, 3000}
    assert _cut(row, min_p=.1) == 0.0      # e^-2 = .135, the rest below e^-3
    assert set(_draws(row, min_p=.1).tolist()) == {7, 3, 3000}


@gpu_test
def test_edge_underflowing_mass():
    """logits +-1e4 at T = 0.05: e_i of the low half is exactly 0."""
    row = torch.full((EV,), -1e4)
    row[[5, 2000, 4098]] = 1e4
    T = 0.05
    assert _cut(row, T, top_p=.9) == 1e4
    assert _cut(row, T, top_p=.3) == 1e4   # ties are kept together
    assert _cut(row, T, min_p=.5) == 1e4
    assert _cut(row, T, top_k=3) == 1e4
    assert _cut(row, T, top_k=4) == -1e4
    assert _cut(row, T, top_k=4, top_p=.9) == 1e4
    assert set(_draws(row, T=T, top_p=.9).tolist()) == {5, 2000, 4098}


TOPK4_ROWS, TOPK4_SEED, TOPK4_MAX = 4096, 1234, 30.7


def _chi2_top4(tokens):
    lg = _chi2_logits().astype(np.float64)
    assert set(np.unique(tokens).tolist()) <= {12, 13, 14, 15}, np.unique(tokens)
    p = np.exp(lg[12:] - lg.max())
    want = TOPK4_ROWS * p / p.sum()
    got = np.bincount(np.asarray(tokens, dtype=np.int64) - 12, minlength=4)
    assert got.sum() == TOPK4_ROWS
    return float(((got - want) ** 2 / want).sum())


@gpu_test
def test_distribution_top_k_chi_square():
    logits = torch.from_numpy(_chi2_logits()).repeat(TOPK4_ROWS, 1).cuda()
    tok = F.sample_batch(logits, 1.0, top_k=4, seeds=TOPK4_SEED,
                         counters=torch.arange(TOPK4_ROWS).cuda()).cpu().numpy()
    stat = _chi2_top4(tok)
    print(f"chi-square on GPU {stat:.2f}")
    assert stat <= TOPK4_MAX


@gpu_test
def test_binding_errors_raise():
    from modal_examples_amd.ops._build import get_ext

    ext = get_ext(required=True)
    x = torch.randn(4, 100, device="cuda")
    t = torch.ones(4, device="cuda")
    k = torch.zeros(4, dtype=torch.int32, device="cuda")
    z = torch.zeros(4, dtype=torch.int64, device="cuda")
    bad_calls = [
        lambda: ext.sampling_cutoff(x.double(), t, k, t, t),        # dtype
        lambda: ext.sampling_cutoff(x, t, k.long(), t, t),
        lambda: ext.sampling_cutoff(x, t.double(), k, t, t),
        lambda: ext.sampling_cutoff(x.cpu(), t, k, t, t),           # device
        lambda: ext.sampling_cutoff(x, t, k, t.cpu(), t),
        lambda: ext.sampling_cutoff(x, t[:3], k, t, t),             # length
        lambda: ext.sampling_cutoff(x, t, k, t, t.repeat(2)),
        lambda: ext.sampling_cutoff(x[0], t, k, t, t),              # shape
        lambda: ext.sample_batch(x.half(), t, z, z, None),
        lambda: ext.sample_batch(x, t, z.int(), z, None),
        lambda: ext.sample_batch(x, t, z, z.cpu(), None),
        lambda: ext.sample_batch(x, t, z, z[:2], None),
        lambda: ext.sample_batch(x, t, z, z, t[:1]),
        lambda: ext.sample_batch(x.cpu(), t, z, z, None),
    ]
    for j, call in enumerate(bad_calls):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        F.sample_batch(x, 1.0, top_k=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        F.sampling_cutoff(x, 1.0, top_p=torch.ones(4))
    # the process is alive and the op still works
    assert F.sample_batch(x, 0.0).cpu().tolist() == x.argmax(-1).cpu().tolist()


# ---- CPU conditions (unmarked: they need no GPU)

def test_reference_cutoff_matches_the_specification_loop():
    """ops.reference.sampling_cutoff_ref, the float64 reference of the GPU
    tests, against the specification written as a loop over tokens."""
    g = _gen(21)
    rows = [2.0 * _randn(g, 300) for _ in range(3)]
    r = 2.0 * _randn(g, 300)
    r[::3] = NEG_INF
    rows.append(r)
    r = torch.round(2.0 * _randn(g, 300))  # many ties
    r[5], r[200] = -0.0, 0.0
    rows.append(r)
    x = torch.stack(rows)
    sets = PARAM_SETS + ((5, .3, 0., 1.), (0, 1., 1., 1.), (299, 1., 0., 1.),
                         (300, 1., 0., 1.), (250, .99, .001, .5), (1, 1., 0., 1.),
                         (0, 1e-6, 0., 1.), (3, 1., 0., 0.), (0, 1., 0., 1.))
    for k, p, q, T in sets:
        got = cutoff_ref(x, k, p, q, T)
        want = np.array([cutoff_loop(row.numpy(), k, p, q, T) for row in x])
        assert (got == want.astype(np.float32)).all(), (k, p, q, T, got, want)


def test_cpu_dispatch_is_the_reference_and_matches_host_model():
    """F.sample_batch on CPU tensors: the reference's hash is the kernel's."""
    x = 2.0 * _randn(_gen(22), 6, 1025)
    for seed in SEEDS:
        got = F.sample_batch(x, 0.7, seeds=seed).numpy()
        assert (got == gumbel_scores(x.numpy(), 0.7, seed).argmax(-1)).all()
    seeds = [SEEDS[r % 4] for r in range(6)]
    counters = np.arange(6) * 5 + 1
    c = F.sampling_cutoff(x, 1.0, top_k=40, top_p=.8, min_p=.02).numpy()
    tok = F.sample_batch(x, 1.0, top_k=40, top_p=.8, min_p=.02,
                         seeds=torch.tensor(seeds),
                         counters=torch.from_numpy(counters)).numpy()
    excused, total = _check_tokens(x, 1.0, seeds, counters, c, tok)
    assert (excused, total) == (0, 6)
    assert (F.sample_batch(x, 0.0, top_k=3).numpy() == x.numpy().argmax(-1)).all()
    with pytest.raises(ValueError):
        F.sample_batch(x, 1.0, top_p=torch.ones(5))


@functools.lru_cache(maxsize=None)
def _mass_precision():
    """Largest differences between float64 and the emulated kernel arithmetic:
    (mass fraction above a token, relative e_i where e_i >= 1e-3)."""
    d_mass = d_e = 0.0
    for V in VOCABS:
        lg = (2.0 * _randn(_gen(1000 + V), 5, V)).numpy()
        for k, p, q, T in PARAM_SETS:
            t32 = np.float32(T)
            for x in lg:
                order = np.argsort(-x, kind="stable")
                xs = x[order]
                n = k if 0 < k < V else V
                e32, fx = _emulated_mass(xs, np.float32(1.0) / t32)
                s64 = xs.astype(np.float64) / np.float64(t32)
                e64 = np.exp(s64 - s64[0])
                f64 = (np.cumsum(e64[:n]) - e64[:n]) / e64[:n].sum()
                femu = (np.cumsum(fx[:n]) - fx[:n]) / fx[:n].sum()
                d_mass = max(d_mass, float(np.abs(f64 - femu).max()))
                big = e64 >= 1e-3
                d_e = max(d_e, float(np.abs(e32[big] / e64[big] - 1.0).max()))
    return d_mass, d_e


def test_host_mass_precision_sets_cut_delta():
    """CUT_DELTA is 100x the float32 + fixed-point error of the kernel's own
    arithmetic, and within what the sandwich may use."""
    d_mass, d_e = _mass_precision()
    print(f"mass fraction: {d_mass:.3g}; relative e_i: {d_e:.3g}")
    assert 100.0 * max(d_mass, d_e) <= CUT_DELTA <= 1e-3


def test_host_band_pins_the_cutoff():
    """The two reference cutoffs of the sandwich differ by 2 kept tokens at
    most (15 are allowed), so a cutoff inside the band is pinned."""
    worst = 0
    for V in (1000, 4099):
        logits = 2.0 * _randn(_gen(V), 8, V)
        for k, p, q, T in PARAM_SETS:
            lo, hi = cutoff_band(logits, k, p, q, T)
            assert (lo <= hi).all()
            kept_lo = (logits.numpy() >= lo[:, None]).sum(-1)
            kept_hi = (logits.numpy() >= hi[:, None]).sum(-1)
            worst = max(worst, int((kept_lo - kept_hi).max()))
    print(f"kept tokens across the band: at most {worst}")
    assert worst <= 15


def test_host_near_tie_share_under_filters():
    near = total = 0
    for V in (1000, 4099):
        logits = 2.0 * _randn(_gen(V), 8, V)
        lg = logits.numpy()
        for k, p, q, T in PARAM_SETS:
            keep = lg >= cutoff_ref(logits, k, p, q, T)[:, None]
            for seed in range(1, 65):
                sc = np.where(keep, row_scores(lg, T, seed, np.arange(8)), NEG_INF)
                top2 = np.partition(sc, -2, axis=-1)[:, -2:]
                near += int(((top2[:, 1] - top2[:, 0]) < DELTA).sum())
                total += 8
    print(f"near-tie share {near}/{total} = {near / total:.5f}")
    assert total == 4096 and near <= 0.01 * total


def test_host_chi_square_top_k_precheck():
    lg = np.tile(_chi2_logits(), (TOPK4_ROWS, 1))
    sc = row_scores(lg, 1.0, TOPK4_SEED, np.arange(TOPK4_ROWS))
    sc[:, :12] = NEG_INF
    stat = _chi2_top4(sc.argmax(-1))
    print(f"chi-square of the host model {stat:.2f}")
    assert stat <= TOPK4_MAX
