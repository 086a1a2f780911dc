"""Strict tier for the attention forward (csrc/attention_fwd32.hip), the
parts that need no GPU: the shape table, the case builders, the judge that
decides whether an (o, lse) pair is a correct forward, and the proof that the
judge would notice a subtly wrong kernel.  test_attention_forward_gpu.py runs
the kernel through the same builders and the same judge.

The rules, on every element and every row (no fraction is left out):

  o     With o64 the fp64 truth on the bf16 inputs and e_y the max error of
        the bf16-emulating yardstick (reference.attention_fwd_ref with
        emulate_bf16=True) against o64,
            max|o - o64| <= 2 * e_y + 2**-8 * max|o64|
        (the rule of test_attention_backward_gpu.py), with no NaN or Inf.
  lse   |lse - lse64| <= 1e-3 on every row.
  exact A case that carries `exact` (selector_case) must match it bit for
        bit.
  rows that see no key (causal, Sq > Sk): o exactly 0, lse exactly -inf.

The tiles behind the shape table: q block 128 (4 waves x 32 rows), KV block
64 at D=64 and 32 at D=128, score fragments of 32 keys."""
import functools
import math

import pytest
import torch

from modal_examples_amd.ops import functional as F
from modal_examples_amd.ops import reference as ref

BF = torch.bfloat16
LSE_TOL = 1e-3
B = 2
DS = (64, 128)

# (Hq, Hkv, Sq, Sk, causal)
SHAPES = [
    (3, 3, 160, 160, True),    # full q block + ragged one; Sk 2.5 / 5 blocks
    (2, 2, 129, 129, True),    # one row past a q block
    (4, 2, 96, 224, True),     # causal_off > 0, GQA group of 2
    (2, 2, 1, 33, True),       # single query, one key past a fragment
    (3, 3, 160, 77, False),    # cross attention, Sk no multiple of 32
    (2, 2, 130, 1, False),     # a single key
    (2, 2, 33, 64, False),     # Sk exactly one KV block at D=64
    (2, 2, 31, 65, False),     # one key past that block
    (2, 2, 256, 256, False),   # exact multiples everywhere
    (2, 2, 256, 256, True),    # `full` shortcut on every block but the diagonal
]
# the ramp / random families of the GPU tier
WIDE_SHAPES = [
    (3, 3, 160, 160, True), (3, 3, 160, 160, False), (4, 2, 96, 224, True),
    (3, 3, 160, 77, False), (2, 2, 256, 256, True), (2, 2, 256, 256, False),
]
# causal with Sq > Sk: rows i < Sq - Sk see no key.  (160,96) and (200,77)
# hide part of q block 0, (130,1) hides it whole and leaves one live row.
HIDDEN_SHAPES = [(2, 2, 160, 96, True), (2, 2, 200, 77, True),
                 (2, 2, 130, 1, True)]
GROWTHS = (3.0, 12.0, -3.0, -12.0)


def shape_id(s):
    return "Hq%d-Hkv%d-Sq%d-Sk%d-%s" % (s[0], s[1], s[2], s[3],
                                         "causal" if s[4] else "full")


def visible_counts(Sq, Sk, causal):
    """n_i, the number of keys row i sees, int64 [Sq] (0 for a hidden row)."""
    if not causal:
        return torch.full((Sq,), Sk, dtype=torch.long)
    return (torch.arange(Sq) + (Sk - Sq) + 1).clamp(0, Sk)


def _finish(name, q, k, v, causal, scale, **extra):
    """The case dict: bf16 inputs, the fp64 truth on them and the error of
    the bf16-emulating yardstick.  Computed once and never modified."""
    q64, k64, v64 = q.double(), k.double(), v.double()
    o64, lse64 = ref.attention_fwd_ref(q64, k64, v64, causal, scale)
    o_y, _ = ref.attention_fwd_ref(q64, k64, v64, causal, scale,
                                   emulate_bf16=True)
    Sq, Sk = q.shape[2], k.shape[2]
    c = dict(name=name, q=q, k=k, v=v, causal=causal, scale=scale, o64=o64,
             lse64=lse64, e_y=(o_y - o64).abs().max().item(),
             hidden=visible_counts(Sq, Sk, causal) == 0)
    c.update(extra)
    return c


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _code(idx):
    """+-1 code of the low 10 bits of idx: [..., 10] float."""
    bits = (idx.unsqueeze(-1) >> torch.arange(10)) & 1
    return (bits * 2 - 1).float()


@functools.lru_cache(maxsize=None)
def selector_case(Hq, Hkv, Sq, Sk, causal, D, seed=0):
    """Every query selects ONE visible key so sharply that P is exactly
    one-hot in fp32, and the output is exactly a gathered V row whatever the
    summation order, the block size or the rescale schedule.

    Key j carries the +-1 code of j's low 10 bits in dims 0..9 (zero
    elsewhere); query i carries 512 x the code of its key pi(b,h,i).  The
    selected raw score is 5120, any other at most 4096: after scaling the
    gap is >= 1024/sqrt(128) > 90, and exp(-90) vanishes next to 1 in fp32.
    pi is random among the keys row i sees; every third row takes its LAST
    visible key (the causal diagonal i + Sk - Sq, or Sk - 1).  Late-block
    winners pass through the kernel's `> m_run + 8` rescale with rs ~ 0."""
    assert Sk <= 1024 and not (causal and Sq > Sk)
    g = _gen(seed)
    scale = 1.0 / math.sqrt(D)
    n = visible_counts(Sq, Sk, causal)
    pi = (torch.rand(B, Hq, Sq, generator=g) * n).long().clamp(max=Sk - 1)
    pi = torch.minimum(pi, n - 1)
    last = torch.arange(Sq) % 3 == 2
    pi = torch.where(last, n - 1, pi)
    k = torch.zeros(B, Hkv, Sk, D)
    k[..., :10] = _code(torch.arange(Sk))
    q = torch.zeros(B, Hq, Sq, D)
    q[..., :10] = 512.0 * _code(pi)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    v = torch.where(v == 0, torch.ones_like(v), v)
    G = Hq // Hkv
    vh = v.repeat_interleave(G, dim=1)  # head h reads kv head h // G
    exact = vh.gather(2, pi.unsqueeze(-1).expand(B, Hq, Sq, D))
    c = _finish("selector", q.to(BF), k.to(BF), v, causal, scale, exact=exact,
                pi=pi, lse_expect=torch.full((B, Hq, Sq), 5120.0 * scale,
                                             dtype=torch.float64))
    # soundness: what makes the bitwise comparison meaningful
    assert torch.equal(c["q"].float(), q) and torch.equal(c["k"].float(), k)
    assert torch.equal(c["o64"].to(BF), exact), "gather != fp64 reference"
    o32 = ref.attention_ref(c["q"].float(), c["k"].float(), v.float(), causal,
                            scale)
    assert torch.equal(o32.to(BF), exact), "gather != fp32 reference"
    assert (exact != 0).all(), "a selected V element is 0"
    assert (c["lse64"] - c["lse_expect"]).abs().max() < 1e-9
    assert bool(((pi == n - 1) | ~last).all()) and bool((pi < n).all())
    return c


@functools.lru_cache(maxsize=None)
def count_case(Hq, Hkv, Sq, Sk, causal, D, seed=1):
    """q = 0: every visible score is 0, so lse[b,h,i] = log(n_i) and o is
    the mean of the visible V rows.  log(n+1) - log(n) >= 1/256 for n <= 256,
    so the 1e-3 LSE bound separates every count from its neighbours."""
    assert Sk <= 256
    g = _gen(seed)
    q = torch.zeros(B, Hq, Sq, D).to(BF)
    k = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    n = visible_counts(Sq, Sk, causal).double()
    c = _finish("count", q, k, v, causal, 1.0 / math.sqrt(D),
                lse_expect=torch.log(n).expand(B, Hq, Sq))
    assert (c["lse64"] - c["lse_expect"])[..., n > 0].abs().max() < 1e-12
    assert bool((c["lse64"][..., n == 0] == float("-inf")).all())
    return c


@functools.lru_cache(maxsize=None)
def ramp_case(Hq, Hkv, Sq, Sk, causal, D, growth, seed=2):
    """Random q/k/v whose scaled scores carry a ramp: dim 0 of every query
    is a constant and dim 0 of key j a multiple of (1 + j/32), so the score
    of key j is growth * (1 + j/32) on top of N(0,1) noise.

      +3   the running max is deferred for several blocks, then one rescale
           (another cadence at KV block 64 than at 32)
      +12  a rescale on every block
      -3   the max sits in block 0: never a rescale, late P is tiny
      -12  every real score is far below 0: a zero-padded tail key left
           unmasked (score 0) would win the row"""
    g = _gen(seed)
    scale = 1.0 / math.sqrt(D)
    q = torch.randn(B, Hq, Sq, D, generator=g)
    k = torch.randn(B, Hkv, Sk, D, generator=g)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    qc = 16.0
    q[..., 0] = qc
    k[..., 0] = growth * (1.0 + torch.arange(Sk) / 32.0) / (scale * qc)
    c = _finish("ramp%+d" % growth, q.to(BF), k.to(BF), v, causal, scale)
    # the ramp survives the bf16 rounding of K: per 32 keys the mean score of
    # the last visible row moves by growth, to 10 % and the noise of a mean
    if Sk >= 64 and (not causal or Sq >= Sk):
        s = (c["q"][0, 0, -1].double() @ c["k"][0, 0].double().T) * scale
        step = (s[32:64].mean() - s[:32].mean()).item()
        assert abs(step - growth) < 0.1 * abs(growth) + 1.0, step
    return c


def bshd_views(c, device="cpu"):
    """Strided [B,S,H,D] views of the case's q/k/v on `device`, as a
    sequence-major model hands them over: cut from one fused [B,S,3,H,D]
    projection where q and k/v have one shape, else q from [B,Sq,Hq,D] and
    k/v from a fused [B,Sk,2,Hkv,D] projection."""
    q, k, v = (c[n].transpose(1, 2) for n in "qkv")
    if q.shape == k.shape:
        fused = torch.stack([q, k, v], dim=2).contiguous().to(device)
        return fused[:, :, 0], fused[:, :, 1], fused[:, :, 2]
    kv = torch.stack([k, v], dim=2).contiguous().to(device)
    return q.contiguous().to(device), kv[:, :, 0], kv[:, :, 1]


@functools.lru_cache(maxsize=None)
def random_case(Hq, Hkv, Sq, Sk, causal, D, scale=None, seed=3):
    """Plain randn q/k/v; `views` are the strided sequence-major views of
    the same data (bshd_views)."""
    g = _gen(seed)
    q = torch.randn(B, Hq, Sq, D, generator=g).to(BF)
    k = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    c = _finish("random", q, k, v, causal,
                scale if scale is not None else 1.0 / math.sqrt(D))
    c["views"] = bshd_views(c)
    return c


# ------------------------------------------------------------------ the judge

def judge(c, o, lse, label):
    """Raise AssertionError unless (o [B,Hq,Sq,D], lse [B,Hq,Sq] or None) is
    a correct forward of case c by the rules in the module docstring.  Prints
    the measured figures (pytest -s shows them)."""
    o64, hidden = c["o64"], c["hidden"]
    assert tuple(o.shape) == tuple(o64.shape), f"{label}: o shape {o.shape}"
    o_bits = o.detach().cpu()
    o = o_bits.double()
    assert torch.isfinite(o).all(), f"{label}: NaN/Inf in o"
    err = (o - o64).abs().max().item()
    top = o64.abs().max().item()
    e_y = c["e_y"]
    ratio = err / e_y if e_y > 0 else (0.0 if err == 0 else math.inf)
    print(f"ATTN_FWD_RATIO {label} err={err:.4e} e_y={e_y:.4e} "
          f"ratio={ratio:.3f} max|o64|={top:.4e}")
    assert err <= 2.0 * e_y + 2.0 ** -8 * top, (
        f"{label}: max err {err:.4e} > 2*{e_y:.4e} + 2^-8*{top:.4e}")
    if "exact" in c:
        assert o_bits.dtype is BF, f"{label}: o is {o_bits.dtype}"
        bad = (o_bits != c["exact"]).any(-1)
        assert not bad.any(), (
            f"{label}: {int(bad.sum())} rows differ from the gathered V rows,"
            f" first (b,h,i) = {tuple(bad.nonzero()[0].tolist())}")
    if hidden.any():
        assert bool((o[:, :, hidden] == 0).all()), (
            f"{label}: a row that sees no key is not exactly 0")
    if lse is None:
        return
    assert tuple(lse.shape) == tuple(c["lse64"].shape), (
        f"{label}: lse shape {lse.shape}")
    lse = lse.detach().cpu().double()
    assert not torch.isnan(lse).any(), f"{label}: NaN in lse"
    if hidden.any():
        assert bool((lse[:, :, hidden] == float("-inf")).all()), (
            f"{label}: lse of a row that sees no key is not -inf")
    live = ~hidden
    assert torch.isfinite(lse[:, :, live]).all(), f"{label}: Inf in lse"
    for name in ("lse64", "lse_expect"):
        if name in c:
            lerr = (lse - c[name])[:, :, live].abs().max().item()
            print(f"ATTN_FWD_LSE {label} vs {name} err={lerr:.3e}")
            assert lerr <= LSE_TOL, (
                f"{label}: lse off {name} by {lerr:.3e} > {LSE_TOL}")


def rejected(c, o, lse, label="mutant"):
    try:
        judge(c, o, lse, label)
    except AssertionError:
        return True
    return False


def kernel_like(c, dtype=BF):
    """What a correct kernel returns for c: the truth rounded to bf16."""
    return c["o64"].to(dtype), c["lse64"].float()


# -------------------------------------------------- the judge accepts and bites

def _table_cases(shape, D):
    yield selector_case(*shape, D)
    yield count_case(*shape, D)
    yield random_case(*shape, D)
    yield ramp_case(*shape, D, -12.0)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_judge_accepts_the_reference(shape, D):
    for c in _table_cases(shape, D):
        o, lse = kernel_like(c)
        judge(c, o, lse, f"{c['name']} {shape_id(shape)} D{D}")
        judge(c, o, None, f"{c['name']} {shape_id(shape)} D{D} no-lse")
        # and the fp32 reference the loose tier compares against
        o32 = ref.attention_ref(c["q"], c["k"], c["v"], c["causal"],
                                c["scale"])
        l32 = ref.attention_lse_ref(c["q"], c["k"], c["causal"], c["scale"])
        judge(c, o32, l32, f"{c['name']} {shape_id(shape)} D{D} fp32 ref")


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("growth", GROWTHS)
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=shape_id)
def test_judge_accepts_the_reference_on_ramps(shape, growth, D):
    c = ramp_case(*shape, D, growth)
    judge(c, *kernel_like(c), f"ramp{growth:+.0f} {shape_id(shape)} D{D}")


def _attn64(c, mask, gqa="div", pad=0):
    """fp64 attention of case c under an arbitrary visibility mask [Sq,Sk+pad]
    (pad zero K/V rows appended), rounded as a kernel rounds its results;
    the vehicle of the mutants below."""
    q, k, v = (c[n].double() for n in "qkv")
    if pad:
        z = torch.zeros(*k.shape[:2], pad, k.shape[3], dtype=torch.float64)
        k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
    Hq, Hkv = q.shape[1], k.shape[1]
    heads = torch.arange(Hq)
    hk = heads // (Hq // Hkv) if gqa == "div" else heads % Hkv
    k, v = k[:, hk], v[:, hk]
    s = torch.matmul(q, k.transpose(-1, -2)) * c["scale"]
    s = s.masked_fill(~mask, float("-inf"))
    m = s.amax(-1, keepdim=True)
    live = m > float("-inf")
    p = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))
    l = p.sum(-1, keepdim=True)
    o = torch.where(live, torch.matmul(p, v) / l.clamp(min=1e-300),
                    torch.zeros_like(l))
    lse = (torch.where(live, m, torch.zeros_like(m)) + torch.log(l))
    return o.to(BF), lse.squeeze(-1).float()


def _mask(c, shift=0, shift_from_row=0, pad=0):
    Sq, Sk = c["q"].shape[2], c["k"].shape[2]
    if not c["causal"]:
        return torch.ones(Sq, Sk + pad, dtype=torch.bool)
    off = (Sk - Sq) + shift * (torch.arange(Sq) >= shift_from_row).long()
    return torch.arange(Sk + pad)[None, :] <= (torch.arange(Sq) + off)[:, None]


def _m_identity(c):
    return _attn64(c, _mask(c))


def _m_off_plus(c):
    return _attn64(c, _mask(c, +1))


def _m_off_minus(c):
    return _attn64(c, _mask(c, -1))


def _m_off_plus_late(c):  # only the last 32 rows
    return _attn64(c, _mask(c, +1, c["q"].shape[2] - 32))


def _m_off_minus_late(c):
    return _attn64(c, _mask(c, -1, c["q"].shape[2] - 32))


def _m_last_key_dropped(c):
    m = _mask(c)
    m[:, -1] = False
    return _attn64(c, m)


def _m_tail_unmasked(c):
    Sk = c["k"].shape[2]
    pad = -Sk % 64
    m = _mask(c, pad=pad)
    if not c["causal"]:
        return _attn64(c, m, pad=pad)
    m[:, Sk:] = m[:, Sk - 1:Sk]  # the kvp >= Sk test is what is missing
    return _attn64(c, m, pad=pad)


def _m_gqa_mod(c):
    return _attn64(c, _mask(c), gqa="mod")


def _m_rows_shifted(c):
    o, lse = _m_identity(c)
    return o.roll(1, dims=2), lse.roll(1, dims=2)


def _m_row_from_next_head(c):
    o, lse = _m_identity(c)
    i = o.shape[2] // 2
    o[:, :, i] = o.roll(1, dims=1)[:, :, i]
    return o, lse


def _m_hidden_row_mean_of_block(c):
    """The parent kernel on a hidden row of a live q block: the mean of the
    first 64 (zero-padded) keys and a huge negative finite lse."""
    o, lse = _m_identity(c)
    v = c["v"].double()[:, :, :64].sum(2) / 64
    G = o.shape[1] // v.shape[1]
    h = c["hidden"]
    o[:, :, h] = v.repeat_interleave(G, 1).to(BF)[:, :, None]
    lse[:, :, h] = -1e30
    return o, lse


MUTANTS = [_m_off_plus, _m_off_minus, _m_off_plus_late, _m_off_minus_late,
           _m_last_key_dropped, _m_tail_unmasked, _m_gqa_mod, _m_rows_shifted,
           _m_row_from_next_head]


def test_mutant_vehicle_reproduces_the_reference():
    for shape in SHAPES + HIDDEN_SHAPES:
        c = random_case(*shape, 64)
        o, lse = _m_identity(c)
        assert torch.equal(o, c["o64"].to(BF)), shape_id(shape)
        assert torch.equal(lse, c["lse64"].float()), shape_id(shape)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__[3:])
def test_judge_rejects_the_mutant(mutant, D):
    """Each wrong kernel must fail the judge on at least one table shape,
    under at least one builder; the survivors-everywhere would be the gaps of
    this suite."""
    killed = []
    for shape in SHAPES:
        for c in _table_cases(shape, D):
            if rejected(c, *mutant(c)):
                killed.append(f"{c['name']} {shape_id(shape)}")
    print(f"ATTN_FWD_MUTANT {mutant.__name__[3:]} D{D} rejected on "
          f"{len(killed)} cases: {killed}")
    assert killed, (f"mutant {mutant.__name__[3:]} D{D} passes the judge on "
                    f"every table shape {[shape_id(s) for s in SHAPES]}")


# which single shapes are there for which mutant: the table must not lose them
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mutant,builder,shape", [
    (_m_off_plus_late, count_case, (2, 2, 256, 256, True)),
    (_m_off_minus_late, count_case, (2, 2, 256, 256, True)),
    (_m_off_minus_late, selector_case, (3, 3, 160, 160, True)),
    (_m_off_plus, count_case, (4, 2, 96, 224, True)),
    (_m_last_key_dropped, count_case, (2, 2, 256, 256, False)),
    (_m_last_key_dropped, selector_case, (3, 3, 160, 77, False)),
    (_m_tail_unmasked, count_case, (2, 2, 31, 65, False)),
    (_m_tail_unmasked, count_case, (2, 2, 1, 33, True)),
    (_m_gqa_mod, selector_case, (4, 2, 96, 224, True)),
    (_m_rows_shifted, selector_case, (2, 2, 129, 129, True)),
    (_m_row_from_next_head, selector_case, (2, 2, 256, 256, False)),
], ids=lambda x: shape_id(x) if isinstance(x, tuple) else x.__name__)
def test_named_shape_rejects_the_mutant(mutant, builder, shape, D):
    c = builder(*shape, D)
    assert rejected(c, *mutant(c)), (
        f"{mutant.__name__[3:]} survives {c['name']} {shape_id(shape)} D{D}")


@pytest.mark.parametrize("D", DS)
def test_ramp_minus12_rejects_the_unmasked_tail(D):
    # every real score is far below the pad's 0: the pad takes the row
    for shape in [(3, 3, 160, 77, False), (3, 3, 160, 160, True)]:
        c = ramp_case(*shape, D, -12.0)
        if -c["k"].shape[2] % 64:
            assert rejected(c, *_m_tail_unmasked(c)), shape_id(shape)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", HIDDEN_SHAPES, ids=shape_id)
def test_judge_on_hidden_rows(shape, D):
    for c in (random_case(*shape, D), count_case(*shape, D)):
        label = f"{c['name']} {shape_id(shape)} D{D}"
        assert c["hidden"].sum() == shape[2] - shape[3]
        judge(c, *kernel_like(c), label)
        assert rejected(c, *_m_hidden_row_mean_of_block(c)), label
        o, lse = kernel_like(c)
        lse[:, :, c["hidden"]] = -1e30  # finite is not -inf
        assert rejected(c, o, lse), label
        o, lse = kernel_like(c)
        o[0, 0, 0, 0] = 2.0 ** -20      # tiny is not 0
        assert rejected(c, o, lse), label


def test_judge_rejects_nan_inf_and_shapes():
    c = random_case(2, 2, 33, 64, False, 64)
    o, lse = kernel_like(c)
    judge(c, o, lse, "sane")
    for bad in (float("nan"), float("inf")):
        o2 = o.clone()
        o2[1, 1, 5, 7] = bad
        assert rejected(c, o2, lse)
        l2 = lse.clone()
        l2[1, 0, 3] = bad
        assert rejected(c, o, l2)
    assert rejected(c, o[:, :, :-1], lse)
    assert rejected(c, o, lse[:, :, :-1])
    o2 = o.clone()
    o2[0, 1, 32, 63] += 0.25   # ONE element of 8448
    assert rejected(c, o2, lse)
    l2 = lse.clone()
    l2[0, 1, 32] += 2e-3
    assert rejected(c, o, l2)


def test_selector_is_bitwise_only_for_the_gather():
    c = selector_case(4, 2, 96, 224, True, 128)
    o, lse = kernel_like(c)
    judge(c, o, lse, "selector")
    o2 = o.clone().view(torch.int16)
    o2[1, 3, 95, 127] ^= 1     # one ulp of one element
    assert rejected(c, o2.view(BF), lse)


# ------------------------------------------------------- yardstick soundness

@pytest.mark.parametrize("D", DS)
def test_fwd_ref_matches_attention_ref_and_lse_ref(D):
    for shape in SHAPES + HIDDEN_SHAPES:
        c = random_case(*shape, D)
        q, k, v = (c[n].double() for n in "qkv")
        o, lse = ref.attention_fwd_ref(q, k, v, c["causal"], c["scale"])
        assert o.dtype is torch.float64 and lse.dtype is torch.float64
        o_a = ref.attention_ref(q, k, v, c["causal"], c["scale"])
        l_a = ref.attention_lse_ref(q, k, c["causal"], c["scale"])
        assert (o - o_a).abs().max() <= 1e-12, shape_id(shape)
        live = ~c["hidden"]
        assert (lse - l_a)[:, :, live].abs().max() <= 1e-12
        assert torch.equal(lse[:, :, ~live], l_a[:, :, ~live])
        # default scale, fp32 working precision
        o32, l32 = ref.attention_fwd_ref(c["q"], c["k"], c["v"], c["causal"])
        assert o32.dtype is torch.float32 and l32.dtype is torch.float32
        if c["scale"] == 1.0 / math.sqrt(D):
            assert (o32.double() - o).abs().max() <= 1e-5


@pytest.mark.parametrize("D", DS)
def test_fwd_ref_bf16_emulation_is_a_sane_yardstick(D):
    for shape in WIDE_SHAPES:
        for c in (random_case(*shape, D), ramp_case(*shape, D, 12.0)):
            top = c["o64"].abs().max().item()
            # at least the rounding of the output, at most a few bf16 ulps
            assert 2.0 ** -11 * top < c["e_y"] < 2.0 ** -6 * top, (
                shape_id(shape), c["name"], c["e_y"], top)


# ------------------------------------------------------- rows that see no key

def _parent_attention_ref(q, k, v, causal, scale):
    """reference.attention_ref before it learned about hidden rows."""
    Hq, Sq = q.shape[1], q.shape[2]
    Hkv, Sk = k.shape[1], k.shape[2]
    qf, kf, vf = q.float(), k.float(), v.float()
    if Hkv != Hq:
        rep = Hq // Hkv
        kf = kf.repeat_interleave(rep, dim=1)
        vf = vf.repeat_interleave(rep, dim=1)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        mask = torch.ones(Sq, Sk, dtype=torch.bool).tril(Sk - Sq)
        s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, vf).to(q.dtype)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_attention_ref_unchanged_where_every_row_sees_a_key(shape, D):
    c = random_case(*shape, D)
    got = ref.attention_ref(c["q"], c["k"], c["v"], c["causal"], c["scale"])
    want = _parent_attention_ref(c["q"], c["k"], c["v"], c["causal"],
                                 c["scale"])
    assert got.dtype is BF and torch.equal(got, want)


@pytest.mark.parametrize("Sq,Sk", [(8, 4), (200, 77)])
def test_hidden_rows_are_zero_and_minus_inf(Sq, Sk):
    g = _gen(7)
    q = torch.randn(2, 4, Sq, 64, generator=g).to(BF)
    k = torch.randn(2, 2, Sk, 64, generator=g).to(BF)
    v = torch.randn(2, 2, Sk, 64, generator=g).to(BF)
    nh = Sq - Sk
    for wide in (lambda t: t, torch.Tensor.float, torch.Tensor.double):
        qq, kk, vv = wide(q), wide(k), wide(v)
        o = ref.attention_ref(qq, kk, vv, True, 0.125)
        lse = ref.attention_lse_ref(qq, kk, True, 0.125)
        of, lf = ref.attention_fwd_ref(qq, kk, vv, True, 0.125)
        oe, le = ref.attention_fwd_ref(qq, kk, vv, True, 0.125,
                                       emulate_bf16=True)
        for oo in (o, of, oe):
            assert torch.isfinite(oo).all()
            assert bool((oo[:, :, :nh] == 0).all())
            assert bool((oo[:, :, nh:].abs().sum(-1) > 0).all())
        for ll in (lse, lf, le):
            assert bool((ll[:, :, :nh] == float("-inf")).all())
            assert torch.isfinite(ll[:, :, nh:]).all()
        # the live rows are the attention of the last Sk queries, Sq == Sk
        tail = ref.attention_ref(qq[:, :, nh:], kk, vv, True, 0.125)
        assert (o[:, :, nh:].double() - tail.double()).abs().max() <= 1e-6
    # F.attention on the CPU is the same reference
    assert torch.equal(F.attention(q, k, v, causal=True),
                       ref.attention_ref(q, k, v, True, 0.125))


def test_no_key_at_all_raises_on_the_cpu_too():
    q, kv = torch.zeros(1, 2, 4, 64), torch.zeros(1, 2, 0, 64)
    with pytest.raises(ValueError, match="Sk"):
        F.attention(q, kv, kv)
    with pytest.raises(ValueError, match="Sk"):
        F.attention_qkv(q.transpose(1, 2), kv.transpose(1, 2),
                        kv.transpose(1, 2), causal=True)
    # no query is no error: the empty tensor of the right shape
    assert F.attention(q[:, :, :0], q, q).shape == (1, 2, 0, 64)
    assert F.attention_qkv(q[:0].transpose(1, 2), q[:0].transpose(1, 2),
                           q[:0].transpose(1, 2)).shape == (0, 4, 128)


@pytest.mark.parametrize("Sq,Sk", [(8, 4), (200, 77)])
def test_hidden_rows_have_finite_zero_gradients(Sq, Sk):
    g = _gen(8)
    q, k, v = (torch.randn(1, 2, s, 64, generator=g, dtype=torch.float64)
               .requires_grad_(True) for s in (Sq, Sk, Sk))
    dout = torch.randn(1, 2, Sq, 64, generator=g, dtype=torch.float64)
    nh = Sq - Sk
    o = F.attention(q, k, v, causal=True)  # grad mode: the reference
    gq, gk, gv = torch.autograd.grad(o, (q, k, v), dout)
    for t in (gq, gk, gv):
        assert torch.isfinite(t).all()
    assert bool((gq[:, :, :nh] == 0).all())
    # (row nh sees one key: its P is the constant 1 and dq is truly zero)
    assert bool((gq[:, :, nh + 1:].abs().sum(-1) > 0).all())
    # the hidden rows' dout reaches nothing: same k/v gradients without them
    q2 = q.detach()[:, :, nh:].clone().requires_grad_(True)
    o2 = ref.attention_ref(q2, k, v, True, 0.125)
    gq2, gk2, gv2 = torch.autograd.grad(o2, (q2, k, v), dout[:, :, nh:])
    assert (gq[:, :, nh:] - gq2).abs().max() <= 1e-12
    assert (gk - gk2).abs().max() <= 1e-12 and (gv - gv2).abs().max() <= 1e-12
