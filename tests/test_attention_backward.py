"""CPU tier for the attention backward: the torch reference of the
recompute-from-LSE algorithm (the HIP kernel's specification and the
yardstick for its tolerance) against autograd, and the unchanged CPU
dispatch of F.attention in grad mode.

Below them, the strict tier for csrc/attention_bwd.hip, the parts that need
no GPU: the shape table, the case builders, the judge that decides whether
(dq, dk, dv) is a correct backward, and the proof that the judge would
notice a subtly wrong kernel.  test_attention_backward_strict_gpu.py runs
the kernel through the same builders and the same judge.

The rule, on every element of dq, dk and dv (none is excused).  The kernel
is handed o = bf16(o64) and lse = fp32(lse64), g64 is the fp64 backward on
the unrounded o64 and lse64, and A the matching magnitude of
reference.attention_bwd_bound_ref (the absolute-value propagation of P into
dv, of |dS| + P*E_q into dq and dk):

    |got - g64| <= 2^-8 * (A + |g64|) + eps32 * A,     got finite,
    got == 0 exactly where A + |g64| == 0 (masked, single-key or zero-dout
    rows, scale 0).

2^-8 is bf16's unit roundoff and the first term the worst case of the
kernel's two roundings on the way to an element (P or dS, and the output;
dS inherits the one rounding of o through delta, the P*E_q part), with no
factor on top.  eps32 = 2^-20 * (1 + M), M = max(|s*scale| + |lse|) of the
case, is 16 fp32 ulps of the exponential's argument: an allowance for the
fp32 argument, the fast exponential and the fp32 sums that is chosen to be
negligible, not tuned.  It is capped at 1 % of 2^-8; the cap binds only for
the peaked family (M = 68, 1.7 % uncapped), where it makes the rule
tighter.  A case that carries `exact` (unit_case) must match it bit for bit.

The tiles behind the shape table: dK/dV 128 keys per workgroup, 32 per
wave, query slices of 32 rows, the G heads of a group outermost; dQ and
delta 128 query rows per workgroup, key tiles of 32.

Worst err / tol of the bf16 yardstick (roundings at the kernel's places,
fp64 sums), measured here, D = 64 | 128:

    family   dq             dk             dv
    random   0.394 | 0.399  0.625 | 0.651  0.948 | 0.887
    peaked   0.446 | 0.339  0.505 | 0.552  0.910 | 0.931
    scale    0.382 | 0.441  0.479 | 0.391  0.745 | 0.828
    graded   0.374 | 0.411  0.748 | 0.627  0.870 | 0.854
    unit     0 (bitwise)

Mutants of the reference (bwd_vehicle), each rejected by the cases NAMED
lists for it: diagonal one key too far; qb_start rounded up; dQ's causal
limit one tile short; last ragged query slice missing from dK/dV; last
ragged key tile missing from dQ; one head missing from the group sum; delta
of row i taken from row i^1; lse of head h taken from head 0; scale missing
from dK; dq zeroed on rows whose dout is below 2^-8 of the largest.  The
loose tier's rule (one number per tensor, max err <= 2*e_y + 2^-8 *
max|g64|) applied to the same cases rejects the first nine on homogeneous
random data too.  It ACCEPTS, on every case of this tier, dq zeroed on the
small rows; on the graded family also the dQ limit one tile short (and, at
D = 64, qb_start rounded up); and one dq element off by four times itself
in a row whose dout is 2^-11 of the largest.  Uneven inputs are where one
global slack goes blind."""
import functools
import math

import pytest
import torch

from modal_examples_amd.ops import functional as F
from modal_examples_amd.ops import reference as ref

# (B, Hq, Hkv, Sq, Sk, D, causal)
CASES = [
    (2, 4, 4, 40, 40, 16, False),
    (2, 4, 4, 40, 40, 16, True),
    (1, 4, 2, 33, 33, 32, True),    # GQA
    (1, 4, 2, 17, 50, 16, False),   # Sq != Sk
    (1, 4, 2, 17, 50, 16, True),    # causal, Sk > Sq
    (1, 2, 1, 50, 9, 16, False),
]


def _inputs(B, Hq, Hkv, Sq, Sk, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).double()
    return mk(B, Hq, Sq, D), mk(B, Hkv, Sk, D), mk(B, Hkv, Sk, D), \
        mk(B, Hq, Sq, D)


def _autograd64(q, k, v, dout, causal, scale):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = ref.attention_ref(q, k, v, causal, scale)
    assert o.dtype is torch.float64
    o.backward(dout)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("case", CASES, ids=str)
def test_bwd_ref_fp64_matches_autograd(case):
    B, Hq, Hkv, Sq, Sk, D, causal = case
    q, k, v, dout = _inputs(B, Hq, Hkv, Sq, Sk, D)
    scale = 1.0 / math.sqrt(D)
    o, gq, gk, gv = _autograd64(q, k, v, dout, causal, scale)
    lse = ref.attention_lse_ref(q, k, causal, scale)
    assert lse.shape == (B, Hq, Sq) and lse.dtype is torch.float64

    # lse == logsumexp of the scaled masked scores, built independently here
    rep = Hq // Hkv
    s = torch.matmul(q, k.repeat_interleave(rep, 1).transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(~torch.ones(Sq, Sk, dtype=torch.bool).tril(Sk - Sq),
                          float("-inf"))
    assert (lse - torch.logsumexp(s, -1)).abs().max() <= 1e-9

    dq, dk, dv = ref.attention_bwd_ref(q, k, v, o, lse, dout, causal, scale)
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    for got, want in ((dq, gq), (dk, gk), (dv, gv)):
        assert got.dtype is torch.float64
        assert (got - want).abs().max() <= 1e-9


@pytest.mark.parametrize("case", CASES, ids=str)
def test_bwd_ref_bf16_emulation_is_a_sane_yardstick(case):
    B, Hq, Hkv, Sq, Sk, D, causal = case
    q, k, v, dout = _inputs(B, Hq, Hkv, Sq, Sk, D, seed=1)
    scale = 1.0 / math.sqrt(D)
    o = ref.attention_ref(q, k, v, causal, scale)
    lse = ref.attention_lse_ref(q, k, causal, scale)
    truth = ref.attention_bwd_ref(q, k, v, o, lse, dout, causal, scale)
    emu = ref.attention_bwd_ref(q, k, v, o.to(torch.bfloat16).double(),
                                lse.float(), dout, causal, scale,
                                emulate_bf16=True)
    for got, want in zip(emu, truth):
        assert torch.isfinite(got).all()
        err = (got - want).abs().max().item()
        assert 0.0 < err < 0.05 * want.abs().max().item()


def test_bwd_ref_default_scale_and_fp32():
    q, k, v, dout = (t.float() for t in _inputs(1, 2, 2, 12, 12, 16, seed=2))
    o = ref.attention_ref(q, k, v, True)
    lse = ref.attention_lse_ref(q, k, True)
    dq, dk, dv = ref.attention_bwd_ref(q, k, v, o, lse, dout, True)
    assert dq.dtype is torch.float32
    _, gq, gk, gv = _autograd64(q.double(), k.double(), v.double(),
                                dout.double(), True, 1.0 / math.sqrt(16))
    for got, want in ((dq, gq), (dk, gk), (dv, gv)):
        assert (got.double() - want).abs().max() <= 1e-4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_cpu_grad_mode_keeps_reference_path(dtype):
    torch.manual_seed(3)
    q = torch.randn(1, 4, 20, 64).to(dtype).requires_grad_(True)
    k = torch.randn(1, 2, 24, 64).to(dtype).requires_grad_(True)
    v = torch.randn(1, 2, 24, 64).to(dtype).requires_grad_(True)
    o = F.attention(q, k, v, causal=True)
    assert torch.equal(o, ref.attention_ref(q, k, v, True, 1.0 / 8.0))
    o.float().square().sum().backward()
    for t in (q, k, v):
        assert t.grad is not None and torch.isfinite(t.grad).all()
        assert float(t.grad.abs().sum()) > 0


def test_cpu_attention_qkv_grad_reaches_fused_leaf():
    torch.manual_seed(4)
    qkv = torch.randn(2, 10, 3, 2, 64).to(torch.bfloat16).requires_grad_(True)
    o = F.attention_qkv(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    assert o.shape == (2, 10, 128)
    o.float().sum().backward()
    assert qkv.grad.shape == qkv.shape
    assert all(float(qkv.grad[:, :, i].abs().sum()) > 0 for i in range(3))


# ===================================================================== strict
# The strict tier (module docstring): shape table, builders, judge, mutants.
# test_attention_backward_strict_gpu.py runs the kernel through the same
# builders and the same judge.

BF = torch.bfloat16
B = 2
DS = (64, 128)
U = 2.0 ** -8           # bf16 unit roundoff
EPS32_UNIT = 2.0 ** -20  # 16 fp32 ulps
EPS32_CAP = 0.01 * U     # the fp32 allowance stays negligible next to 2^-8

# (Hq, Hkv, Sq, Sk, causal)
SHAPES = [
    (2, 2, 200, 237, True),    # causal_off 37: qb_start 2 by truncation
    (2, 2, 384, 384, True),    # three key and three query blocks
    (2, 2, 33, 300, True),     # causal_off 267: nothing skipped
    (4, 2, 96, 224, True),     # the forward's GQA shape, causal_off 128
    (6, 2, 160, 160, True),    # G = 3
    (5, 1, 130, 97, False),    # MQA, G = 5, ragged
    (2, 2, 300, 33, False),    # ten query slices, a wave with one key
    (2, 2, 200, 77, False),
    (2, 2, 129, 129, True),
    (2, 2, 1, 33, True),
    (2, 2, 130, 1, False),
    (1, 1, 32, 32, True),
    (1, 1, 1, 1, False),
]
PEAKED_SHAPES = [(2, 2, 200, 237, True), (2, 2, 384, 384, True)]
SCALE_SHAPES = [(6, 2, 160, 160, True), (5, 1, 130, 97, False)]
SCALES = (0.3, -0.125, 0.0)
GRADED_SHAPES = [(2, 2, 200, 237, True), (5, 1, 130, 97, False)]
NAMES = ("dq", "dk", "dv")


def shape_id(s):
    return "Hq%d-Hkv%d-Sq%d-Sk%d-%s" % (s[0], s[1], s[2], s[3],
                                         "causal" if s[4] else "full")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _finish(name, q, k, v, dout, causal, scale, o=None, lse=None, **extra):
    """The case dict.  q/k/v/dout are bf16; o (bf16) and lse (fp32) are what
    the kernel is handed: bf16(o64) and fp32(lse64) of the true forward
    unless the builder specifies them, in which case they are the truth.
    g64 is the fp64 backward on the unrounded o64/lse64, A the magnitudes
    of reference.attention_bwd_bound_ref, yard the bf16-emulating yardstick
    on the kernel's inputs.  Computed once and never modified."""
    q64, k64, v64, d64 = q.double(), k.double(), v.double(), dout.double()
    if o is None:
        o64 = ref.attention_ref(q64, k64, v64, causal, scale)
        lse64 = ref.attention_lse_ref(q64, k64, causal, scale)
        o, lse = o64.to(BF), lse64.float()
    else:
        assert o.dtype is BF and lse.dtype is torch.float32
        o64, lse64 = o.double(), lse.double()
    g64 = ref.attention_bwd_ref(q64, k64, v64, o64, lse64, d64, causal, scale)
    bound = ref.attention_bwd_bound_ref(q64, k64, v64, o64, lse64, d64,
                                        causal, scale)
    # 16 fp32 ulps of the exponential's argument, and never more than 1 % of
    # 2^-8: the peaked family (M = 68) would otherwise get 1.7 %
    eps32 = min(EPS32_UNIT * (1.0 + bound["M"]), EPS32_CAP)
    assert eps32 <= 0.01 * U, (name, bound["M"], eps32)
    yard = ref.attention_bwd_ref(q64, k64, v64, o.double(), lse.double(), d64,
                                 causal, scale, emulate_bf16=True)
    c = dict(name=name, q=q, k=k, v=v, dout=dout, o=o, lse=lse, causal=causal,
             scale=scale, g64=g64,
             A=(bound["A_dq"], bound["A_dk"], bound["A_dv"]),
             eps32=eps32, M=bound["M"], yard=yard,
             e_y=tuple((y - t).abs().max().item() for y, t in zip(yard, g64)))
    c.update(extra)
    return c, bound


@functools.lru_cache(maxsize=None)
def random_case(Hq, Hkv, Sq, Sk, causal, D, scale=None, qmul=1.0, seed=11):
    """Plain randn q/k/v and a dout that is independent of o; qmul = 8 is
    the peaked family, `scale` the scale family."""
    g = _gen(seed)
    q = (torch.randn(B, Hq, Sq, D, generator=g) * qmul).to(BF)
    k = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    dout = torch.randn(B, Hq, Sq, D, generator=g).to(BF)
    name = "peaked" if qmul != 1.0 else "random" if scale is None \
        else "scale%g" % scale
    c, _ = _finish(name, q, k, v, dout, causal,
                   1.0 / math.sqrt(D) if scale is None else scale)
    if scale == 0.0:  # nothing flows into q and k: the zero rule applies
        for i in (0, 1):
            assert not (c["A"][i] + c["g64"][i].abs()).any()
    return c


@functools.lru_cache(maxsize=None)
def graded_case(Hq, Hkv, Sq, Sk, causal, D, seed=12):
    """A loss that weighs rows unevenly: row i of dout times 2^-(i mod 12),
    every seventh row exactly 0 (a masked token).  The gradients of one
    tensor then span twelve binades and one global slack checks only the
    largest; dq of a zero row must be exactly 0."""
    g = _gen(seed)
    q = torch.randn(B, Hq, Sq, D, generator=g).to(BF)
    k = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(BF)
    i = torch.arange(Sq)
    w = torch.where(i % 7 == 0, torch.zeros(Sq), 2.0 ** -(i % 12).float())
    dout = (torch.randn(B, Hq, Sq, D, generator=g).to(BF).float()
            * w[:, None]).to(BF)
    c, _ = _finish("graded", q, k, v, dout, causal, 1.0 / math.sqrt(D),
                   zero_rows=i % 7 == 0)
    z = c["zero_rows"]
    assert not c["dout"][:, :, z].any() and bool(c["dout"][:, :, ~z].any())
    assert not (c["A"][0] + c["g64"][0].abs())[:, :, z].any()
    return c


@functools.lru_cache(maxsize=None)
def unit_case(Hq, Hkv, Sq, Sk, causal, D, seed=13):
    """P exactly 1 on every visible pair, everything else small integers,
    so the fp64 gradients are bf16 numbers and any correct kernel returns
    them bit for bit, whatever its tiling or summation order.

    q has one entry of +-1 or +-2 at dim i mod D/2, k one at D/2 + j mod
    D/2: every score is exactly 0.  The kernel is handed lse = 0, so its
    P = exp(0 * scale - 0) is 1 where visible.  v holds integers in [-2, 2],
    the handed o integers in [-1, 1], dout one entry of +-1 at dim i mod D,
    scale is 0.125 at both D.  Then dV counts the visible queries of the
    whole group with signs, dS is an integer in [-3, 3], and dQ, dK are
    0.125 x integers below 256."""
    g = _gen(seed)
    h = D // 2

    def one_hot(H, S, dims, top):
        val = torch.randint(1, top + 1, (B, H, S), generator=g).float()
        sgn = torch.randint(0, 2, (B, H, S), generator=g).float() * 2 - 1
        t = torch.zeros(B, H, S, D)
        t.scatter_(-1, dims.expand(B, H, S).unsqueeze(-1),
                   (val * sgn).unsqueeze(-1))
        return t

    q = one_hot(Hq, Sq, torch.arange(Sq) % h, 2)
    k = one_hot(Hkv, Sk, h + torch.arange(Sk) % h, 2)
    dout = one_hot(Hq, Sq, torch.arange(Sq) % D, 1)
    v = torch.randint(-2, 3, (B, Hkv, Sk, D), generator=g).float()
    o = torch.randint(-1, 2, (B, Hq, Sq, D), generator=g).float()
    lse = torch.zeros(B, Hq, Sq)
    c, bound = _finish("unit", q.to(BF), k.to(BF), v.to(BF), dout.to(BF),
                       causal, 0.125, o=o.to(BF), lse=lse)
    # soundness: what makes the bitwise comparison meaningful
    for t, t16 in ((q, c["q"]), (k, c["k"]), (v, c["v"]), (dout, c["dout"])):
        assert torch.equal(t16.float(), t)
    seen = torch.ones(Sq, Sk, dtype=torch.bool)
    if causal:
        seen = seen.tril(Sk - Sq)
    assert torch.equal(bound["P"], seen.double().expand(B, Hq, Sq, Sk))
    assert c["M"] == 0.0
    dq, dk, dv = c["g64"]
    for t in (dq * 8, dk * 8, dv):
        assert torch.equal(t, t.round()) and t.abs().max() < 256
    g32 = ref.attention_bwd_ref(*(c[n].float() for n in "qkv"), o, lse,
                                dout, causal, 0.125)
    for t64, t32 in zip(c["g64"], g32):
        assert t32.dtype is torch.float32 and torch.equal(t32.double(), t64)
        assert torch.equal(t64.to(BF).double(), t64)
    if Sq > 1 or Sk > 1:
        assert dv.any()
    c["exact"] = tuple(t.to(BF) for t in c["g64"])
    return c


def family_cases(D):
    """(family, shape, case) for every case of the strict tier at head dim
    D, built lazily."""
    for s in SHAPES:
        yield "random", s, random_case(*s, D)
        yield "unit", s, unit_case(*s, D)
    for s in PEAKED_SHAPES:
        yield "peaked", s, random_case(*s, D, qmul=8.0)
    for s in SCALE_SHAPES:
        for sc in SCALES:
            yield "scale", s, random_case(*s, D, scale=sc)
    for s in GRADED_SHAPES:
        yield "graded", s, graded_case(*s, D)


# ------------------------------------------------------------------ the judge

def judge(c, grads, label):
    """Raise AssertionError unless grads = (dq, dk, dv) is a correct
    backward of case c by the rules in the module docstring; returns the
    worst err / tol per tensor and prints them (pytest -s shows them)."""
    ratios = []
    for i, (name, got, want, A) in enumerate(zip(NAMES, grads, c["g64"],
                                                 c["A"])):
        assert tuple(got.shape) == tuple(want.shape), (
            f"{label} {name}: shape {tuple(got.shape)}")
        bits = got.detach().cpu()
        got = bits.double()
        assert torch.isfinite(got).all(), f"{label} {name}: NaN/Inf"
        size = A + want.abs()
        tol = U * size + c["eps32"] * A
        err = (got - want).abs()
        zero = size == 0
        assert bool((got[zero] == 0).all()), (
            f"{label} {name}: {int((got[zero] != 0).sum())} elements that "
            "nothing flows into are not exactly 0")
        ratio = (err[~zero] / tol[~zero]).max().item() if (~zero).any() else 0.0
        ratios.append(ratio)
        print(f"ATTN_BWD_ELEM_RATIO {label} {name} ratio={ratio:.3f} "
              f"max_err={err.max().item():.3e} zero_elems={int(zero.sum())}")
        bad = err > tol
        assert not bad.any(), (
            f"{label} {name}: {int(bad.sum())} of {bad.numel()} elements "
            f"outside 2^-8*(A+|g64|)+eps32*A, worst err/tol {ratio:.3f} at "
            f"{tuple(bad.nonzero()[0].tolist())}")
        if "exact" in c:
            assert bits.dtype is BF, f"{label} {name}: {bits.dtype}"
            diff = bits != c["exact"][i]
            assert not diff.any(), (
                f"{label} {name}: {int(diff.sum())} elements differ from the "
                f"exact result, first at {tuple(diff.nonzero()[0].tolist())}")
    return ratios


def old_rule_accepts(c, grads):
    """The loose tier's rule (test_attention_backward_gpu.py): one number
    per tensor, max err <= 2 * e_y + 2^-8 * max|g64|."""
    for got, want, e_y in zip(grads, c["g64"], c["e_y"]):
        got = got.detach().cpu().double()
        if not torch.isfinite(got).all():
            return False
        if (got - want).abs().max().item() > \
                2.0 * e_y + U * want.abs().max().item():
            return False
    return True


def rejected(c, grads, label="mutant"):
    try:
        judge(c, grads, label)
    except AssertionError:
        return True
    return False


def kernel_like(c):
    """What a correct kernel returns: the yardstick, as bf16."""
    return tuple(t.to(BF) for t in c["yard"])


# ---------------------------------------------------------------- the mutants

def _pairs(Sq, Sk, causal, shift=0):
    """Visible (query, key) pairs [Sq,Sk]."""
    m = torch.ones(Sq, Sk, dtype=torch.bool)
    return m.tril(Sk - Sq + shift) if causal else m


def bwd_vehicle(c, shift=0, dq_pairs=None, kv_pairs=None, drop_head=False,
                delta_swap=False, lse_head0=False, dk_unscaled=False,
                dq_zero_small=False):
    """The kernel's algorithm in fp64 on the kernel's inputs of case c with
    bf16 roundings at its places, and one deliberate defect; with no defect
    it is the yardstick.  dq_pairs / kv_pairs [Sq,Sk] restrict which pairs
    the dQ kernel / the dK-dV kernel visits."""
    q, k, v, o, d = (c[n].double() for n in ("q", "k", "v", "o", "dout"))
    lse = c["lse"].double()
    Bn, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    G, scale = Hq // Hkv, c["scale"]
    rnd = lambda t: t.to(BF).double()
    if lse_head0:
        lse = lse[:, :1].expand(Bn, Hq, Sq)
    delta = (d * o).sum(-1)
    if delta_swap:
        i = torch.arange(Sq) ^ 1
        delta = delta[:, :, torch.where(i < Sq, i, torch.arange(Sq))]
    grp = lambda t: t.reshape(Bn, Hkv, G, *t.shape[2:])
    qg, dg = grp(q), grp(d)
    kg, vg = k.unsqueeze(2), v.unsqueeze(2)
    s = torch.matmul(qg, kg.transpose(-1, -2)) * scale
    seen = _pairs(Sq, Sk, c["causal"], shift)
    p = torch.where(seen, torch.exp(s - grp(lse).unsqueeze(-1)),
                    torch.zeros_like(s))
    dp = torch.matmul(dg, vg.transpose(-1, -2))
    ds = rnd(p * (dp - grp(delta).unsqueeze(-1)))
    p = rnd(p)
    ds_q = ds if dq_pairs is None else ds * dq_pairs
    ds_kv = ds if kv_pairs is None else ds * kv_pairs
    p_kv = p if kv_pairs is None else p * kv_pairs
    if drop_head:
        ds_kv, p_kv = ds_kv[:, :, :-1], p_kv[:, :, :-1]
        qg, dg = qg[:, :, :-1], dg[:, :, :-1]
    dv = torch.matmul(p_kv.transpose(-1, -2), dg).sum(2)
    dk = torch.matmul(ds_kv.transpose(-1, -2), qg).sum(2)
    dk = dk if dk_unscaled else dk * scale
    dq = (torch.matmul(ds_q, kg) * scale).reshape(Bn, Hq, Sq, D)
    if dq_zero_small:
        top = d.abs().amax(-1, keepdim=True)
        dq = torch.where(top < U * top.max(), torch.zeros_like(dq), dq)
    return dq.to(BF), dk.to(BF), dv.to(BF)


def _dims(c):
    return c["q"].shape[2], c["k"].shape[2], c["k"].shape[2] - c["q"].shape[2]


def _m_diagonal_plus_one(c):
    return bwd_vehicle(c, shift=1)


def _m_qb_start_rounded_up(c):
    """dK/dV: qb_start = ceil((k0 - causal_off) / 32), so the slice that
    the diagonal of a 128-key block cuts through is skipped."""
    Sq, Sk, off = _dims(c)
    if not c["causal"]:
        return bwd_vehicle(c)
    t = (torch.arange(Sk) // 128) * 128 - off          # k0 - causal_off
    cut = (t > 0) & (t % 32 != 0)
    skip = cut[None, :] & ((torch.arange(Sq) // 32)[:, None] == (t // 32)[None])
    return bwd_vehicle(c, kv_pairs=~skip)


def _m_dq_limit_one_short(c):
    """dQ: the causal key-tile limit of a 128-row query block one less."""
    Sq, Sk, off = _dims(c)
    if not c["causal"]:
        return bwd_vehicle(c)
    lim = ((torch.arange(Sq) // 128) * 128 + 127 + off + 32) // 32 - 1
    nkb = torch.clamp(lim, max=(Sk + 31) // 32)
    return bwd_vehicle(c, dq_pairs=(torch.arange(Sk) // 32)[None] < nkb[:, None])


def _m_last_query_slice_missing(c):
    Sq, Sk, _ = _dims(c)
    keep = (torch.arange(Sq) < Sq // 32 * 32) | (Sq % 32 == 0)
    return bwd_vehicle(c, kv_pairs=keep[:, None].expand(Sq, Sk))


def _m_last_key_tile_missing(c):
    Sq, Sk, _ = _dims(c)
    keep = (torch.arange(Sk) < Sk // 32 * 32) | (Sk % 32 == 0)
    return bwd_vehicle(c, dq_pairs=keep[None].expand(Sq, Sk))


def _m_group_one_head_short(c):
    return bwd_vehicle(c, drop_head=True)


def _m_delta_of_neighbour_row(c):
    return bwd_vehicle(c, delta_swap=True)


def _m_lse_of_head0(c):
    return bwd_vehicle(c, lse_head0=True)


def _m_dk_without_scale(c):
    return bwd_vehicle(c, dk_unscaled=True)


def _m_dq_zero_on_small_rows(c):
    return bwd_vehicle(c, dq_zero_small=True)


MUTANTS = [_m_diagonal_plus_one, _m_qb_start_rounded_up, _m_dq_limit_one_short,
           _m_last_query_slice_missing, _m_last_key_tile_missing,
           _m_group_one_head_short, _m_delta_of_neighbour_row, _m_lse_of_head0,
           _m_dk_without_scale, _m_dq_zero_on_small_rows]


# -------------------------------------------------- the judge accepts and bites

@pytest.mark.parametrize("D", DS)
def test_bound_ref_is_made_of_what_it_says(D):
    c = random_case(4, 2, 96, 224, True, D)
    args = [c[n].double() for n in "qkv"] + [
        c["o"].double(), c["lse"].double(), c["dout"].double()]
    b = ref.attention_bwd_bound_ref(*args, True, c["scale"])
    Bn, Hq, Sq, Sk = 2, 4, 96, 224
    assert b["P"].shape == (Bn, Hq, Sq, Sk) and b["E_q"].shape == (Bn, Hq, Sq)
    assert all(t.dtype is torch.float64 for n, t in b.items() if n != "M")
    seen = _pairs(Sq, Sk, True)
    assert not b["P"][..., ~seen].any() and bool((b["P"][..., seen] > 0).all())
    assert (b["P"].sum(-1) - 1).abs().max() < 1e-2  # lse is fp32(lse64)
    q, k, v, o, _, d = args
    kk, vv = (t.repeat_interleave(2, 1) for t in (k, v))
    delta = (d * o).sum(-1, keepdim=True)
    ds = b["P"] * (d @ vv.transpose(-1, -2) - delta)
    e_q = (d.abs() * o.abs()).sum(-1)
    assert torch.equal(b["E_q"], e_q)
    ds_abs = ds.abs() + b["P"] * e_q.unsqueeze(-1)
    assert (b["dS_abs"] - ds_abs).abs().max() < 1e-12
    grp = lambda t: t.reshape(Bn, 2, 2, *t.shape[2:]).sum(2)
    a_dv = grp(b["P"].transpose(-1, -2) @ d.abs())
    a_dk = grp(ds_abs.transpose(-1, -2) @ q.abs()) * c["scale"]
    a_dq = (ds_abs @ kk.abs()) * c["scale"]
    for got, want in ((b["A_dv"], a_dv), (b["A_dk"], a_dk), (b["A_dq"], a_dq)):
        assert got.shape == want.shape and (got - want).abs().max() < 1e-12
    # the magnitudes dominate the gradients they bound, and a negative scale
    # changes no magnitude
    for A, g in zip(c["A"], c["g64"]):
        assert bool((A >= g.abs() * (1 - 1e-12)).all())
    neg = ref.attention_bwd_bound_ref(q, -k, v, o, args[4], d, True,
                                      -c["scale"])
    for n in ("P", "A_dq", "A_dk", "A_dv"):
        assert (neg[n] - b[n]).abs().max() < 1e-12
    # (the case's M is taken at the unrounded lse64)
    assert abs(b["M"] - c["M"]) < 1e-5 and 1.0 < b["M"] < 39.0


@pytest.mark.parametrize("D", DS)
def test_judge_accepts_the_yardstick(D):
    """The bf16 yardstick (roundings at the kernel's places, fp64 sums) on
    every case of the tier; its worst err / tol per family is in the module
    docstring.  The fp64 truth itself and its bf16 rounding pass too."""
    worst = {}
    for fam, s, c in family_cases(D):
        label = f"{fam} {shape_id(s)} D{D}"
        r = judge(c, kernel_like(c), "yardstick " + label)
        assert max(r) <= 1.0
        w = worst.setdefault(fam, [0.0, 0.0, 0.0])
        worst[fam] = [max(a, b) for a, b in zip(w, r)]
        if "exact" not in c:
            judge(c, c["g64"], "truth " + label)
        judge(c, tuple(t.to(BF) for t in c["g64"]), "bf16(truth) " + label)
    for fam, w in worst.items():
        print("ATTN_BWD_YARD_WORST D%d %s dq=%.3f dk=%.3f dv=%.3f"
              % (D, fam, *w))
    assert worst["unit"] == [0.0, 0.0, 0.0]


def test_table_reaches_the_paths_it_names():
    """The arithmetic of the kernel's slice skip and key-tile limit on the
    table: the paths each shape is in the table for."""
    def qb_starts(Sq, Sk):
        off = Sk - Sq
        return [max(k0 - off, 0) // 32 for k0 in range(0, Sk, 128)]

    def dq_limits(Sq, Sk):
        return [min((qb * 128 + 127 + Sk - Sq + 32) // 32, (Sk + 31) // 32)
                for qb in range((Sq + 127) // 128)]

    assert qb_starts(200, 237) == [0, 2] and (128 - 37) % 32 != 0
    assert qb_starts(384, 384) == [0, 4, 8]
    assert dq_limits(384, 384) == [4, 8, 12]
    assert qb_starts(33, 300) == [0, 0, 0] and dq_limits(33, 300) == [10]
    assert dq_limits(200, 237) == [6, 8] and (255 + 37 + 32) // 32 > 8
    assert all(s[2] <= 384 and s[3] <= 384 for s in SHAPES)
    assert {s[0] // s[1] for s in SHAPES} == {1, 2, 3, 5}


@pytest.mark.parametrize("D", DS)
def test_mutant_vehicle_reproduces_the_yardstick(D):
    for fam, s, c in family_cases(D):
        for got, want in zip(bwd_vehicle(c), kernel_like(c)):
            assert torch.equal(got, want), (fam, shape_id(s))


# which case is there for which mutant: the table must not lose them
NAMED = [
    (_m_diagonal_plus_one, unit_case, (1, 1, 32, 32, True), {}),
    (_m_diagonal_plus_one, random_case, (2, 2, 200, 237, True), {}),
    (_m_qb_start_rounded_up, unit_case, (2, 2, 200, 237, True), {}),
    (_m_qb_start_rounded_up, random_case, (2, 2, 200, 237, True),
     {"qmul": 8.0}),
    (_m_dq_limit_one_short, unit_case, (2, 2, 384, 384, True), {}),
    (_m_dq_limit_one_short, graded_case, (2, 2, 200, 237, True), {}),
    (_m_last_query_slice_missing, unit_case, (2, 2, 300, 33, False), {}),
    (_m_last_query_slice_missing, random_case, (5, 1, 130, 97, False), {}),
    (_m_last_key_tile_missing, unit_case, (2, 2, 300, 33, False), {}),
    (_m_last_key_tile_missing, graded_case, (5, 1, 130, 97, False), {}),
    (_m_group_one_head_short, unit_case, (6, 2, 160, 160, True), {}),
    (_m_group_one_head_short, random_case, (5, 1, 130, 97, False), {}),
    (_m_delta_of_neighbour_row, unit_case, (2, 2, 129, 129, True), {}),
    (_m_delta_of_neighbour_row, random_case, (6, 2, 160, 160, True), {}),
    (_m_lse_of_head0, random_case, (4, 2, 96, 224, True), {}),
    (_m_lse_of_head0, random_case, (5, 1, 130, 97, False), {"scale": 0.3}),
    (_m_dk_without_scale, unit_case, (5, 1, 130, 97, False), {}),
    (_m_dk_without_scale, random_case, (6, 2, 160, 160, True),
     {"scale": -0.125}),
    (_m_dq_zero_on_small_rows, graded_case, (2, 2, 200, 237, True), {}),
    (_m_dq_zero_on_small_rows, graded_case, (5, 1, 130, 97, False), {}),
]
# (mutant, case) pairs of NAMED that the old max rule accepts, both head dims
OLD_RULE_ACCEPTS = {
    ("dq_limit_one_short", "graded"), ("dq_zero_on_small_rows", "graded")}


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize(
    "mutant,builder,shape,kw", NAMED,
    ids=["%s-%s-%s" % (m.__name__[3:], b.__name__[:-5], shape_id(s))
         for m, b, s, _ in NAMED])
def test_named_case_rejects_the_mutant(mutant, builder, shape, kw, D):
    c = builder(*shape, D, **kw)
    g = mutant(c)
    assert rejected(c, g), (
        f"{mutant.__name__[3:]} survives {c['name']} {shape_id(shape)} D{D}")
    old = old_rule_accepts(c, g)
    print(f"ATTN_BWD_MUTANT {mutant.__name__[3:]} {c['name']} "
          f"{shape_id(shape)} D{D}: old rule "
          f"{'ACCEPTS' if old else 'rejects'}")
    assert old == ((mutant.__name__[3:], c["name"]) in OLD_RULE_ACCEPTS)


@pytest.mark.parametrize("D", DS)
def test_only_the_graded_family_sees_small_rows_zeroed(D):
    """Where the old rule goes blind: dq zeroed on the rows whose dout is
    below 2^-8 of the largest passes max err <= 2*e_y + 2^-8*max|g64| on
    every case of the tier, and the per-element bound on all but graded."""
    for fam, s, c in family_cases(D):
        g = _m_dq_zero_on_small_rows(c)
        assert old_rule_accepts(c, g), (fam, shape_id(s))
        assert rejected(c, g) == (fam == "graded"), (fam, shape_id(s))


def test_judge_rejects_nan_inf_shapes_and_single_elements():
    c = graded_case(5, 1, 130, 97, False, 64)
    good = kernel_like(c)
    judge(c, good, "sane")

    def with_(i, idx, val=None, add=None):
        g = [t.clone() for t in good]
        g[i][idx] = val if val is not None else g[i][idx] + add
        return g

    for i in range(3):
        for bad in (float("nan"), float("inf")):
            assert rejected(c, with_(i, (1, 0, 5, 7), bad))
        g = list(good)
        g[i] = g[i][:, :, :-1]
        assert rejected(c, g)
    # ONE small element of a tensor whose largest are 2^11 times larger:
    # row 11 of dout carries 2^-11, its dq with it
    i = (0, 3, 11, int(c["g64"][0][0, 3, 11].abs().argmax()))
    small = c["g64"][0][i].abs().item()
    assert small < 2.0 ** -8 * c["g64"][0].abs().max().item()
    g = with_(0, i, add=4 * small)
    assert rejected(c, g) and old_rule_accepts(c, g)
    # a zero row of dout: nothing but 0 passes
    assert bool(c["zero_rows"][7])
    assert rejected(c, with_(0, (1, 2, 7, 0), val=2.0 ** -30))
    # the exact family: one ulp of one element
    u = unit_case(2, 2, 1, 33, True, 128)
    good = kernel_like(u)
    judge(u, good, "unit")
    g = [t.clone() for t in good]
    nz = g[2].nonzero()[0]
    bits = g[2].view(torch.int16)
    bits[tuple(nz)] ^= 1
    assert rejected(u, g)
    assert rejected(u, [t.float() for t in good])  # bitwise means bf16
