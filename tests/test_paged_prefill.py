"""Paged prefill attention without a GPU: the reference against dense causal
attention and against the decode lane, the CPU dispatch of F.paged_prefill,
the engine's prefill_attn="paged" lane token for token, and the comparator
floor of the GPU cases in test_paged_prefill_gpu.py."""
import math

import pytest
import torch

import modal_examples_amd.ops.functional as F
import modal_examples_amd.ops.reference as ref
from modal_examples_amd.models.llama.engine import BLOCK, LlamaEngine
from modal_examples_amd.models.llama.model import LlamaConfig
from test_kernel_edges_gpu import BF16_TOL, FP8_TOL, _err_ratio
from test_paged_prefill_gpu import ALL_CASES, _prefill_case


def _paged(pairs, Hkv, G, D, block_size, dtype, seed=0):
    """A ragged batch of (n_b, S_b) through a shuffled table; also returns
    each sequence's dense K/V [Hkv, S_b, D]."""
    g = torch.Generator().manual_seed(seed)
    need = [max(1, (S + block_size - 1) // block_size) for _, S in pairs]
    nblocks = sum(need) + 3
    perm = torch.randperm(nblocks, generator=g)
    kc = torch.randn(nblocks, Hkv, block_size, D, generator=g).to(dtype)
    vc = torch.randn(nblocks, Hkv, block_size, D, generator=g).to(dtype)
    bt = torch.zeros(len(pairs), max(need) + 1, dtype=torch.int32)
    dense, at = [], 0
    for b, (_, S) in enumerate(pairs):
        idx = perm[at: at + need[b]]
        at += need[b]
        bt[b, : need[b]] = idx.int()
        dense.append(tuple(c[idx].transpose(0, 1).reshape(Hkv, -1, D)[:, :S]
                           for c in (kc, vc)))
    cu = [0]
    for n, _ in pairs:
        cu.append(cu[-1] + n)
    q = torch.randn(cu[-1], Hkv * G, D, generator=g).to(dtype)
    return (q, kc, vc, bt, torch.tensor(cu, dtype=torch.int32),
            torch.tensor([S for _, S in pairs], dtype=torch.int32), dense)


def test_reference_equals_dense_causal_attention():
    """Per sequence, paged_prefill_ref is attention_ref(causal) with Sq = n_b
    and Sk = S_b, in fp64."""
    pairs = [(5, 5), (17, 40), (1, 33), (0, 9), (12, 12), (3, 64)]
    for D, G, bs in ((64, 1, 16), (32, 3, 5)):
        q, kc, vc, bt, cu, lens, dense = _paged(pairs, 2, G, D, bs,
                                                torch.float64)
        got = ref.paged_prefill_ref(q, kc, vc, bt, cu, lens, bs)
        assert got.dtype == torch.float64 and got.shape == q.shape
        for b, (n, S) in enumerate(pairs):
            if n == 0:
                continue
            k, v = dense[b]
            qb = q[cu[b]: cu[b + 1]].transpose(0, 1)[None]  # [1,Hq,n,D]
            want = ref.attention_ref(qb, k[None], v[None], causal=True)
            torch.testing.assert_close(got[cu[b]: cu[b + 1]],
                                       want[0].transpose(0, 1),
                                       atol=1e-12, rtol=1e-12)


def test_reference_equals_decode_lane_for_single_tokens():
    pairs = [(1, 1), (1, 16), (1, 17), (1, 50)]
    q, kc, vc, bt, cu, lens, _ = _paged(pairs, 2, 2, 64, 16, torch.float32)
    got = ref.paged_prefill_ref(q, kc, vc, bt, cu, lens, 16, 0.2)
    want = ref.paged_decode_ref(q, kc, vc, bt, lens, 16, 0.2)
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)


def test_reference_edge_cases():
    """n_b = 0 sequences own no rows; S_b < n_b zeroes the rows whose
    position would be negative and leaves the rest causal."""
    pairs = [(0, 20), (6, 4), (0, 0), (2, 7)]
    q, kc, vc, bt, cu, lens, dense = _paged(pairs, 2, 2, 32, 4, torch.float64)
    got = ref.paged_prefill_ref(q, kc, vc, bt, cu, lens, 4)
    assert got.shape[0] == 8 and torch.isfinite(got).all()
    assert (got[0:2] == 0).all()  # positions -2 and -1
    k, v = dense[1]
    want = ref.attention_ref(q[2:6].transpose(0, 1)[None], k[None], v[None],
                             causal=True)[0].transpose(0, 1)
    torch.testing.assert_close(got[2:6], want, atol=1e-12, rtol=1e-12)
    assert (got[6:8] != 0).any()


def test_cpu_dispatch_takes_the_reference():
    pairs = [(4, 9), (7, 7)]
    q, kc, vc, bt, cu, lens, _ = _paged(pairs, 2, 2, 64, 16, torch.bfloat16)
    want = ref.paged_prefill_ref(q, kc, vc, bt, cu, lens, 16)
    assert torch.equal(F.paged_prefill(q, kc, vc, bt, cu, lens, 16), want)
    # max_q_len sizes the GPU grid; the CPU path has no use for it
    assert torch.equal(
        F.paged_prefill(q, kc, vc, bt, cu, lens, 16, max_q_len=1), want)
    # fp8 caches are widened: the result is the reference on the dequantised
    # values
    k8, v8 = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
    want8 = ref.paged_prefill_ref(q, k8.float(), v8.float(), bt, cu, lens, 16)
    assert torch.equal(F.paged_prefill(q, k8, v8, bt, cu, lens, 16), want8)
    with pytest.raises(ValueError, match="block_table"):
        F.paged_prefill(q, kc, vc, None, cu, lens, 16)


def test_gpu_wrapper_arguments(monkeypatch):
    """What the extension is handed: a contiguous table (an expand()ed one
    would be read out of bounds), int32 cu_q/seq_lens, and max_q_len = T when
    the caller gives none."""
    seen = {}

    class FakeExt:
        @staticmethod
        def paged_prefill(q, k, v, bt, cu, lens, bs, scale, max_q_len):
            seen.update(bt=bt, cu=cu, lens=lens, bs=bs, scale=scale,
                        max_q_len=max_q_len)
            return torch.zeros_like(q)

    monkeypatch.setattr(F, "_ext_for", lambda *a: FakeExt())
    q = torch.randn(11, 4, 64).to(torch.bfloat16)
    kc = torch.randn(3, 2, 16, 64).to(torch.bfloat16)
    bt = torch.zeros(1, 4, dtype=torch.int32).expand(2, -1)
    cu, lens = torch.tensor([0, 5, 11]), torch.tensor([5, 30])
    F.paged_prefill(q, kc, kc, bt, cu, lens, 16)
    assert seen["bt"].is_contiguous() and seen["bt"].shape == (2, 4)
    assert seen["cu"].dtype == torch.int32 and seen["lens"].dtype == torch.int32
    assert seen["max_q_len"] == 11 and seen["bs"] == 16
    assert seen["scale"] == 1.0 / math.sqrt(64)
    F.paged_prefill(q, kc, kc, bt, cu, lens, 16, scale=0.3, max_q_len=6)
    assert seen["max_q_len"] == 6 and seen["scale"] == 0.3


# ------------------------------------------------------------------ engine

def _engine(**kw):
    return LlamaEngine(LlamaConfig.small(), device="cpu", dtype=torch.float32,
                       use_graph=False, eos_id=-1, seed=0, kv_blocks=256, **kw)


def _generate(eng, prompts, n=6):
    outs = []
    for p in prompts:
        rid = eng.add_request(p, max_new_tokens=n, temperature=0.0)
        while eng.has_work:
            eng.step()
        outs.append(eng.finished[rid].out_tokens)
    return outs


@pytest.mark.parametrize("chunk", [8, 40])
def test_engine_chunked_prefill_paged_lane(chunk):
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, 1024, (100,), generator=g).tolist()
    mono = _generate(_engine(), [prompt])
    dec = _generate(_engine(chunked_prefill=chunk), [prompt])
    pag = _generate(_engine(chunked_prefill=chunk, prefill_attn="paged"),
                    [prompt])
    assert pag == dec == mono


def test_engine_prefix_cache_paged_lane():
    g = torch.Generator().manual_seed(6)
    system = torch.randint(0, 1024, (3 * BLOCK,), generator=g).tolist()
    prompts = [system + [7, 8, 9], system + [11, 12]]
    cold = _generate(_engine(), prompts)
    dec = _generate(_engine(prefix_cache=True), prompts)
    eng = _engine(prefix_cache=True, prefill_attn="paged")
    assert _generate(eng, prompts) == dec == cold
    assert eng.prefix_hit_tokens == 3 * BLOCK


def test_engine_fp8_kv_paged_lane_matches_decode_lane():
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(0, 1024, (45,), generator=g).tolist()
    kw = dict(kv_dtype="fp8", chunked_prefill=16)
    assert (_generate(_engine(prefill_attn="paged", **kw), [prompt])
            == _generate(_engine(**kw), [prompt]))


def test_engine_rejects_unknown_prefill_attn():
    with pytest.raises(ValueError, match="prefill_attn"):
        _engine(prefill_attn="nope")
    assert _engine().prefill_attn == "decode"


# ------------------------------------------------------- comparator floor

def _kernel_rounding_model(c):
    """The kernel's roundings on exact arithmetic otherwise: scores and
    exp(s - m) in f32, l summed in f32 from the unrounded P, P rounded to
    bf16 before PV, the output rounded to bf16."""
    Hkv, G = c.kc.shape[1], c.q.shape[1] // c.kc.shape[1]
    D, bs = c.q.shape[2], c.block_size
    kf, vf = c.kc.float(), c.vc.float()
    out = torch.zeros(c.q.shape, dtype=torch.bfloat16)
    for b, (n, prefix) in enumerate(c.pairs):
        if n == 0:
            continue
        S, lo = n + prefix, int(c.cu[b])
        idx = c.bt[b, : (S + bs - 1) // bs].long()
        k = kf[idx].transpose(0, 1).reshape(Hkv, -1, D)[:, :S]
        v = vf[idx].transpose(0, 1).reshape(Hkv, -1, D)[:, :S]
        qb = c.q[lo: lo + n].float().transpose(0, 1).reshape(Hkv, G, n, D)
        s = torch.matmul(qb, k[:, None].transpose(-1, -2)) * c.sc
        seen = (torch.arange(S)[None, :]
                <= torch.arange(prefix, S)[:, None])
        s = s.masked_fill(~seen, float("-inf"))
        p = torch.exp(s - s.amax(-1, keepdim=True))
        l = p.sum(-1, keepdim=True)
        o = torch.matmul(p.bfloat16().float(), v[:, None]) / l
        out[lo: lo + n] = o.reshape(Hkv * G, n, D).transpose(0, 1).bfloat16()
    return out


def test_comparator_floor():
    """What the number formats alone cost on every GPU case: the rounding
    model above against the fp64 reference, as a fraction of the bound.  The
    tolerances must sit at least 4x above it, which leaves the kernel's fast
    exp, defer-max and summation order the room they are given elsewhere in
    this project."""
    worst = {False: 0.0, True: 0.0}
    for case in ALL_CASES:
        c = _prefill_case(*case)
        tol = FP8_TOL if c.fp8 else BF16_TOL
        f = float(_err_ratio(_kernel_rounding_model(c), c.want, *tol).max())
        worst[c.fp8] = max(worst[c.fp8], f)
    print(f"comparator floor: bf16 cache {worst[False]:.4f}, fp8 cache "
          f"{worst[True]:.4f} of the bound")
    assert max(worst.values()) <= 0.25
