"""Multi-LoRA delta on the GPU (csrc/lora.hip): exact integer cases bit for
bit, random cases element by element against lora_bound_ref, row
independence, graph replay, launcher errors, and the engine's adapter lane.

What each shape (N, K, O, S, R) reaches.  The shrink loop runs 64-wide
chunks over a K-slice: a body of two chunks while more than two remain, then
a tail of two chunks or of one; K is cut into min(16, ceil(K/512)) slices of
whole chunks.  Expand blocks are 128 columns; align strides rows by 256 and
adapters by 8.

  (1, 64, 128, 1, 16)       1 slice of 1 chunk: no body, tail of one; one
                            column block; one row, one adapter
  (37, 128, 384, 4, 32)     2 chunks: no body, tail of two; three column blocks
  (37, 192, 128, 2, 16)     3 chunks: one body trip, tail of one
  (1, 256, 128, 2, 32)      4 chunks: one body trip, tail of two
  (37, 320, 128, 32, 64)    5 chunks: two body trips, tail of one; S = 32:
                            empty adapters, pad-slot loop trips 2..4
  (260, 384, 256, 3, 16)    6 chunks: two body trips, tail of two; N > 256:
                            second trip of align's row loops; ~65 rows per
                            adapter: segments of three M-tiles
  (260, 1024, 128, 32, 32)  2 even slices of 8 chunks
  (37, 1088, 128, 2, 64)    17 chunks in 3 slices of 6, 6 and 5: uneven last
"""
import functools

import pytest
import torch

from modal_examples_amd.models.llama.engine import LlamaEngine
from modal_examples_amd.ops import functional as OF
from modal_examples_amd.ops import reference as ref
from test_lora import CFG, PROMPT, adapter_state

pytestmark = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda"
SHAPES = [(1, 64, 128, 1, 16), (37, 128, 384, 4, 32), (37, 192, 128, 2, 16),
          (1, 256, 128, 2, 32), (37, 320, 128, 32, 64),
          (260, 384, 256, 3, 16), (260, 1024, 128, 32, 32),
          (37, 1088, 128, 2, 64)]


def _sparse(g, shape, nnz, values):
    """Rows of zeros with nnz entries drawn from `values` along the last dim."""
    out = torch.zeros(shape)
    pos = torch.rand(shape, generator=g).argsort(-1)[..., :nnz]
    pick = values[torch.randint(len(values), pos.shape, generator=g)]
    return out.scatter_(-1, pos, pick)


@functools.lru_cache(maxsize=None)
def case(shape, exact):
    """(y0, x, bank_a, bank_b, idx) on the CPU in bf16 (idx int32, about a
    fifth of the rows without adapter, the first row always with one).
    exact: small-integer x, sparse integer A, sparse B in {-1, 0, 1} * 2^-j —
    every t and every output is exactly representable in bf16."""
    N, K, O, S, R = shape
    g = torch.Generator().manual_seed(sum(shape) + exact)
    idx = torch.randint(-1, S, (N,), generator=g)
    idx[torch.rand(N, generator=g) < 0.1] = -1
    idx[0] = S - 1
    if exact:
        x = torch.randint(-2, 3, (N, K), generator=g).float()
        a = _sparse(g, (S, R, K), 4, torch.tensor([-1.0, 1.0]))
        b = _sparse(g, (S, O, R), 2,
                    torch.tensor([1.0, -1.0, 0.5, -0.5, 0.25, -0.25]))
        y = torch.randint(-3, 4, (N, O), generator=g).float()
    else:
        x = torch.randn(N, K, generator=g)
        a = torch.randn(S, R, K, generator=g) * K ** -0.5
        b = torch.randn(S, O, R, generator=g) * 0.5
        y = torch.randn(N, O, generator=g)
    bf = torch.bfloat16
    out = (y.to(bf), x.to(bf), a.to(bf), b.to(bf), idx.to(torch.int32))
    if exact:
        want = ref.lora_apply_ref(*(t.double() for t in out[:4]), out[4])
        assert torch.equal(want, want.bfloat16().double()), "case not exact"
    return out


def run_gpu(y, x, a, b, idx):
    """ops.lora_apply_ on GPU copies of a case -> the updated y on the CPU."""
    yd, S = y.to(DEV), a.shape[0]
    OF.lora_apply_(yd, x.to(DEV), a.to(DEV), b.to(DEV),
                   OF.lora_schedule(idx.to(DEV), S))
    return yd.cpu()


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_exact(shape):
    c = case(shape, True)
    want = ref.lora_apply_ref(*(t.double() for t in c[:4]), c[4]).bfloat16()
    assert torch.equal(run_gpu(*c), want)


@requires_gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_bounded(shape):
    c = case(shape, False)
    want, tol = ref.lora_bound_ref(*c)
    err = (run_gpu(*c).double() - want).abs()
    on = tol > 0
    print(f"{shape}: worst err/tol {(err[on] / tol[on]).max().item():.3f}")
    assert (err <= tol).all()


@requires_gpu
@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[5], SHAPES[7]])
def test_rows(shape):
    y, x, a, b, idx = c = case(shape, False)
    got = run_gpu(*c)
    assert torch.equal(run_gpu(*c), got)           # reproducible
    off = idx < 0
    assert off.any() and torch.equal(got[off].view(torch.int16),
                                     y[off].view(torch.int16))
    for n in (0, len(idx) // 2, len(idx) - 1):     # a row alone = in the batch
        alone = run_gpu(y[n:n + 1], x[n:n + 1], a, b, idx[n:n + 1])
        assert torch.equal(alone[0], got[n]), n
    none = torch.full_like(idx, -1)
    assert torch.equal(run_gpu(y, x, a, b, none).view(torch.int16),
                       y.view(torch.int16))


@requires_gpu
def test_graph_replay():
    shape = SHAPES[5]
    y0, x, a, b, idx = (t.to(DEV) for t in case(shape, False))
    y, S = torch.empty_like(y0), a.shape[0]

    def step():
        y.copy_(y0)
        OF.lora_apply_(y, x, a, b, OF.lora_schedule(idx, S))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for seed in range(3):  # new adapters and inputs in place, then replay
        g = torch.Generator().manual_seed(seed)
        idx.copy_(torch.randint(-1, S, idx.shape, generator=g).to(DEV))
        x.copy_(torch.randn(x.shape, generator=g).to(DEV))
        graph.replay()
        got = y.clone()
        step()
        assert torch.equal(got, y), seed


@requires_gpu
def test_launcher_errors():
    y, x, a, b, idx = (t.to(DEV) for t in case(SHAPES[1], False))
    sched = OF.lora_schedule(idx, 4)
    bad = [(y, x, a[:, :8].contiguous(), b[:, :, :8].contiguous(), sched),
           (y, x[:, :96].contiguous(), a[:, :, :96].contiguous(), b, sched),
           (y[:, :64].contiguous(), x, a, b[:, :64].contiguous(), sched),
           (y, x, a.repeat(9, 1, 1), b.repeat(9, 1, 1), sched),
           (y[:, ::2], x, a, b[:, ::2], sched),
           (y, x.float(), a, b, sched),
           (y[:5], x[:5], a, b, sched)]
    for args in bad:
        with pytest.raises(ValueError):
            OF.lora_apply_(*args)
    with pytest.raises(RuntimeError):  # the extension's own checks
        OF._ext_for(y).lora_apply_(y[:5], x[:5], a, b, sched.sched)
    empty = OF.lora_schedule(idx[:0], 4)
    assert OF.lora_apply_(y[:0], x[:0], a, b, empty).shape == (0, y.shape[1])


@requires_gpu
@pytest.mark.parametrize("lane", [{}, {"weight_dtype": "int4"},
                                  {"spec_tokens": 2}])
def test_engine_mixed_batch_matches_solo(lane):
    torch.manual_seed(0)
    eng = LlamaEngine(CFG, device="cuda", max_batch=8, kv_blocks=256,
                      use_graph=True, lora_slots=4, **lane)
    eng.load_adapter("a", adapter_state(CFG, 10, r=8))
    eng.load_adapter("b", adapter_state(CFG, 11, r=16))
    jobs = [(PROMPT, None), (PROMPT, "a"), (PROMPT[:9], "b"), (PROMPT[:23], "a")]

    def serve(batch):
        rids = []
        for p, name in batch:  # one prefill per step, then a shared decode
            rids.append(eng.add_request(p, max_new_tokens=6, adapter=name))
            eng.step()
        eng.run_until_done()
        return [eng.finished[r].out_tokens for r in rids]

    solo = [serve([j])[0] for j in jobs]
    assert serve(jobs) == solo
    assert solo[1] != solo[0]
    eng.close()
