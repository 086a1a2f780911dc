#!/usr/bin/env python3
"""Decode throughput of speculative decoding under spec_attn="rows" (k+1 rows
of the paged decode kernel per request) and "packed" (the packed multi-token
decode kernel): Llama-3-8B shapes, random weights, bf16, spec_tokens=4 with
oracle drafts, so every verify step carries full runs of 5 positions.

One engine, one process: the lane is switched between runs, so both lanes
use the same weights, and the runs alternate.  Per batch size, every lane
first learns its own greedy answer (the oracle): a run without drafts, then
runs drafted with the previous answer until the answer repeats.  The
repetition matters with random weights: their logits are nearly flat, and
the GEMMs of a 5-row verify step round differently from those of a 1-row
step, so the undrafted answer is not quite what a drafted run emits.  Each
lane is then timed with its answer as its drafts; the share of drafts
accepted is reported beside the rate.  The clock starts once
every request has its first token (prefill is the same under both lanes) and
stops after a device synchronise at the end; tokens/s counts the tokens
emitted in between.

Usage: python scripts/bench_spec_packed_engine.py [--layers N] [--reps R]
           [--batches 1,8,64] [--context 4096] [--new 60]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from modal_examples_amd.models.llama.engine import LlamaEngine  # noqa: E402
from modal_examples_amd.models.llama.model import LlamaConfig  # noqa: E402

LANES = ("rows", "packed")
KEY = 16  # prompt tokens that identify a request to the oracle


def run(eng, prompts, new, oracle):
    """Greedy answers, decode seconds, decode tokens, verify steps and the
    share of drafts accepted."""
    prop0, acc0 = eng.spec_proposed, eng.spec_accepted
    eng._propose = lambda r: (oracle[tuple(r.prompt[:KEY])][
        len(r.out_tokens): len(r.out_tokens) + eng.spec_tokens]
        if oracle else [])
    rids = [eng.add_request(p, max_new_tokens=new, temperature=0.0)
            for p in prompts]
    live = {r.req_id: r for r in list(eng.waiting) + list(eng.running)}
    assert len(live) == len(rids)
    while any(not r.out_tokens for r in live.values()):
        eng.step()  # prefill: every request gets its first token
    torch.cuda.synchronize()
    before = sum(len(r.out_tokens) for r in live.values())
    steps, t0 = 0, time.perf_counter()
    while eng.has_work:
        eng.step()
        steps += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    outs = [eng.finished[i].out_tokens for i in rids]
    assert all(len(o) == new for o in outs), [eng.finished[i].error
                                              for i in rids]
    share = (eng.spec_accepted - acc0) / max(1, eng.spec_proposed - prop0)
    return outs, dt, sum(len(o) for o in outs) - before, steps, share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0,
                    help="truncate the model (0 = all 32 layers)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--context", type=int, default=4096)
    ap.add_argument("--new", type=int, default=60)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU lanes"
    cfg = LlamaConfig.llama3_8b()
    if args.layers:
        cfg.n_layers = args.layers
    batches = [int(b) for b in args.batches.split(",")]
    per_seq = (args.context + args.new + 8) // 16 + 2
    torch.manual_seed(0)
    eng = LlamaEngine(cfg, device="cuda", dtype=torch.bfloat16,
                      max_batch=max(batches), use_graph=False, eos_id=-1,
                      kv_blocks=max(batches) * per_seq + 8, spec_tokens=4,
                      spec_attn="packed")
    g = torch.Generator().manual_seed(0)
    results = {"model": f"llama3_8b shapes, {cfg.n_layers} layers, bf16, "
                        f"context {args.context}, spec_tokens 4, oracle "
                        f"drafts, {args.new} new tokens per request"}
    for B in batches:
        prompts = [torch.randint(0, cfg.vocab_size, (args.context,),
                                 generator=g).tolist() for _ in range(B)]
        oracle, answers = {}, {}
        for lane in LANES:
            eng.spec_attn = lane
            outs = run(eng, prompts, args.new, None)[0]
            for _ in range(5):
                answers[lane] = outs
                oracle[lane] = {tuple(p[:KEY]): a
                                for p, a in zip(prompts, outs)}
                outs = run(eng, prompts, args.new, oracle[lane])[0]
                if outs == answers[lane]:
                    break
        best = {lane: None for lane in LANES}
        for _ in range(args.reps):
            for lane in LANES:
                eng.spec_attn = lane
                outs, dt, toks, steps, share = run(eng, prompts, args.new,
                                                   oracle[lane])
                if best[lane] is None or dt < best[lane][0]:
                    best[lane] = (dt, toks, steps, share,
                                  outs == answers[lane])
        r = {}
        for lane in LANES:
            dt, toks, steps, share, same = best[lane]
            r[lane] = {"decode_s": round(dt, 4), "tokens": toks,
                       "verify_steps": steps,
                       "drafts_accepted": round(share, 3),
                       "emits_its_oracle": same,
                       "tokens_per_s": round(toks / dt, 1),
                       "ms_per_step": round(dt / steps * 1e3, 3)}
        r["packed_over_rows_tokens_per_s"] = round(
            r["packed"]["tokens_per_s"] / r["rows"]["tokens_per_s"], 3)
        r["lanes_same_tokens"] = answers["rows"] == answers["packed"]
        results[f"batch_{B}"] = r
        print(f"batch_{B}", json.dumps(r), flush=True)
    print(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()
