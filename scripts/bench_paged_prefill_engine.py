#!/usr/bin/env python3
"""Time-to-first-token of the engine's two cached-prefix prefill lanes under
prefill_attn="decode" (C decode rows per chunk) and "paged" (the MFMA paged
prefill kernel): Llama-3-8B shapes, random weights, bf16, one process, the
two engines alternating after a warm-up of each.

  (a) an 8192-token prompt with chunked_prefill=512
  (b) a prefix-cache hit on 2048 tokens followed by a 2048-token suffix

Usage: python scripts/bench_paged_prefill_engine.py [--layers N] [--reps R]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from modal_examples_amd.models.llama.engine import LlamaEngine  # noqa: E402
from modal_examples_amd.models.llama.model import LlamaConfig  # noqa: E402

LANES = ("decode", "paged")


def ttft(eng, prompt):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rid = eng.add_request(prompt, max_new_tokens=1, temperature=0.0)
    while eng.has_work:
        eng.step()
    torch.cuda.synchronize()
    r = eng.finished[rid]
    assert r.out_tokens, r.error
    return time.perf_counter() - t0, r.out_tokens[0]


def run(name, engines, prompts, results):
    """prompts[0] warms every engine; the rest are timed, lanes alternating."""
    times = {lane: [] for lane in LANES}
    same = 0
    for i, p in enumerate(prompts):
        toks = {}
        for lane in LANES:
            dt, toks[lane] = ttft(engines[lane], p)
            if i:
                times[lane].append(dt)
        same += i > 0 and toks["decode"] == toks["paged"]
    r = {f"{lane}_ttft_s": [round(t, 4) for t in times[lane]] for lane in LANES}
    r["speedup_of_best"] = round(min(times["decode"]) / min(times["paged"]), 2)
    r["first_token_equal"] = f"{same}/{len(prompts) - 1}"
    results[name] = r
    print(name, json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=0,
                    help="truncate the model (0 = all 32 layers)")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU lanes"
    cfg = LlamaConfig.llama3_8b()
    cfg.max_seq = 16384  # the default 8192 would cut the 8192-token prompt
    if args.layers:
        cfg.n_layers = args.layers
    g = torch.Generator().manual_seed(0)

    def rand_prompt(n):
        return torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()

    def engines(**kw):
        out = {}
        for lane in LANES:
            torch.manual_seed(0)
            out[lane] = LlamaEngine(cfg, device="cuda", dtype=torch.bfloat16,
                                    use_graph=False, eos_id=-1, kv_blocks=4096,
                                    prefill_attn=lane, **kw)
        return out

    results = {"model": f"llama3_8b shapes, {cfg.n_layers} layers, bf16"}
    engs = engines(chunked_prefill=512)
    run("chunked_8192_by_512", engs,
        [rand_prompt(8192) for _ in range(args.reps + 1)], results)
    del engs
    torch.cuda.empty_cache()
    engs = engines(prefix_cache=True)
    system = rand_prompt(2048)
    run("prefix_hit_2048_suffix_2048", engs,
        [system + rand_prompt(2048) for _ in range(args.reps + 1)], results)
    results["prefix_hit_tokens"] = {lane: engs[lane].prefix_hit_tokens
                                    for lane in LANES}
    print(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()
