#!/usr/bin/env python3
"""Filtered sampling on MI355X: the engine's sort-based nucleus path against
the radix-select path of `F.sample_batch`.

Three comparisons on float32 logits [64, 128256] and [256, 128256]:

  (i)   the parent nucleus path (the body of `LlamaEngine._sample_rows` at
        top_p = 0.9, copied below so that it stays the yardstick whatever the
        engine does later) against `F.sample_batch(top_p=0.9)`;
  (ii)  the same parent path against `F.sample_batch(top_k=50, top_p=0.9)`
        (the parent has no top-k: its nucleus path is the nearest it offers);
  (iii) `F.sample` against unfiltered `F.sample_batch` with every parameter
        a device tensor, as the engine passes them.

Method: every variant is warmed up, then timed with device events over
`--iters` calls per window; the two sides of a comparison alternate window by
window in one process, `--repeats` windows each, and the table gives the
median and the min..max spread of the per-call time.  The parent path contains
a host synchronisation (`(temps <= 0).all()`), which the event window
includes, as an engine step does.  Token agreement between the two sides
under one seed is printed next to the times (T = 1, so the scores are formed
identically and only the nucleus boundary can differ).

Needs a GPU; there is no CPU fallback for a timing.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import modal_examples_amd.ops.functional as F  # noqa: E402

VOCAB = 128256


def parent_sample_rows(logits, temps, top_p, seed):
    """LlamaEngine._sample_rows of the parent commit, verbatim but for
    `self`."""
    temps = temps.to(logits.device)
    greedy = logits.argmax(-1).int()
    if (temps <= 0).all():
        return greedy
    scaled = logits / temps.clamp_min(1e-5).unsqueeze(-1)
    if top_p < 1.0:
        # nucleus filter: mask tokens outside the top-p probability mass
        sorted_logits, idx = scaled.sort(-1, descending=True)
        probs = torch.softmax(sorted_logits.float(), -1)
        cum = probs.cumsum(-1)
        drop_sorted = cum - probs > top_p  # keep first token crossing p
        drop = torch.zeros_like(drop_sorted).scatter(-1, idx, drop_sorted)
        scaled = scaled.masked_fill(drop, float("-inf"))
    sampled = F.sample(scaled, 1.0, seed=seed)
    return torch.where(temps <= 0, greedy, sampled.to(greedy.device))


def window(fn, iters):
    """Per-call milliseconds of `iters` back-to-back calls (device events)."""
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def compare(name, old, new, iters, repeats, warmup):
    for _ in range(warmup):
        old()
        new()
    torch.cuda.synchronize()
    t_old, t_new = [], []
    for _ in range(repeats):  # alternate the two sides
        t_old.append(window(old, iters))
        t_new.append(window(new, iters))
    a, b = old(), new()
    agree = float((a == b).float().mean())
    mo, mn = statistics.median(t_old), statistics.median(t_new)
    return (f"{name:34s} {mo:9.4f} [{min(t_old):.4f}..{max(t_old):.4f}]  "
            f"{mn:9.4f} [{min(t_new):.4f}..{max(t_new):.4f}]  "
            f"{mo / mn:7.2f}x  {100 * agree:6.2f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--vocab", type=int, default=VOCAB)
    ap.add_argument("--out", default=None, help="also write the table here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampling needs a GPU: timings are not taken on a CPU")
    lines = [f"# sampling: parent path vs F.sample_batch on "
             f"{torch.cuda.get_device_name(0)}; per-call ms, median "
             f"[min..max] over {args.repeats} alternating windows of "
             f"{args.iters} calls (device events)",
             f"{'comparison':34s} {'old ms':>9s} {'':19s} {'new ms':>9s} "
             f"{'':19s} {'old/new':>8s}  {'same token':>9s}"]
    seed = 1234
    for rows in args.rows:
        g = torch.Generator(device="cuda").manual_seed(rows)
        x = 2.0 * torch.randn(rows, args.vocab, device="cuda", generator=g)
        temps = torch.ones(rows, device="cuda")
        ctr = torch.arange(rows, device="cuda")
        seeds = torch.full((rows,), seed, dtype=torch.int64, device="cuda")
        tag = f"[{rows}x{args.vocab}]"
        lines.append(compare(
            f"(i)   nucleus .9 {tag}",
            lambda: parent_sample_rows(x, temps, 0.9, seed),
            lambda: F.sample_batch(x, temps, top_p=0.9, seeds=seed, counters=ctr),
            args.iters, args.repeats, args.warmup))
        lines.append(compare(
            f"(ii)  + top_k 50 {tag}",
            lambda: parent_sample_rows(x, temps, 0.9, seed),
            lambda: F.sample_batch(x, temps, top_k=50, top_p=0.9, seeds=seed,
                                   counters=ctr),
            args.iters, args.repeats, args.warmup))
        lines.append(compare(
            f"(iii) unfiltered {tag}",
            lambda: F.sample(x, 1.0, seed=seed),
            lambda: F.sample_batch(x, temps, seeds=seeds, counters=ctr),
            args.iters, args.repeats, args.warmup))
        # the cutoff kernel alone, against itself for the spread
        cut = lambda: F.sampling_cutoff(x, temps, top_p=0.9)  # noqa: E731
        lines.append(compare(f"      cutoff kernel alone {tag}", cut, cut,
                             args.iters, args.repeats, args.warmup))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
