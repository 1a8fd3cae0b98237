"""Chunks that see their context (mc_extend_rows) against the two ways the calls before it give the same cache and pick:
  (a) steps:   one ragged step (mc_ragged_step) per chunk token, the rows in lockstep, a row idle once its chunk is through;
  (b) prefill: mc_rows_prefill of context + chunk from position 0, one call per row where the sum exceeds max_seq_len.
Llama-3-8B widths, int4 g128 synthetic weights, B = 8 rows, max_seq_len 2048.  The variants alternate inside every repetition; each
ends with a host sync and is timed between two; median, minimum and maximum of REPS after a warm-up round.
usage: python tools/rows_extend_bench.py [--reps N] [--out profiles/rows_extend_bench.json] [--once SHAPE]
  --once SHAPE: the context, a warm-up and ONE mc_extend_rows call of that shape, nothing else -- for a kernel trace (MC_PX_KEYS=0
  in the environment: the same call with no tile's keys split)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metalchat_amd as mc

SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
B, S = 8, 2048
# (chunk lengths, context lengths); 0 = the row is not in the call
CASES = {
    "8x16@1900": ([16] * B, [1900] * B),
    "8x64@1024": ([64] * B, [1024] * B),
    "2x256@1536": ([256, 0, 0, 256, 0, 0, 0, 0], [1536, 0, 0, 1536, 0, 0, 0, 0]),
    "mixed": ([2, 130, 17, 64, 33, 100, 16, 48], [1900, 100, 1500, 700, 1024, 1800, 300, 1200]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", default=None, choices=sorted(CASES))
    ap.add_argument("--cases", default=None, help="comma-separated subset of the shapes")
    a = ap.parse_args()
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **SHAPE)
    dec.init_synthetic(1)
    batch = mc.Batch(dec, B)
    rng = np.random.default_rng(0)

    def ids(n):
        return rng.integers(0, SHAPE["vocab"], n).astype(np.int32)

    def one_row(r, tokens):
        call = [None] * B
        call[r] = tokens
        batch.prefill_rows(call)

    def make(lens, ctx):
        context = [ids(c) if n else None for n, c in zip(lens, ctx)]
        chunks = [ids(n) if n else None for n in lens]
        for r in range(B):  # the rows' contexts (the cache contents do not matter to the time, the lengths do)
            if lens[r]:
                one_row(r, context[r])
        return context, chunks

    def extend(lens, ctx, context, chunks):
        batch.extend_rows(chunks, ctx)

    def steps(lens, ctx, context, chunks):
        for i in range(max(lens)):
            tok = np.array([chunks[r][i] if i < lens[r] else 0 for r in range(B)], np.int32)
            pos = np.array([ctx[r] + i if i < lens[r] else -1 for r in range(B)], np.int32)
            batch.step_rows(tok, pos)

    def prefill(lens, ctx, context, chunks):
        whole = [np.concatenate([context[r], chunks[r]]) if lens[r] else None for r in range(B)]
        if sum(len(w) for w in whole if w is not None) <= S:
            batch.prefill_rows(whole)
            return
        for r in range(B):
            if lens[r]:
                one_row(r, whole[r])

    if a.once:
        lens, ctx = CASES[a.once]
        context, chunks = make(lens, ctx)
        extend(lens, ctx, context, chunks)  # warm-up: allocations, code load
        extend(lens, ctx, context, chunks)
        print(f"one mc_extend_rows call of {a.once} done (MC_PX_KEYS={os.environ.get('MC_PX_KEYS', 'unset')})")
        return

    variants = (("extend", extend), ("steps", steps), ("prefill", prefill))
    results = []
    for name in (a.cases.split(",") if a.cases else CASES):
        lens, ctx = CASES[name]
        context, chunks = make(lens, ctx)
        row = dict(case=name, lens=lens, context=ctx, rows=int(sum(lens)))
        ts = {label: [] for label, _ in variants}
        for rep in range(a.reps + 1):  # (round 0: the warm-up)
            for label, fn in variants:
                t0 = time.perf_counter()
                fn(lens, ctx, context, chunks)
                if rep:
                    ts[label].append((time.perf_counter() - t0) * 1e3)
        for label, _ in variants:
            row[label + "_ms"] = round(float(np.median(ts[label])), 3)
            row[label + "_ms_min"] = round(min(ts[label]), 3)
            row[label + "_ms_max"] = round(max(ts[label]), 3)
        best = min(row["steps_ms"], row["prefill_ms"])
        spread = max(row[v + "_ms_max"] - row[v + "_ms_min"] for v in ("extend", "steps", "prefill"))
        row["best_other_ms"] = best
        row["speedup"] = round(best / row["extend_ms"], 2)
        row["condition_met"] = bool(row["extend_ms"] < best - spread)  # below the smaller of (a), (b) by more than any min-max spread
        print(f"{name:11s} {row['rows']:4d} rows: extend {row['extend_ms']:8.2f} ms   steps {row['steps_ms']:8.2f} ms   "
              f"prefill {row['prefill_ms']:8.2f} ms   x{row['speedup']:.2f}   condition met: {row['condition_met']}", flush=True)
        results.append(row)
    doc = dict(model="Llama-3-8B widths, 32 layers, int4 g128, synthetic weights", B=B, max_seq_len=S, device=acc.name(),
               key_ranges=os.environ.get("MC_PX_KEYS", "the host's rule"),
               timing="median, min and max of %d calls per variant, the variants alternating, after one warm-up round; each call ends "
                      "with a host sync" % a.reps, results=results)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
