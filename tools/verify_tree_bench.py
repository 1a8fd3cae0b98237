"""Speculative verify over a draft tree (mc_tree_verify) against mc_verify_rows of the same lengths, in one process.

Llama-3-8B widths, int4 g128 synthetic weights, B = 8 rows, max_seq_len 2048, 16 nodes per row behind 1900 keys.  Alternating inside
every repetition:
  verify        mc_verify_rows of 16-token chunks: the yardstick (this call is what it was before mc_tree_verify existed)
  tree_chain    mc_tree_verify of the same chunks as chain trees: the same bits, plus the walk and a compaction launch that moves nothing
  tree_binary   mc_tree_verify of a binary tree (node i's parent is (i - 1) // 2) with random tokens: nothing is accepted
  tree_accept   the same tree whose right children carry the target's own picks: the path 0, 2, 6, 14 is accepted and the compaction
                moves three slots per row in every layer
Synthetic weights give a draft no agreement with its target: this reports what the tree form costs, not acceptance rates.
Each call ends with a host sync and is timed between two; median, minimum and maximum of REPS after a warm-up round.
Under `rocprofv3 --kernel-trace --stats -- python tools/verify_tree_bench.py --reps 2` (a run of its own) the kernel statistics show
the accept and compaction launches' own times.

usage: python tools/verify_tree_bench.py [--reps N] [--out profiles/verify_tree_bench.json]"""
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
B, S, CTX, N = 8, 2048, 1900, 16


def stats(ts):
    return round(float(np.median(ts)), 3), round(float(min(ts)), 3), round(float(max(ts)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **SHAPE)
    dec.init_synthetic(1)
    batch = mc.Batch(dec, B)
    rng = np.random.default_rng(0)
    ids = lambda n: rng.integers(0, SHAPE["vocab"], n).astype(np.int32)
    for r in range(B):  # the rows' contexts (the cache contents do not matter to the time, the lengths do)
        call = [None] * B
        call[r] = ids(CTX)
        batch.prefill_rows(call)
    ctx = np.full(B, CTX, np.int32)
    chain = [np.arange(-1, N - 1, dtype=np.int32)] * B
    binary = [np.array([-1] + [(i - 1) // 2 for i in range(1, N)], np.int32)] * B
    chunks = [ids(N) for _ in range(B)]
    # the accepting tree: level by level the right child (2 i + 2) of every node takes the target's pick after the node
    good = [c.copy() for c in chunks]
    for level in range(4):
        _, _, picks, _ = batch.verify_tree(good, binary, ctx)
        for r in range(B):
            for i in range(N):
                if 2 * i + 2 < N:
                    good[r][2 * i + 2] = picks[r][i]
    accepted, _, _, paths = batch.verify_tree(good, binary, ctx)
    print("accepting tree: accepted", list(accepted), "path of row 0", list(paths[0]), flush=True)
    if not all(list(p) == [0, 2, 6, 14] for p in paths):
        print("warning: not every row accepts the path 0, 2, 6, 14:", [list(p) for p in paths], flush=True)

    variants = (("verify", lambda: batch.verify_rows(chunks, ctx)), ("tree_chain", lambda: batch.verify_tree(chunks, chain, ctx)),
                ("tree_binary", lambda: batch.verify_tree(chunks, binary, ctx)), ("tree_accept", lambda: batch.verify_tree(good, binary, ctx)))
    ts = {label: [] for label, _ in variants}
    for rep in range(a.reps + 1):  # (round 0: the warm-up)
        for label, fn in variants:
            t0 = time.perf_counter()
            fn()
            if rep:
                ts[label].append((time.perf_counter() - t0) * 1e3)
    row = dict(nodes=N, rows=N * B)
    for label, _ in variants:
        row[label + "_ms"], row[label + "_ms_min"], row[label + "_ms_max"] = stats(ts[label])
    spread = max(row[v + "_ms_max"] - row[v + "_ms_min"] for v, _ in variants)
    row["largest_min_max_spread_ms"] = round(spread, 3)
    for label in ("tree_chain", "tree_binary", "tree_accept"):
        row[label + "_minus_verify_ms"] = round(row[label + "_ms"] - row["verify_ms"], 3)
    print("  ".join(f"{v} {row[v + '_ms']:.3f} ms ({row[v + '_ms_min']:.3f} - {row[v + '_ms_max']:.3f})" for v, _ in variants), flush=True)
    doc = dict(model="Llama-3-8B widths, 32 layers, int4 g128, synthetic weights", B=B, max_seq_len=S, context=CTX, device=acc.name(),
               timing="median, min and max of %d calls per variant, the variants alternating, after one warm-up round; each call ends with "
                      "a host sync" % a.reps, results=[row])
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
