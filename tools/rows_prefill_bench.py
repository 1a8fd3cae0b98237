"""The packed prompt pass (mc_rows_prefill) against the sequential loop it replaces (mc_decoder_prefill + mc_batch_fork per prompt),
Llama-3-8B widths, int4 g128 synthetic weights, B = 8 rows.  Each call returns after a host sync, so both are timed between two
syncs; median of REPS after a warm-up.
usage: python tools/rows_prefill_bench.py [--reps N] [--out profiles/rows_prefill_bench.json] [--once SHAPE]
  --once SHAPE: one packed call of that shape (8x64, 8x128, 8x256, mixed) after a warm-up, nothing else -- for a kernel trace"""
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
B = 8
CASES = {
    "8x64": [64] * B,
    "8x128": [128] * B,
    "8x256": [256] * B,
    "mixed": [33, 250, 97, 180, 64, 211, 45, 128],  # 1008 rows
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", default=None, choices=sorted(CASES))
    a = ap.parse_args()
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=2048, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **SHAPE)
    dec.init_synthetic(1)
    batch = mc.Batch(dec, B)
    rng = np.random.default_rng(0)
    if a.once:
        prompts = [rng.integers(0, SHAPE["vocab"], n).astype(np.int32) for n in CASES[a.once]]
        batch.prefill_rows(prompts)  # warm-up: allocations, code load, derived weight copies
        batch.prefill_rows(prompts)
        print(f"one packed call of {a.once} done")
        return

    def packed(prompts):
        batch.prefill_rows(prompts)

    def sequential(prompts):
        for r, p in enumerate(prompts):
            dec.prefill(p, 0)
            batch.fork(r, len(p))

    results = []
    for name, lens in CASES.items():
        prompts = [rng.integers(0, SHAPE["vocab"], n).astype(np.int32) for n in lens]
        row = dict(case=name, lens=lens, rows=int(sum(lens)))
        for label, fn in (("sequential", sequential), ("packed", packed)):
            fn(prompts)  # warm-up
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn(prompts)
                ts.append((time.perf_counter() - t0) * 1e3)
            row[label + "_ms"] = round(float(np.median(ts)), 3)
            row[label + "_ms_all"] = [round(t, 3) for t in ts]
        row["speedup"] = round(row["sequential_ms"] / row["packed_ms"], 3)
        print(f"{name:6s} {row['rows']:5d} rows: sequential {row['sequential_ms']:8.2f} ms   packed {row['packed_ms']:8.2f} ms   "
              f"x{row['speedup']:.2f}", flush=True)
        results.append(row)
    doc = dict(model="Llama-3-8B widths, 32 layers, int4 g128, synthetic weights", B=B, max_seq_len=2048, device=acc.name(),
               timing="median of %d calls after one warm-up; each call ends with a host sync" % a.reps, results=results)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
