"""Batched decode throughput (mc_batch_*): Llama-3-8B int4 g128, synthetic weights, S = 2048.

A 2028-token prompt pass fills the decoder's cache and is forked into every row; for B in 1, 2, 4, 8 one mc_batch_generate of
20 lockstep steps (positions 2028 .. 2047) is timed between two synchronisations, after one untimed call.  For comparison the
batch-1 decoder's mc_decoder_generate of 20 tokens from the same position, in the same process.  Prints one JSON line.
usage: python tools/batch_bench.py [--out FILE] [--only B]   (--only: that batch size alone, e.g. under a kernel trace)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metalchat_amd as mc

S, PROMPT, STEPS, REPS = 2048, 2028, 20, 3
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
HBM_TBPS = 8.0


def timed(fn):
    fn()  # untimed: first-use costs
    best = None
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()  # (ends with a host synchronisation)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **SHAPE)
    dec.init_synthetic(1)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, SHAPE["vocab"], PROMPT).astype(np.int32), 0)
    wbytes = dec.weight_bytes()
    L, KV, hd = SHAPE["n_layers"], SHAPE["n_kv_heads"], SHAPE["head_dim"]
    kv_row = 2 * L * KV * hd * 2 * (PROMPT + STEPS // 2)  # K and V of one row at the mean context of the 20 steps
    rows = []
    sizes = [int(sys.argv[sys.argv.index("--only") + 1])] if "--only" in sys.argv else [1, 2, 4, 8]
    for B in sizes:
        batch = mc.Batch(dec, B)
        for r in range(B):
            batch.fork(r, PROMPT)
        first = rng.integers(0, SHAPE["vocab"], B).astype(np.int32)
        dt = timed(lambda: batch.generate(first, PROMPT, STEPS))
        ms = dt * 1e3 / STEPS
        by = wbytes + B * kv_row
        rows.append(dict(B=B, ms_per_step=round(ms, 4), tokens_per_s=round(B * STEPS / dt, 1), bytes_per_step=by,
                         frac_of_8tbps=round(by / (ms * 1e-3) / (HBM_TBPS * 1e12), 4)))
        batch.release()
    dt1 = timed(lambda: dec.generate(7, PROMPT, STEPS))
    base = STEPS / dt1
    for r in rows:
        r["x_batch1_decoder"] = round(r["tokens_per_s"] / base, 3)
    out = dict(metric="batch_decode", model="llama3-8b-int4-g128-synthetic", S=S, context=PROMPT, steps=STEPS,
               batch1_decoder_tokens_per_s=round(base, 1), batch1_decoder_ms_per_token=round(dt1 * 1e3 / STEPS, 4),
               weight_bytes=wbytes, rows=rows, device=acc.name())
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
