"""Ragged batched decode (mc_ragged_*): Llama-3-8B int4 g128, synthetic weights, S = 2048, B = 8.

A 2028-token prompt pass fills the decoder's cache and is forked into all 8 rows before each case.  Four calls of 20 chained steps each:
  (a) lockstep   mc_batch_generate at 2028
  (b) ragged     every row at 2028 (the same work as (a), with mc_b_rows_begin for mc_step_set)
  (c) ragged     row r at 1028 + 128 r (rows rewind into the forked prompt; mean context 1476)
  (d) ragged     rows 0-3 at 2028, rows 4-7 idle
Each is timed as the best of 3 after one untimed call, every call ending with a host synchronisation.  Prints one JSON line
and writes it to --out (default profiles/ragged_decode_bench.json).
usage: python tools/ragged_bench.py [--out FILE] [--only a|b|c|d]   (--only: that call alone, e.g. under a kernel trace)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metalchat_amd as mc

S, PROMPT, STEPS, REPS, B = 2048, 2028, 20, 3, 8
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
CASES = {
    "a": ("lockstep", [PROMPT] * B),
    "b": ("ragged_equal", [PROMPT] * B),
    "c": ("ragged_spread", [1028 + 128 * r for r in range(B)]),
    "d": ("ragged_half_idle", [PROMPT] * 4 + [-1] * 4),
}


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
    batch = mc.Batch(dec, B)
    first = rng.integers(0, SHAPE["vocab"], B).astype(np.int32)
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    rows = {}
    for key, (name, pos) in CASES.items():
        if only and key != only:
            continue
        for r in range(B):  # every case starts from the forked prompt (a ragged call shortens the rows it rewinds)
            batch.fork(r, PROMPT)
        if key == "a":
            fn = lambda: batch.generate(first, PROMPT, STEPS)  # noqa: E731
        else:
            fn = lambda pos=pos: batch.generate_rows(first, pos, STEPS)  # noqa: E731
        dt = timed(fn)
        active = sum(p >= 0 for p in pos)
        rows[key] = dict(case=name, positions=pos, active_rows=active, ms_per_step=round(dt * 1e3 / STEPS, 4),
                         tokens_per_s=round(active * STEPS / dt, 1))
    for key in ("b", "c", "d"):
        if key in rows and "a" in rows:
            rows[key]["x_lockstep_ms_per_step"] = round(rows[key]["ms_per_step"] / rows["a"]["ms_per_step"], 4)
    out = dict(metric="ragged_decode", model="llama3-8b-int4-g128-synthetic", S=S, prompt=PROMPT, steps=STEPS, batch=B,
               cases=rows, device=acc.name())
    batch.release()
    dec.release()
    line = json.dumps(out)
    print(line)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ragged_decode_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
