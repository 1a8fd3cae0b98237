"""fp8 KV caches (mc_kv_batch_create, Part 2o): what a ragged step costs on an fp8 batch against the same step on a bfloat16 batch.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 and B = 64.  A prompt pass of 2028 tokens fills the decoder's cache and is
forked into every row of two batches per B (the fp8 fork quantises).  A sample is 16 mc_ragged_step calls with every row at position 2028,
each ending in its own host synchronisation; the four variants alternate in one process: a warm-up round, then 5 timed rounds; median, min
and max of ms per step.  "faster": the fp8 median is below the bfloat16 median by more than the larger min-max spread of the two.
kv_bytes: what mc_kv_batch_bytes reports for each batch.
Prints one JSON line and writes it to --out (default profiles/kv_fp8_bench.json).

usage: python tools/kv_fp8_bench.py [--out FILE] [--layers N]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metalchat_amd as mc

S, CONTEXT, STEPS, ROUNDS = 2048, 2028, 16, 5
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
SIZES = [8, 64]


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    shape = dict(SHAPE, n_layers=int(arg("--layers", SHAPE["n_layers"])))
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **shape)
    dec.init_synthetic(1)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, shape["vocab"], CONTEXT).astype(np.int32), 0)
    tokens = rng.integers(0, shape["vocab"], 64).astype(np.int32)
    variants, kv_bytes = {}, {}
    for B in SIZES:
        for kv in ("bf16", "fp8"):
            batch = mc.Batch(dec, B, wide=True, kv=kv)
            for r in range(B):
                batch.fork(r, CONTEXT)
            kv_bytes[f"{kv}_{B}"] = batch.kv_bytes

            def run(b=batch):
                for _ in range(STEPS):
                    b.step_rows(tokens[:b.B], [CONTEXT] * b.B)   # (ends with a host synchronisation)
            variants[f"{kv}_{B}"] = run
    times = {k: [] for k in variants}
    for rnd in range(ROUNDS + 1):
        for name, run in variants.items():
            t0 = time.perf_counter()
            run()
            if rnd:   # (round 0 warms up)
                times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
    rows = {name: dict(B=int(name.split("_")[1]), ms_per_step=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4),
                       kv_bytes=kv_bytes[name]) for name, ts in times.items()}
    out = dict(metric="kv_fp8_step", model="llama3-8b-int4-g128-synthetic", S=S, context=CONTEXT, layers=shape["n_layers"], steps=STEPS, rounds=ROUNDS,
               rows=rows, device=acc.name())
    for B in SIZES:
        a, b = rows[f"bf16_{B}"], rows[f"fp8_{B}"]
        spread = max(a["max"] - a["min"], b["max"] - b["min"])
        out[f"b{B}_fp8_vs_bf16"] = dict(difference_ms=round(b["ms_per_step"] - a["ms_per_step"], 4), larger_spread_ms=round(spread, 4),
                                       faster=bool(a["ms_per_step"] - b["ms_per_step"] > spread))
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "kv_fp8_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
