"""Rolling rows (mc_rolling_set): what a ragged step costs once every row has rolled, against the same step at the last linear
position.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 (mc_batch_create) and B = 64 (mc_wide_batch_create).  A prompt pass of
S - 1 tokens fills the decoder's cache and is forked into every row of two batches per B:
  edge    rolling off, every row stepped at S - 1 (its length becomes S; the next step at S - 1 is a rewind by one, which a row of
          length S still takes) -- the last position a batch reaches without rolling: kv_len = S, mc_b_rows_begin
  rolled  rolling on, three untimed steps take every row past the end, then every row stepped at its length -- kv_len = S over the
          same kernels, mc_b_rows_begin_rolling (which also writes the rope rows) for mc_b_rows_begin
Both are single mc_ragged_step calls, 20 to a sample, each ending in its own host synchronisation; the variants alternate in one
process: a warm-up round, then 5 timed rounds; median, min and max of ms per step.  "equal": the medians differ by less than the
larger min-max spread of the two.
--edge-only: the edge variant alone -- runs on a build without Part 2j, to compare the default path across builds;
--parent FILE: the JSON line such a run wrote, merged in as `parent_edge` with the same comparison against this build's edge.
Prints one JSON line and writes it to --out (default profiles/rolling_rows_bench.json).

usage: python tools/rolling_rows_bench.py [--out FILE] [--edge-only] [--parent FILE] [--layers N]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metalchat_amd as mc

S, STEPS, ROUNDS = 2048, 20, 5
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
SIZES = [8, 64]


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def forked(dec, B, rolling):
    batch = mc.Batch(dec, B, wide=B > 8)
    for r in range(B):
        batch.fork(r, S - 1)
    if rolling:
        batch.set_rolling(True)
    return batch


def compare(a, b):
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    return dict(difference_ms=round(b["ms_per_step"] - a["ms_per_step"], 4), larger_spread_ms=round(spread, 4),
                equal=bool(abs(b["ms_per_step"] - a["ms_per_step"]) < spread))


def main():
    edge_only = "--edge-only" in sys.argv
    shape = dict(SHAPE, n_layers=int(arg("--layers", SHAPE["n_layers"])))
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **shape)
    dec.init_synthetic(1)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, shape["vocab"], S - 1).astype(np.int32), 0)
    tokens = rng.integers(0, shape["vocab"], 64).astype(np.int32)
    variants, rolled_batches = {}, {}
    for B in SIZES:
        edge = forked(dec, B, False)

        def run_edge(b=edge):
            for _ in range(STEPS):
                b.step_rows(tokens[:b.B], [S - 1] * b.B)   # (ends with a host synchronisation)
        variants[f"edge_{B}"] = run_edge
        if edge_only:
            continue
        rolled = forked(dec, B, True)
        rolled.generate_rows(tokens[:B], [S - 1] * B, 3)
        rolled_batches[B] = rolled

        def run_rolled(b=rolled):
            for _ in range(STEPS):
                b.step_rows(tokens[:b.B], b.lengths())
        variants[f"rolled_{B}"] = run_rolled
    times = {k: [] for k in variants}
    for rnd in range(ROUNDS + 1):
        for name, run in variants.items():
            t0 = time.perf_counter()
            run()
            if rnd:   # (round 0 warms up)
                times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
    rows = {name: dict(B=int(name.split("_")[1]), ms_per_step=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))
            for name, ts in times.items()}
    out = dict(metric="rolling_rows_step", model="llama3-8b-int4-g128-synthetic", S=S, layers=shape["n_layers"], steps=STEPS, rounds=ROUNDS,
               rows=rows, device=acc.name())
    if not edge_only:
        for B in SIZES:
            assert min(rolled_batches[B].lengths()) > S + ROUNDS * STEPS   # every timed step ran past the end
            out[f"b{B}_rolled_vs_edge"] = compare(rows[f"edge_{B}"], rows[f"rolled_{B}"])
    parent = arg("--parent")
    if parent:
        with open(parent) as f:
            prows = json.loads(f.readline())["rows"]
        out["parent_edge"] = {k: v for k, v in prows.items() if k.startswith("edge_")}
        for B in SIZES:
            out[f"b{B}_edge_vs_parent_edge"] = compare(prows[f"edge_{B}"], rows[f"edge_{B}"])
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "rolling_rows_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
