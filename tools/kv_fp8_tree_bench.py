"""mc_tree_verify on an fp8 batch (mc_kv_tree_set, Part 2q) against the same call on a bfloat16 batch of the same build.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 rows, both batches over one decoder.  One case:
  tree     mc_tree_verify, 8 rows x a branching tree of 16 nodes behind 1900 keys.  Three calls in front of the timed ones put each batch's own
           picks on the path 0 -> 2 -> 5 -> 11, so every timed call accepts at least three drafts off the first chain and its compaction moves them
Every call ends with a host synchronisation and is timed between two.  A process warms each case up once and takes the median of REPS
calls per case and format, the two formats alternating call by call.  The figures are the median of the medians of PROCS fresh processes
with [min, max] over them.  "faster" / "slower": the fp8 median differs from the bfloat16 median by more than the larger min-max spread of
the two; else "equal".  Prints one JSON line and writes it to --out (default profiles/kv_fp8_tree_bench.json).

usage: python tools/kv_fp8_tree_bench.py [--procs N] [--reps N] [--layers N] [--out FILE]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, B, CTX = 2048, 8, 1900
TREE = [-1, 0, 0, 1, 1, 2, 2, 3, 5, 5, 8, 5, 11, 0, 13, 11]
PATH = [0, 2, 5, 11]
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
CASES, FORMATS = ("tree",), ("bf16", "fp8")


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(reps, layers):
    """one process: {case: {format: median ms}} as a JSON line"""
    import numpy as np

    import metalchat_amd as mc

    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **dict(SHAPE, n_layers=layers))
    dec.init_synthetic(1)
    rng = np.random.default_rng(0)
    ids = lambda n: rng.integers(0, SHAPE["vocab"], n).astype(np.int32)
    batches, trees = {}, {}
    parents, ctx = [np.array(TREE, np.int32)] * B, [CTX] * B
    for kv in FORMATS:
        b = batches[kv] = mc.Batch(dec, B, wide=True, kv=kv)
        b.set_kv_packed(True)
        b.set_kv_tree(True)
        for r in range(B):   # the rows' contexts (the cache contents do not matter to the time, the lengths do)
            b.prefill_rows([ids(CTX) if q == r else None for q in range(B)])
        t = trees[kv] = [ids(len(TREE)) for _ in range(B)]
        for d in range(1, len(PATH)):   # the batch's own pick after the path's node at depth d - 1 becomes the node at depth d
            picks = b.verify_tree(t, parents, ctx)[2]
            for r in range(B):
                t[r][PATH[d]] = picks[r][PATH[d - 1]]
        assert min(b.verify_tree(t, parents, ctx)[0]) >= len(PATH) - 1
    calls = dict(tree=lambda b, kv: b.verify_tree(trees[kv], parents, ctx))
    out = {}
    for case in CASES:
        ts = {kv: [] for kv in FORMATS}
        for rep in range(reps + 1):   # (round 0 warms up)
            for kv in FORMATS:
                t0 = time.perf_counter()
                calls[case](batches[kv], kv)
                if rep:
                    ts[kv].append((time.perf_counter() - t0) * 1e3)
        out[case] = {kv: statistics.median(ts[kv]) for kv in FORMATS}
    print("RESULT " + json.dumps(dict(device=acc.name(), ms=out)), flush=True)


def main():
    reps, layers, procs = int(arg("--reps", 7)), int(arg("--layers", SHAPE["n_layers"])), int(arg("--procs", 5))
    if "--child" in sys.argv:
        return child(reps, layers)
    runs = []
    for i in range(procs):   # fresh processes, one at a time
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps), "--layers", str(layers)], capture_output=True,
                           text=True, timeout=600)
        if p.returncode != 0:
            sys.exit(f"a measuring process ended with status {p.returncode}:\n{p.stderr[-2000:]}")
        runs.append(json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:]))
        print(f"process {i + 1} of {procs}: {runs[-1]['ms']}", file=sys.stderr, flush=True)
    rows = {}
    for case in CASES:
        row = {}
        for kv in FORMATS:
            ts = [r["ms"][case][kv] for r in runs]
            row[kv] = dict(ms=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))
        spread = max(row[kv]["max"] - row[kv]["min"] for kv in FORMATS)
        diff = row["fp8"]["ms"] - row["bf16"]["ms"]
        row["fp8_vs_bf16"] = dict(difference_ms=round(diff, 3), larger_spread_ms=round(spread, 3),
                                  verdict="equal" if abs(diff) <= spread else ("faster" if diff < 0 else "slower"))
        rows[case] = row
    out = dict(metric="kv_fp8_tree", model="llama3-8b-int4-g128-synthetic", S=S, B=B, context=CTX, nodes=len(TREE), path=PATH, layers=layers,
               processes=procs, reps=reps, rows=rows, device=runs[0]["device"])
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "kv_fp8_tree_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
