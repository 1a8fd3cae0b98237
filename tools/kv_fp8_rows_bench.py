"""The packed passes on an fp8 batch (mc_kv_packed_set, Part 2p) against the same calls on a bfloat16 batch of the same build.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 rows, both batches over one decoder.  Three cases:
  extend   mc_extend_rows, 8 rows x 16 tokens behind 1900 keys
  verify   mc_verify_rows of the same chunks
  prefill  mc_rows_prefill, 8 prompts x 256 tokens at position 0
Every call ends with a host synchronisation and is timed between two.  A process warms each case up once and takes the median of REPS
calls per case and format, the two formats alternating call by call.  The figures are the median of the medians of PROCS fresh processes
with [min, max] over them.  "faster" / "slower": the fp8 median differs from the bfloat16 median by more than the larger min-max spread of
the two; else "equal".  Prints one JSON line and writes it to --out (default profiles/kv_fp8_rows_bench.json).

usage: python tools/kv_fp8_rows_bench.py [--procs N] [--reps N] [--layers N] [--out FILE]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, B, CTX, CHUNK, PROMPT = 2048, 8, 1900, 16, 256
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
CASES, FORMATS = ("extend", "verify", "prefill"), ("bf16", "fp8")


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
    batches = {}
    for kv in FORMATS:
        b = batches[kv] = mc.Batch(dec, B, wide=True, kv=kv)
        b.set_kv_packed(True)
        for r in range(B):   # the rows' contexts (the cache contents do not matter to the time, the lengths do)
            b.prefill_rows([ids(CTX) if q == r else None for q in range(B)])
    chunks, prompts, ctx = [ids(CHUNK) for _ in range(B)], [ids(PROMPT) for _ in range(B)], [CTX] * B
    calls = dict(extend=lambda b: b.extend_rows(chunks, ctx), verify=lambda b: b.verify_rows(chunks, ctx), prefill=lambda b: b.prefill_rows(prompts))
    out = {}
    for case in CASES:   # (prefill last: it rewinds every row to 256)
        ts = {kv: [] for kv in FORMATS}
        for rep in range(reps + 1):   # (round 0 warms up)
            for kv in FORMATS:
                t0 = time.perf_counter()
                calls[case](batches[kv])
                if rep:
                    ts[kv].append((time.perf_counter() - t0) * 1e3)
        out[case] = {kv: statistics.median(ts[kv]) for kv in FORMATS}
    print("RESULT " + json.dumps(dict(device=acc.name(), ms=out)), flush=True)


def main():
    reps, layers, procs = int(arg("--reps", 7)), int(arg("--layers", SHAPE["n_layers"])), int(arg("--procs", 5))
    if "--child" in sys.argv:
        return child(reps, layers)
    runs = []
    for _ in range(procs):   # fresh processes, one at a time
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps), "--layers", str(layers)], capture_output=True,
                           text=True, timeout=600)
        if p.returncode != 0:
            sys.exit(f"a measuring process ended with status {p.returncode}:\n{p.stderr[-2000:]}")
        runs.append(json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:]))
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
    out = dict(metric="kv_fp8_rows", model="llama3-8b-int4-g128-synthetic", S=S, B=B, context=CTX, chunk=CHUNK, prompt=PROMPT, layers=layers,
               processes=procs, reps=reps, rows=rows, device=runs[0]["device"])
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "kv_fp8_rows_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
