"""Shared-prefix rows (mc_prefix_*): what a ragged step costs when every row attends ONE copy of its prompt, against the same rows
holding full copies.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 (mc_batch_create) and B = 64 (mc_wide_batch_create).  A prompt pass of
1920 tokens fills the decoder's cache; per B two batches:
  full      every row forked from the decoder (its own copy of the 1920 positions)
  attached  the 1920 positions forked ONCE into the shared prefix (shared = 1920), every row attached
Both then take 108 untimed chained steps with the same tokens, so every row sits at position 2028 behind 108 slots of its own, and the
timed region is single mc_ragged_step calls at position 2028, 20 to a sample, each ending in its own host synchronisation.  The variants
alternate in one process: a warm-up round, then 5 timed rounds; median, min and max of ms per step.  "faster": the attached median is
below the full one by more than the larger min-max spread of the two.
--full-only: the full variant alone -- runs on a build without Part 2r, to compare the default path across builds;
--parent FILE: the JSON line such a run wrote, merged in as `parent_full` with the same comparison against this build's full;
--only NAME: one variant alone (full_64, attached_64, ...), one sample and no file -- the process to put a kernel trace around.
Prints one JSON line and writes it to --out (default profiles/prefix_rows_bench.json).

usage: python tools/prefix_rows_bench.py [--out FILE] [--full-only] [--parent FILE] [--only NAME] [--layers N]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metalchat_amd as mc

S, PREFIX, POS, STEPS, ROUNDS = 2048, 1920, 2028, 20, 5
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
SIZES = [8, 64]


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def rows_at_pos(dec, B, attached, tokens):
    batch = mc.Batch(dec, B, wide=B > 8)
    if attached:
        batch.prefix_fork(PREFIX)
    for r in range(B):
        batch.attach_row(r) if attached else batch.fork(r, PREFIX)
    batch.generate_rows(tokens[:B], [PREFIX] * B, POS - PREFIX)
    assert list(batch.lengths()) == [POS] * B
    return batch


def compare(a, b):
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    diff = b["ms_per_step"] - a["ms_per_step"]
    return dict(difference_ms=round(diff, 4), larger_spread_ms=round(spread, 4), equal=bool(abs(diff) < spread), faster=bool(-diff > spread))


def main():
    full_only, only = "--full-only" in sys.argv, arg("--only")
    shape = dict(SHAPE, n_layers=int(arg("--layers", SHAPE["n_layers"])))
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **shape)
    dec.init_synthetic(1)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, shape["vocab"], PREFIX).astype(np.int32), 0)
    tokens = rng.integers(0, shape["vocab"], 64).astype(np.int32)
    variants = {}
    for B in SIZES:
        for form in ("full",) if full_only else ("full", "attached"):
            name = f"{form}_{B}"
            if only and name != only:
                continue
            batch = rows_at_pos(dec, B, form == "attached", tokens)

            def run(b=batch):
                for _ in range(STEPS):
                    b.step_rows(tokens[:b.B], [POS] * b.B)   # (ends with a host synchronisation)
            variants[name] = run
    times = {k: [] for k in variants}
    for rnd in range(2 if only else ROUNDS + 1):
        for name, run in variants.items():
            t0 = time.perf_counter()
            run()
            if rnd:   # (round 0 warms up)
                times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
    rows = {name: dict(B=int(name.split("_")[1]), ms_per_step=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))
            for name, ts in times.items()}
    out = dict(metric="prefix_rows_step", model="llama3-8b-int4-g128-synthetic", S=S, prefix=PREFIX, position=POS, layers=shape["n_layers"],
               steps=STEPS, rounds=ROUNDS, rows=rows, device=acc.name())
    if not full_only and not only:
        for B in SIZES:
            out[f"b{B}_attached_vs_full"] = compare(rows[f"full_{B}"], rows[f"attached_{B}"])
    parent = arg("--parent")
    if parent:
        with open(parent) as f:
            prows = json.loads(f.readline())["rows"]
        out["parent_full"] = prows
        for B in SIZES:
            out[f"b{B}_full_vs_parent_full"] = compare(prows[f"full_{B}"], rows[f"full_{B}"])
    line = json.dumps(out)
    print(line)
    if only:
        return
    path = arg("--out", os.path.join(ROOT, "profiles", "prefix_rows_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
