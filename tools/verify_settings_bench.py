"""Verify calls for sampling, masked and penalised rows (mc_settings_verify_set, ABI Part 2m): what the settings cost over the greedy call.

Llama-3-8B widths, int4 g128 synthetic weights, B = 8 rows, max_seq_len 2048, chunks of 16 tokens behind 1900 keys (128 packed rows: the
largest verify call).  Alternating inside every repetition:
  greedy_off     mc_verify_rows with the switch off: the call of before this part (the only case --old-api runs: the same file times a
                 build without the part, for the comparison across builds)
  greedy_on      the same call with the switch on, every row greedy and unprocessed: must launch and cost what greedy_off does
  draw           every row MC_SAMPLER_DRAW (top_k 50, temperature 0.8, top_p 0.9): the two pick launches in place of mc_v_argmax_bfloat
  draw_mask_pen  ... and every row behind a ban list (a quarter of the vocabulary) with repetition / frequency / presence penalties and 500
                 tokens of history: + the process launch over the 128 packed rows and the count launch
Fresh seed pairs (MC_VERIFY_MAX_LEN * B) go up in front of every call of the last two, as a serving loop does; the upload is inside the timed
region.  Synthetic weights accept almost nothing, so every call rewinds to the same positions.  Each call ends with a host sync and is timed
between two; median, minimum and maximum of REPS after a warm-up round.  Run several processes (--out appends a run to the file's "runs"):
two cases are "equal" when their medians differ by less than the larger min-max spread over the processes.

usage: python tools/verify_settings_bench.py [--reps N] [--old-api] [--label NAME] [--out profiles/verify_settings_bench.json]"""
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
B, S, CTX, CHUNK = 8, 2048, 1900, 16


def stats(ts):
    return round(float(np.median(ts)), 3), round(float(min(ts)), 3), round(float(max(ts)), 3)


def context(dec, rng):
    batch = mc.Batch(dec, B)
    for r in range(B):  # the rows' contexts (the cache contents do not matter to the time, the lengths do)
        call = [None] * B
        call[r] = rng.integers(0, SHAPE["vocab"], CTX).astype(np.int32)
        batch.prefill_rows(call)
    return batch


def run(a, acc):
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **SHAPE)
    dec.init_synthetic(1)
    rng = np.random.default_rng(0)
    ctx = np.full(B, CTX, np.int32)
    chunks = [rng.integers(0, SHAPE["vocab"], CHUNK).astype(np.int32) for _ in range(B)]
    cases = {"greedy_off": context(dec, rng)}
    seeded = set()
    if not a.old_api:
        on = context(dec, rng)
        on.set_verify_settings(True)
        draw = context(dec, rng)
        draw.set_verify_settings(True)
        full = context(dec, rng)
        full.set_verify_settings(True)
        for r in range(B):
            draw.set_row_sampler(r, mc.SAMPLER_DRAW, 50, 0.8, 0.9)
            full.set_row_sampler(r, mc.SAMPLER_DRAW, 50, 0.8, 0.9)
            full.set_row_mask(r, rng.random(SHAPE["vocab"]) > 0.25)
            full.set_row_penalties(r, 1.2, 0.1, 0.1)
            full.count_row_tokens(r, rng.integers(0, SHAPE["vocab"], 500))
        cases.update(greedy_on=on, draw=draw, draw_mask_pen=full)
        seeded = {"draw", "draw_mask_pen"}
    ts = {label: [] for label in cases}
    for rep in range(a.reps + 1):  # (round 0: the warm-up)
        for label, batch in cases.items():
            t0 = time.perf_counter()
            if label in seeded:
                batch.set_seeds(mc.seed_pairs(rng, CHUNK * B))
            batch.verify_rows(chunks, ctx)
            if rep:
                ts[label].append((time.perf_counter() - t0) * 1e3)
    row = dict(label=a.label, device=acc.name(), reps=a.reps)
    for label in cases:
        row[label + "_ms"], row[label + "_ms_min"], row[label + "_ms_max"] = stats(ts[label])
    print("   ".join(f"{label} {row[label + '_ms']:.3f} ms ({row[label + '_ms_min']:.3f} - {row[label + '_ms_max']:.3f})" for label in cases), flush=True)
    return row


def summary(runs):
    """per label (build): the median of the processes' medians and the min-max spread over all their calls; the verdicts by the project's rule"""
    out = {}
    for label in dict.fromkeys(r["label"] for r in runs):
        mine = [r for r in runs if r["label"] == label]
        out[label] = {}
        for case in ("greedy_off", "greedy_on", "draw", "draw_mask_pen"):
            if all(case + "_ms" in r for r in mine):
                out[label][case] = dict(ms=round(float(np.median([r[case + "_ms"] for r in mine])), 3), min=min(r[case + "_ms_min"] for r in mine),
                                        max=max(r[case + "_ms_max"] for r in mine), processes=len(mine))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--old-api", action="store_true")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = dict(model="Llama-3-8B widths, 32 layers, int4 g128, synthetic weights", B=B, max_seq_len=S, context=CTX, chunk=CHUNK, rows=B * CHUNK,
               timing="per process: median, min and max of the calls per case, the cases alternating, after one warm-up round; each call ends with "
                      "a host sync; the seed upload of the drawing cases is inside the timed region", runs=[])
    if a.out and os.path.exists(a.out):
        doc = json.load(open(a.out))
    doc["runs"].append(run(a, mc.HardwareAccelerator()))
    doc["summary"] = summary(doc["runs"])
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(doc["summary"]))


if __name__ == "__main__":
    main()
