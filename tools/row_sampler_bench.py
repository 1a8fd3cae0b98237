"""Row samplers (mc_row_sampler_*): what one ragged step costs under the three forms of the pick.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 (mc_batch_create) and B = 64 (mc_wide_batch_create).  A prompt pass of
S - 1 tokens fills the decoder's cache and is forked into every row of one batch per B; every row is then stepped at S - 1 (the next
step at S - 1 is a rewind by one, which a row of length S still takes), so every step attends S positions.  Per B:
  greedy   no row sampler set, the decoder greedy: mc_b_argmax_rows_bfloat
  default  no row sampler set, the decoder on make_default_sampler (50, 0.6, 0.9): mc_b_topk_candidates_bfloat + mc_b_sample_rows_bfloat
  mixed    the decoder as in `default`, rows alternating greedy, (50, 0.6, 0.9) and (20, 1.0, 1.0):
           mc_b_topk_candidates_mixed_bfloat + mc_b_pick_mixed_rows_bfloat -- the same work for two rows in three
All are single mc_ragged_step calls, 20 to a sample, each ending in its own host synchronisation; the variants alternate in one
process: a warm-up round, then 5 timed rounds; median, min and max of ms per step.  "equal": the medians differ by less than the
larger min-max spread of the two.
--uniform-only: greedy and default alone -- runs on a build without Part 2k, to compare the unchanged paths across builds;
--parent FILE: the JSON line such a run wrote, merged in as `parent` with the same comparison against this build's rows.
Prints one JSON line and writes it to --out (default profiles/row_sampler_bench.json).

usage: python tools/row_sampler_bench.py [--out FILE] [--uniform-only] [--parent FILE] [--layers N]"""
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
DEFAULT = (50, 0.6, 0.9)
MIXED = [None, DEFAULT, (20, 1.0, 1.0)]   # row r takes MIXED[r % 3]; None = greedy


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def compare(a, b):
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    return dict(difference_ms=round(b["ms_per_step"] - a["ms_per_step"], 4), larger_spread_ms=round(spread, 4),
                equal=bool(abs(b["ms_per_step"] - a["ms_per_step"]) < spread))


def main():
    uniform_only = "--uniform-only" in sys.argv
    shape = dict(SHAPE, n_layers=int(arg("--layers", SHAPE["n_layers"])))
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **shape)
    dec.init_synthetic(1)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, shape["vocab"], S - 1).astype(np.int32), 0)
    tokens = rng.integers(0, shape["vocab"], 64).astype(np.int32)
    pairs = [(1000 + 17 * i, 77 + i) for i in range(64)]
    variants, expect = {}, {}
    for B in SIZES:
        batch = mc.Batch(dec, B, wide=B > 8)
        for r in range(B):
            batch.fork(r, S - 1)
        batch.set_seeds(pairs)

        def settings(form, b=batch):   # (host only: nothing is launched)
            if form == "greedy":
                dec.set_sampler(mc.SAMPLER_GREEDY)
            else:
                dec.set_sampler(mc.SAMPLER_DEFAULT, *DEFAULT)
            if uniform_only:
                return
            b.reset_row_samplers()
            for r in range(b.B if form == "mixed" else 0):
                s = MIXED[r % 3]
                b.set_row_sampler(r, *((mc.SAMPLER_GREEDY,) if s is None else (mc.SAMPLER_DEFAULT,) + s))

        def run(b=batch):
            for _ in range(STEPS):
                b.step_rows(tokens[:b.B], [S - 1] * b.B)   # (ends with a host synchronisation)

        for form, last in (("greedy", "mc_b_argmax_rows_bfloat"), ("default", "mc_b_sample_rows_bfloat"), ("mixed", "mc_b_pick_mixed_rows_bfloat")):
            if form == "mixed" and uniform_only:
                continue
            variants[f"{form}_{B}"] = (lambda form=form, settings=settings: settings(form), run)
            expect[f"{form}_{B}"] = last
    times = {k: [] for k in variants}
    for rnd in range(ROUNDS + 1):
        for name, (prepare, run) in variants.items():
            prepare()
            if rnd == 0:   # (round 0 warms up, and shows that the variant launches what it is named for)
                dec.launch_log(True)
            t0 = time.perf_counter()
            run()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
            else:
                assert dec.launched()[-1] == expect[name], (name, dec.launched()[-3:])
                dec.launch_log(False)
    rows = {name: dict(B=int(name.split("_")[1]), ms_per_step=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))
            for name, ts in times.items()}
    out = dict(metric="row_sampler_step", model="llama3-8b-int4-g128-synthetic", S=S, layers=shape["n_layers"], steps=STEPS, rounds=ROUNDS,
               rows=rows, device=acc.name())
    if not uniform_only:
        for B in SIZES:
            out[f"b{B}_mixed_vs_default"] = compare(rows[f"default_{B}"], rows[f"mixed_{B}"])
    parent = arg("--parent")
    if parent:
        with open(parent) as f:
            prows = json.loads(f.readline())["rows"]
        out["parent"] = prows
        for name in prows:
            out[f"{name}_vs_parent"] = compare(prows[name], rows[name])
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "row_sampler_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
