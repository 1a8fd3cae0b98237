"""MC_SAMPLER_DRAW: what the drawing last phase costs beside MC_SAMPLER_DEFAULT's.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 (mc_batch_create) and B = 64 (mc_wide_batch_create).  A prompt pass of
S - 1 tokens fills the decoder's cache and is forked into every row of one batch per B; every row is then stepped at S - 1, so every step
attends S positions (tools/row_sampler_bench.py's set-up).  Per B, ms per ragged step:
  default  no row sampler set, the decoder on MC_SAMPLER_DEFAULT (50, 0.6, 0.9): mc_b_topk_candidates_bfloat + mc_b_sample_rows_bfloat
  draw     the decoder on MC_SAMPLER_DRAW with the same numbers: mc_b_topk_candidates_bfloat + mc_draw_b_rows_bfloat
  mixed    rows alternating greedy, default and draw: mc_b_topk_candidates_mixed_bfloat + mc_b_pick_mixed_rows_bfloat
and the batch-1 decoder's tokens/s over one chained mc_decoder_generate of 64 tokens from position 1024, under default and under draw.
A step is a single mc_ragged_step call ending in its own host synchronisation, 20 to a sample; the variants alternate in one process: a
warm-up round, then 5 timed rounds, the median of which is the PROCESS's figure.

One process says little about another: run at least five of each build and merge them.  A figure of a build is then the median over its
processes with their min and max, and two figures are "equal" when they differ by less than the larger of the two min-max spreads.
  python tools/draw_sampler_bench.py --out run1.json                     one process of this build (one JSON line)
  python tools/draw_sampler_bench.py --default-only --out p1.json        ... of a build without MC_SAMPLER_DRAW (the parent commit)
  python tools/draw_sampler_bench.py --merge run*.json --parent p*.json  -> profiles/draw_sampler_bench.json (--out to write elsewhere)
--layers N: fewer layers (a quick look; the recorded file is made with all 32)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, STEPS, ROUNDS, B1_POS, B1_TOKENS = 2048, 20, 5, 1024, 64
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
SIZES = [8, 64]
NUMBERS = (50, 0.6, 0.9)
GREEDY, DEFAULT, DRAW = 0, 1, 2   # MC_SAMPLER_*
MIXED = [GREEDY, DEFAULT, DRAW]    # row r takes MIXED[r % 3]


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def args_after(name):
    out = []
    for a in sys.argv[sys.argv.index(name) + 1:] if name in sys.argv else []:
        if a.startswith("--"):
            break
        out.append(a)
    return out


def measure():
    import metalchat_amd as mc

    default_only = "--default-only" in sys.argv
    shape = dict(SHAPE, n_layers=int(arg("--layers", SHAPE["n_layers"])))
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **shape)
    dec.init_synthetic(1)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, shape["vocab"], S - 1).astype(np.int32), 0)
    tokens = rng.integers(0, shape["vocab"], 64).astype(np.int32)
    pairs = [(1000 + 17 * i, 77 + i) for i in range(64)]
    dec.set_seeds(pairs)
    variants, expect = {}, {}
    for B in SIZES:
        batch = mc.Batch(dec, B, wide=B > 8)
        for r in range(B):
            batch.fork(r, S - 1)
        batch.set_seeds(pairs)

        def settings(form, b=batch):   # (host only: nothing is launched)
            dec.set_sampler(DRAW if form == "draw" else DEFAULT, *NUMBERS)
            if default_only:
                return
            b.reset_row_samplers()
            for r in range(b.B if form == "mixed" else 0):
                kind = MIXED[r % 3]
                b.set_row_sampler(r, *((kind,) if kind == GREEDY else (kind,) + NUMBERS))

        def run(b=batch):
            for _ in range(STEPS):
                b.step_rows(tokens[:b.B], [S - 1] * b.B)   # (ends with a host synchronisation)

        for form, last in (("default", "mc_b_sample_rows_bfloat"), ("draw", "mc_draw_b_rows_bfloat"), ("mixed", "mc_b_pick_mixed_rows_bfloat")):
            if form != "default" and default_only:
                continue
            variants[f"{form}_{B}"] = (lambda form=form, settings=settings: settings(form), run, STEPS)
            expect[f"{form}_{B}"] = last
    for form, last in (("default", "mc_sample_bfloat"), ("draw", "mc_draw_bfloat")):
        if form != "default" and default_only:
            continue
        variants[f"batch1_{form}"] = (lambda form=form: dec.set_sampler(DRAW if form == "draw" else DEFAULT, *NUMBERS),
                                      lambda: dec.generate(int(tokens[0]), B1_POS, B1_TOKENS), B1_TOKENS)
        expect[f"batch1_{form}"] = last
    times = {k: [] for k in variants}
    for rnd in range(ROUNDS + 1):
        for name, (prepare, run, count) in variants.items():
            prepare()
            if rnd == 0:   # (round 0 warms up, and shows that the variant launches what it is named for)
                dec.launch_log(True)
            t0 = time.perf_counter()
            run()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3 / count)
            else:
                assert expect[name] in dec.launched(), (name, dec.launched()[-3:])
                dec.launch_log(False)
    rows = {name: dict(ms=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4)) for name, ts in times.items()}
    return dict(metric="draw_sampler_process", S=S, layers=shape["n_layers"], steps=STEPS, rounds=ROUNDS, rows=rows, device=acc.name())


def over_processes(files):
    """the figure of a build per variant: the median of its processes' medians, their min and max"""
    runs = []
    for path in files:
        with open(path) as f:
            runs.append(json.loads(f.readline()))
    assert len(runs) >= 5, "at least five processes of a build"
    assert len({(r["S"], r["layers"], r["steps"], r["rounds"]) for r in runs}) == 1
    out = {}
    for name in runs[0]["rows"]:
        ms = [r["rows"][name]["ms"] for r in runs]
        out[name] = dict(ms=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4), processes=len(ms))
        if name.startswith("batch1_"):
            out[name]["tokens_per_s"] = round(1e3 / out[name]["ms"], 2)
    return out, runs[0]


def compare(a, b):
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    return dict(difference_ms=round(b["ms"] - a["ms"], 4), larger_spread_ms=round(spread, 4), equal=bool(abs(b["ms"] - a["ms"]) < spread))


def merge():
    rows, one = over_processes(args_after("--merge"))
    out = dict(metric="draw_sampler_step", model="llama3-8b-int4-g128-synthetic", S=one["S"], layers=one["layers"], steps=one["steps"],
               rounds=one["rounds"], unit="ms per ragged step (batch1_*: ms per token of one chained call)", rows=rows, device=one["device"])
    for B in SIZES:
        out[f"b{B}_draw_vs_default"] = compare(rows[f"default_{B}"], rows[f"draw_{B}"])
        out[f"b{B}_mixed_vs_default"] = compare(rows[f"default_{B}"], rows[f"mixed_{B}"])
    out["batch1_draw_vs_default"] = compare(rows["batch1_default"], rows["batch1_draw"])
    if "--parent" in sys.argv:
        prows, _ = over_processes(args_after("--parent"))
        out["parent"] = prows
        for name in prows:
            out[f"{name}_vs_parent"] = compare(prows[name], rows[name])
    return out


def main():
    merging = "--merge" in sys.argv
    out = merge() if merging else measure()
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "draw_sampler_bench.json") if merging else None)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
