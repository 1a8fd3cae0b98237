"""Row logit processors (mc_row_mask_*, mc_row_penalty_*): what one ragged step costs with nothing set and with every row masked and
penalised, and what the process kernel itself takes.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 (mc_batch_create) and B = 64 (mc_wide_batch_create).  A prompt pass of
S - 1 tokens fills the decoder's cache and is forked into every row of one batch per B; every row is then stepped at S - 1 (the next
step at S - 1 is a rewind by one, which a row of length S still takes), so every step attends S positions.  The decoder is greedy.  Per B:
  nothing    no row has a mask or penalties: the launches of a batch before this part
  processed  every row carries a mask of every second token, penalties (1.3, 0.5, 0.25) and 512 counted tokens:
             mc_b_logits_process_rows_bfloat between the head and mc_b_argmax_rows_bfloat
All are single mc_ragged_step calls, 20 to a sample, each ending in its own host synchronisation; the variants alternate in one
process: a warm-up round, then 5 timed rounds; median, min and max of ms per step.  "equal": the medians differ by less than the
larger min-max spread of the two.
The kernel alone: mc_b_logits_process_rows_bfloat launched by name on buffers of the same shape (every row masked and penalised),
200 launches between two device events after 20 to warm up, next to the bytes it moves: B x vocab x (2 read + 2 written + 4 counts)
plus the mask words.
--nothing-only: `nothing` alone -- runs on a build without this part, to compare the unchanged path across builds; --append adds the
  line to --out instead of replacing the file, so that several processes collect in one file;
--parent FILE: the JSON lines such runs of the parent commit wrote, one process per line; --same FILE: the lines of --nothing-only
  processes of THIS build, started in turn with the parent's.  Two processes of one build differ by more than the rounds inside one
  process do, so the builds are compared over processes: per build the median of the processes' medians and the least and the most
  of all their rounds (this process's own `nothing` rows count as one more process of this build), then the same rule.
Prints one JSON line and writes it to --out (default profiles/row_logits_bench.json).

usage: python tools/row_logits_bench.py [--out FILE] [--nothing-only [--append]] [--parent FILE [--same FILE]] [--layers N]"""
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
PENALTIES = (1.3, 0.5, 0.25)
KERNEL_WARM, KERNEL_RUNS = 20, 200
RL = np.dtype([("flags", np.uint32), ("rep", np.float32), ("inv_rep", np.float32), ("freq", np.float32), ("pres", np.float32),
               ("pad", np.uint32, (3,))])   # kernels/abi.h row_logits


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def compare(a, b):
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    return dict(difference_ms=round(b["ms_per_step"] - a["ms_per_step"], 4), larger_spread_ms=round(spread, 4),
                equal=bool(abs(b["ms_per_step"] - a["ms_per_step"]) < spread))


def pooled(processes):
    """processes: the `rows` of several processes of one build -> per variant the median of their medians, the least and the most"""
    return {name: dict(B=processes[0][name]["B"], ms_per_step=round(statistics.median(p[name]["ms_per_step"] for p in processes), 4),
                       min=min(p[name]["min"] for p in processes), max=max(p[name]["max"] for p in processes), processes=len(processes))
            for name in processes[0]}


def rows_of(path):
    with open(path) as f:
        return [json.loads(line)["rows"] for line in f if line.strip()]


def kernel_alone(acc, B, vocab):
    """ms per launch of the process kernel over [B][vocab] with every row masked and penalised, and the bytes one launch moves"""
    rng = np.random.default_rng(B)
    nw = (vocab + 31) // 32
    logits = acc.to_device(rng.integers(0x3C00, 0x4100, B * vocab).astype(np.uint16))   # bfloat16 bits of small positive values
    counts = acc.to_device((rng.random(B * vocab) < 0.01).astype(np.int32))
    masks = acc.to_device(np.full(B * nw, 0x55555555, np.uint32))
    tab = np.zeros(B, RL)
    tab["flags"], tab["rep"], tab["inv_rep"], tab["freq"], tab["pres"] = 3, PENALTIES[0], np.float32(1) / np.float32(PENALTIES[0]), PENALTIES[1], PENALTIES[2]
    rows = np.zeros((B, 12), np.int32)   # kernels/abi.h step_state: token 0 at position 0
    task = mc.KernelTask(acc.load("mc_b_logits_process_rows_bfloat"), (-(-vocab // 2048) * 256, B, 1), (256, 1, 1),
                         [logits, np.uint32(vocab), acc.to_device(tab.view(np.uint8)), masks, counts, acc.to_device(rows.reshape(-1)), np.int32(0)])
    for _ in range(KERNEL_WARM):
        task()
    acc.wait()
    acc.timer_begin()
    for _ in range(KERNEL_RUNS):
        task()
    ms = acc.timer_end_ms() / KERNEL_RUNS
    moved = B * vocab * (2 + 2 + 4) + B * nw * 4
    return dict(B=B, ms_per_launch=round(ms, 5), bytes=moved, gb_per_s=round(moved / (ms * 1e-3) / 1e9, 1), launches=KERNEL_RUNS)


def main():
    nothing_only = "--nothing-only" in sys.argv
    shape = dict(SHAPE, n_layers=int(arg("--layers", SHAPE["n_layers"])))
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **shape)
    dec.init_synthetic(1)
    dec.set_sampler(mc.SAMPLER_GREEDY)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, shape["vocab"], S - 1).astype(np.int32), 0)
    tokens = rng.integers(0, shape["vocab"], 64).astype(np.int32)
    history = rng.integers(0, shape["vocab"], 512).astype(np.int32)
    mask = np.arange(shape["vocab"]) % 2 == 0
    variants, expect = {}, {}
    for B in SIZES:
        batch = mc.Batch(dec, B, wide=B > 8)
        for r in range(B):
            batch.fork(r, S - 1)

        def settings(form, b=batch):   # (uploads, no launch)
            if nothing_only:
                return
            b.reset_row_logits()
            for r in range(b.B if form == "processed" else 0):
                b.set_row_mask(r, mask)
                b.set_row_penalties(r, *PENALTIES)
                b.count_row_tokens(r, history)

        def run(b=batch):
            for _ in range(STEPS):
                b.step_rows(tokens[:b.B], [S - 1] * b.B)   # (ends with a host synchronisation)

        for form, before_pick in (("nothing", None), ("processed", "mc_b_logits_process_rows_bfloat")):
            if form == "processed" and nothing_only:
                continue
            variants[f"{form}_{B}"] = (lambda form=form, settings=settings: settings(form), run)
            expect[f"{form}_{B}"] = before_pick
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
                names = dec.launched()
                dec.launch_log(False)
                assert names[-1] == "mc_b_argmax_rows_bfloat", (name, names[-3:])
                process = [n for n in names if n.startswith("mc_b_logits_process")]
                assert process == ([expect[name]] * STEPS if expect[name] else []), (name, len(process))
                assert not expect[name] or names[-2] == expect[name], (name, names[-3:])
    rows = {name: dict(B=int(name.split("_")[1]), ms_per_step=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))
            for name, ts in times.items()}
    out = dict(metric="row_logits_step", model="llama3-8b-int4-g128-synthetic", S=S, layers=shape["n_layers"], steps=STEPS, rounds=ROUNDS,
               rows=rows, device=acc.name())
    if not nothing_only:
        for B in SIZES:
            out[f"b{B}_processed_vs_nothing"] = compare(rows[f"nothing_{B}"], rows[f"processed_{B}"])
        out["kernel"] = {f"b{B}": kernel_alone(acc, B, shape["vocab"]) for B in SIZES}
    parent = arg("--parent")
    if parent:
        same = arg("--same")
        nothing = {name: r for name, r in rows.items() if name.startswith("nothing_")}
        out["parent"] = pooled(rows_of(parent))
        out["this_build"] = pooled((rows_of(same) if same else []) + [nothing])
        for name in out["parent"]:
            out[f"{name}_vs_parent"] = compare(out["parent"][name], out["this_build"][name])
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "row_logits_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a" if "--append" in sys.argv else "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
