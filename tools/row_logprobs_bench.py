"""Row log-probabilities (mc_logprobs_*, include/metalchat_hip.h Part 2n): what one ragged step costs with the switch off, on with
top_n = 0 and on with top_n = 20, and what the two launches themselves take.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 (mc_batch_create) and B = 64 (mc_wide_batch_create).  A prompt pass of
S - 1 tokens fills the decoder's cache and is forked into every row of one batch per B; every row is then stepped at S - 1 (the next
step at S - 1 is a rewind by one, which a row of length S still takes), so every step attends S positions.  The decoder is greedy.  Per B:
  off    the switch is off (the default): the launches of a batch before this part
  on0    mc_logprobs_set(1, 0): mc_logprob_parts_rows_bfloat + mc_logprob_finish_rows_bfloat behind mc_b_argmax_rows_bfloat, the pick's
         log-probability alone
  on20   mc_logprobs_set(1, 20): the same two launches, with the 20 most likely tokens
All are single mc_ragged_step calls, 20 to a sample, each ending in its own host synchronisation; the variants alternate in one
process: a warm-up round, then 5 timed rounds; median, min and max of ms per step.  "equal": the medians differ by less than the
larger min-max spread of the two.  The two `on` forms are costs to report, no bounds.
The launches alone: the two kernels launched by name on buffers of the same shape, back to back: 2000 pairs between two device
events after 200 to warm up, three such samples; median, min and max of ms per pair.
--off-only: `off` alone -- runs on a build without this part, to compare the unchanged path across builds; --append adds the line to
  --out instead of replacing the file, so that several processes collect in one file; --root DIR: the checkout whose package is
  imported (default: this file's);
--parent FILE: the JSON lines such runs of the parent commit wrote, one process per line; --same FILE: the lines of --off-only
  processes of THIS build, started in turn with the parent's.  Two processes of one build differ by more than the rounds inside one
  process do, so the builds are compared over processes: per build the median of the processes' medians and the least and the most
  of all their rounds (this process's own `off` rows count as one more process of this build), then the same rule.
Prints one JSON line and writes it to --out (default profiles/row_logprobs_bench.json).

usage: python tools/row_logprobs_bench.py [--out FILE] [--off-only [--append]] [--root DIR] [--parent FILE [--same FILE]] [--layers N]"""
import json
import os
import statistics
import sys
import time

import numpy as np


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(arg("--root", HERE))
sys.path.insert(0, ROOT)
import metalchat_amd as mc

S, STEPS, ROUNDS = 2048, 20, 5
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
SIZES = [8, 64]
FORMS = {"off": None, "on0": 0, "on20": 20}
KERNEL_WARM, KERNEL_RUNS, KERNEL_SAMPLES = 200, 2000, 3
PICK, PARTS, FINISH = "mc_b_argmax_rows_bfloat", "mc_logprob_parts_rows_bfloat", "mc_logprob_finish_rows_bfloat"


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


def kernels_alone(acc, B, vocab, top_n):
    """ms per pair of launches over [B][vocab], every row active"""
    rng = np.random.default_rng(B)
    nchunk = -(-vocab // 2048)
    logits = acc.to_device(rng.integers(0x3C00, 0x4100, B * vocab).astype(np.uint16))   # bfloat16 bits of small positive values
    parts = acc.to_device(np.zeros(B * nchunk * 4, np.uint32))                          # kernels/abi.h logprob_part: 16 bytes
    keys = acc.to_device(np.zeros(B * nchunk * max(top_n, 1), np.uint64))
    rows = np.zeros((B, 12), np.int32)   # kernels/abi.h step_state: token 0 at position 0, slot r
    rows[:, 5] = np.arange(B)
    rb = acc.to_device(rows.reshape(-1))
    out_lp, out_ids, out_top = (acc.to_device(np.zeros(B * max(top_n, 1), np.uint32)) for _ in range(3))
    first = mc.KernelTask(acc.load(PARTS), (nchunk * 256, B, 1), (256, 1, 1), [logits, np.uint32(vocab), np.uint32(top_n), parts, keys, rb])
    second = mc.KernelTask(acc.load(FINISH), (256, B, 1), (256, 1, 1),
                           [logits, np.uint32(vocab), np.uint32(top_n), np.uint32(nchunk), parts, keys, rb, None, np.uint32(B), out_lp,
                            out_ids if top_n else None, out_top if top_n else None])
    for _ in range(KERNEL_WARM):
        first()
        second()
    acc.wait()
    ms = []
    for _ in range(KERNEL_SAMPLES):
        acc.timer_begin()
        for _ in range(KERNEL_RUNS):
            first()
            second()
        ms.append(acc.timer_end_ms() / KERNEL_RUNS)
    return dict(B=B, top_n=top_n, ms_per_pair=round(statistics.median(ms), 5), min=round(min(ms), 5), max=round(max(ms), 5), bytes_read=B * vocab * 2,
                pairs=KERNEL_RUNS, samples=KERNEL_SAMPLES)


def main():
    off_only = "--off-only" in sys.argv
    shape = dict(SHAPE, n_layers=int(arg("--layers", SHAPE["n_layers"])))
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **shape)
    dec.init_synthetic(1)
    dec.set_sampler(mc.SAMPLER_GREEDY)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, shape["vocab"], S - 1).astype(np.int32), 0)
    tokens = rng.integers(0, shape["vocab"], 64).astype(np.int32)
    variants = {}
    for B in SIZES:
        batch = mc.Batch(dec, B, wide=B > 8)
        for r in range(B):
            batch.fork(r, S - 1)

        def prepare(top_n, b=batch):   # (no launch)
            if off_only:
                return
            b.set_logprobs(top_n or 0, enable=top_n is not None)

        def run(b=batch):
            for _ in range(STEPS):
                b.step_rows(tokens[:b.B], [S - 1] * b.B)   # (ends with a host synchronisation)

        for form, top_n in FORMS.items():
            if form != "off" and off_only:
                continue
            variants[f"{form}_{B}"] = (lambda top_n=top_n, prepare=prepare: prepare(top_n), run)
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
                on = not name.startswith("off_")
                assert names[-3:] == [PICK, PARTS, FINISH] if on else names[-1] == PICK, (name, names[-3:])
                assert len([n for n in names if n.startswith("mc_logprob_")]) == (2 * STEPS if on else 0), name
    rows = {name: dict(B=int(name.split("_")[1]), ms_per_step=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))
            for name, ts in times.items()}
    out = dict(metric="row_logprobs_step", model="llama3-8b-int4-g128-synthetic", S=S, layers=shape["n_layers"], steps=STEPS, rounds=ROUNDS,
               rows=rows, device=acc.name())
    if not off_only:
        for B in SIZES:
            for form in ("on0", "on20"):
                out[f"b{B}_{form}_vs_off"] = compare(rows[f"off_{B}"], rows[f"{form}_{B}"])
        out["kernels"] = {f"b{B}_top{top_n}": kernels_alone(acc, B, shape["vocab"], top_n) for B in SIZES for top_n in (0, 20)}
    parent = arg("--parent")
    if parent:
        same = arg("--same")
        off = {name: r for name, r in rows.items() if name.startswith("off_")}
        out["parent"] = pooled(rows_of(parent))
        out["this_build"] = pooled((rows_of(same) if same else []) + [off])
        for name in out["parent"]:
            out[f"{name}_vs_parent"] = compare(out["parent"][name], out["this_build"][name])
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(HERE, "profiles", "row_logprobs_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a" if "--append" in sys.argv else "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
