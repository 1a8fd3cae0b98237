"""Shared-prefix rows on an fp8 batch (mc_kv_prefix_set, Part 2s): what a ragged step costs when every row attends ONE fp8 copy of its prompt,
against fp8 rows holding full copies and against the two bfloat16 forms of tools/prefix_rows_bench.py.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048, B = 8 and B = 64 (mc_kv_batch_create for fp8; mc_batch_create / mc_wide_batch_create
for bfloat16).  A prompt pass of 1920 tokens fills the decoder's cache; per B the forms
  fp8_attached_gwN  the 1920 positions quantised ONCE into the shared prefix, every row attached, N = 1, 2, 4 groups per P.V workgroup
                    (MC_SP8_GROUPS, read when the batch is created); fp8_attached_rule: the plan's own choice
  fp8_full          every row forked from the decoder (its own quantised copy): the per-row _f8_rows kernels
  bf16_attached, bf16_full   the same two on bfloat16 caches
All then take 108 untimed chained steps with the same tokens, so every row sits at position 2028 behind 108 slots of its own, and the timed
region is single mc_ragged_step calls at position 2028, 20 to a sample, each ending in its own host synchronisation.  The forms alternate in one
process: a warm-up round, then 5 timed rounds; median, min and max of ms per step.  A comparison says "faster" / "slower" when the medians differ
by more than the larger min-max spread of the two, else "equal".
--full-only: fp8_full and bf16_full alone -- runs on a build without Part 2s, to compare the unchanged paths across builds;
--parent FILE: the JSON line such a run wrote, merged in as `parent` with the same comparison against this build's two full forms;
--only NAME: one form alone (fp8_attached_gw1_64, fp8_full_64, ...), one sample and no file -- the process to put a kernel trace around.
Prints one JSON line and writes it to --out (default profiles/kv_fp8_prefix_bench.json).

usage: python tools/kv_fp8_prefix_bench.py [--out FILE] [--full-only] [--parent FILE] [--only NAME] [--layers N]"""
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
FORMS = ["fp8_attached_rule", "fp8_attached_gw1", "fp8_attached_gw2", "fp8_attached_gw4", "fp8_full", "bf16_attached", "bf16_full"]


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def rows_at_pos(dec, B, form, tokens):
    fp8, attached = form.startswith("fp8"), "attached" in form
    if fp8 and attached and form[-1].isdigit():
        os.environ["MC_SP8_GROUPS"] = form[-1]   # read once, when the batch is created
    batch = mc.Batch(dec, B, wide=True, kv="fp8") if fp8 else mc.Batch(dec, B, wide=B > 8)
    os.environ.pop("MC_SP8_GROUPS", None)
    if attached:
        if fp8:
            batch.set_kv_prefix(True)
        batch.prefix_fork(PREFIX)
    for r in range(B):
        batch.attach_row(r) if attached else batch.fork(r, PREFIX)
    batch.generate_rows(tokens[:B], [PREFIX] * B, POS - PREFIX)
    assert list(batch.lengths()) == [POS] * B
    return batch


def compare(a, b):
    """b against a"""
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    diff = b["ms_per_step"] - a["ms_per_step"]
    return dict(difference_ms=round(diff, 4), larger_spread_ms=round(spread, 4), verdict="equal" if abs(diff) < spread else ("faster" if diff < 0 else "slower"))


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
        for form in [f for f in FORMS if not full_only or f.endswith("full")]:
            name = f"{form}_{B}"
            if only and name != only:
                continue
            batch = rows_at_pos(dec, B, form, tokens)

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
    rows = {name: dict(B=int(name.rsplit("_", 1)[1]), ms_per_step=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))
            for name, ts in times.items()}
    out = dict(metric="kv_fp8_prefix_step", model="llama3-8b-int4-g128-synthetic", S=S, prefix=PREFIX, position=POS, layers=shape["n_layers"],
               steps=STEPS, rounds=ROUNDS, rows=rows, device=acc.name())
    if not full_only and not only:
        for B in SIZES:
            for gw in ("rule", "gw1", "gw2", "gw4"):
                out[f"b{B}_fp8_attached_{gw}_vs_fp8_full"] = compare(rows[f"fp8_full_{B}"], rows[f"fp8_attached_{gw}_{B}"])
                out[f"b{B}_fp8_attached_{gw}_vs_bf16_attached"] = compare(rows[f"bf16_attached_{B}"], rows[f"fp8_attached_{gw}_{B}"])
            for gw in (2, 4):
                out[f"b{B}_gw{gw}_vs_gw1"] = compare(rows[f"fp8_attached_gw1_{B}"], rows[f"fp8_attached_gw{gw}_{B}"])
    parent = arg("--parent")
    if parent:
        with open(parent) as f:
            prows = json.loads(f.readline())["rows"]
        out["parent"] = prows
        for name in prows:
            if name in rows:
                out[f"{name}_vs_parent"] = compare(prows[name], rows[name])
    line = json.dumps(out)
    print(line)
    if only:
        return
    path = arg("--out", os.path.join(ROOT, "profiles", "kv_fp8_prefix_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
