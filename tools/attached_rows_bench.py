"""Packed chunks and verify on attached rows (mc_attached_packed_set): what mc_verify_rows and mc_extend_rows cost when the rows attend ONE
copy of their prompt through the mc_ax_* attention, against the same rows holding full copies through mc_px_*.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048.  A prompt pass of 1856 tokens fills the decoder's cache; per B (8: mc_batch_create,
64: mc_wide_batch_create) two batches:
  full      every row forked from the decoder (its own copy of the 1856 positions)
  attached  the 1856 positions forked ONCE into the shared prefix (shared = 1856), every row attached, the switch on
Both take 44 untimed chained steps with the same tokens, so every row sits at position 1900 behind 44 slots of its own.  The timed region is
single calls at position 1900 -- B = 8: 16 tokens a row, B = 64: 2 tokens a row; a verify call rewinds, a chunk is written over -- 5 to a
sample, each ending in its own host synchronisation.  The variants alternate in one process: a warm-up round, then 5 timed rounds, the
process's figure their median.  --processes N (default 3) runs N such processes one after the other; median, min and max over them.
"faster": the attached median is below the full one by more than the larger min-max spread of the two.
--only NAME: one variant alone (attached_verify_8, full_extend_64, ...), in this process, one sample and no file -- the process to put a
kernel trace around.
--kv fp8: both batches are fp8 (mc_kv_batch_create, a wide batch at either B) with mc_kv_packed_set on, the attached one with mc_kv_prefix_set
on as well: mc_ax8_* against mc_px8_* on full byte copies.  A third form, bf16, is the bfloat16 attached batch above in the same process, for
context; it enters no comparison.
Prints one JSON line and writes it to --out (default profiles/attached_rows_bench.json, --kv fp8: profiles/attached_rows_fp8_bench.json).

usage: python tools/attached_rows_bench.py [--kv bf16|fp8] [--out FILE] [--processes N] [--only NAME] [--layers N]"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, PREFIX, POS, CALLS, ROUNDS = 2048, 1856, 1900, 5, 5
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
SIZES = {8: 16, 64: 2}   # B: tokens a row


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def rows_at_pos(mc, dec, B, attached, tokens, fp8=False):
    batch = mc.Batch(dec, B, wide=True, kv="fp8") if fp8 else mc.Batch(dec, B, wide=B > 8)
    if fp8:
        batch.set_kv_packed(True)
    if attached:
        if fp8:
            batch.set_kv_prefix(True)
        batch.prefix_fork(PREFIX)
        batch.set_attached_packed(True)
    for r in range(B):
        batch.attach_row(r) if attached else batch.fork(r, PREFIX)
    batch.generate_rows(tokens[:B], [PREFIX] * B, POS - PREFIX)
    assert list(batch.lengths()) == [POS] * B
    return batch


def measure(only, layers, fp8=False):
    """this process: {variant: ms per call}, the median of its timed rounds"""
    import metalchat_amd as mc

    shape = dict(SHAPE, n_layers=layers)
    acc = mc.HardwareAccelerator()
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **shape)
    dec.init_synthetic(1)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, shape["vocab"], PREFIX).astype(np.int32), 0)
    tokens = rng.integers(0, shape["vocab"], 64).astype(np.int32)
    variants = {}
    for B, n in SIZES.items():
        chunks = [rng.integers(0, shape["vocab"], n).astype(np.int32) for _ in range(B)]
        for form in ("full", "attached") + (("bf16",) if fp8 else ()):
            if only and not (only.startswith(form) and only.endswith(f"_{B}")):
                continue
            batch = rows_at_pos(mc, dec, B, form != "full", tokens, fp8 and form != "bf16")
            for call in ("verify", "extend"):
                name = f"{form}_{call}_{B}"
                if only and name != only:
                    continue

                def run(b=batch, call=call, chunks=chunks):
                    for _ in range(CALLS):   # (each ends with a host synchronisation)
                        b.verify_rows(chunks, [POS] * b.B) if call == "verify" else b.extend_rows(chunks, [POS] * b.B)
                variants[name] = run
    times = {k: [] for k in variants}
    for rnd in range(2 if only else ROUNDS + 1):
        for name, run in variants.items():
            t0 = time.perf_counter()
            run()
            if rnd:   # (round 0 warms up)
                times[name].append((time.perf_counter() - t0) * 1e3 / CALLS)
    return {name: statistics.median(ts) for name, ts in times.items()}, acc.name()


def compare(a, b):
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    diff = b["ms_per_call"] - a["ms_per_call"]
    return dict(difference_ms=round(diff, 4), larger_spread_ms=round(spread, 4), equal=bool(abs(diff) < spread), faster=bool(-diff > spread))


def main():
    only, layers, kv = arg("--only"), int(arg("--layers", SHAPE["n_layers"])), arg("--kv", "bf16")
    if kv not in ("bf16", "fp8"):
        sys.exit("--kv: bf16 or fp8")
    if only or "--child" in sys.argv:
        ms, device = measure(only, layers, kv == "fp8")
        print(json.dumps(dict(ms=ms, device=device)))
        return
    n = int(arg("--processes", 3))
    runs = [json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", "--layers", str(layers), "--kv", kv], text=True).splitlines()[-1])
            for _ in range(n)]
    rows = {name: dict(B=int(name.split("_")[2]), ms_per_call=round(statistics.median(r["ms"][name] for r in runs), 4),
                       min=round(min(r["ms"][name] for r in runs), 4), max=round(max(r["ms"][name] for r in runs), 4)) for name in runs[0]["ms"]}
    out = dict(metric="attached_rows_call", kv=kv, model="llama3-8b-int4-g128-synthetic", S=S, prefix=PREFIX, position=POS, layers=layers, calls=CALLS,
               rounds=ROUNDS, processes=n, tokens_per_row=SIZES, rows=rows, device=runs[0]["device"])
    for B in SIZES:
        for call in ("verify", "extend"):
            out[f"b{B}_{call}_attached_vs_full"] = compare(rows[f"full_{call}_{B}"], rows[f"attached_{call}_{B}"])
    line = json.dumps(out)
    print(line)
    path = arg("--out", os.path.join(ROOT, "profiles", "attached_rows_fp8_bench.json" if kv == "fp8" else "attached_rows_bench.json"))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
