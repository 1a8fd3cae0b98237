"""Wide batches (mc_wide_batch_create): what a step of B rows costs in ONE batch against the same rows in ceil(B / 8) batches of 8.

Llama-3-8B widths, int4 g128, synthetic weights, S = 2048.  A 2028-token prompt pass fills the decoder's cache and is forked into
every row.  Per B in 8, 16, 17, 32, 64 two variants: `wide`, one mc_batch_generate of 20 lockstep steps on a wide batch of B rows,
and `narrow`, the same on each of the ceil(B / 8) mc_batch_create batches one after another -- what the rows cost without the wide
batch.  All variants alternate in one process: a warm-up round, then 5 timed rounds, each timed region ending in the call's own host
synchronisation; median, min and max per variant.  B = 16 runs on mc_b_gemv_*, B = 17 on mc_wb_gemv_*: what the 16-row line costs.
--tiles: also B = 64 with MC_WB_TILES = 1, 2, 4, 8 (weight tiles per workgroup for every matrix, in place of batch_plan.h's rule (wb_tiles)).
Prints one JSON line.

usage: python tools/wide_batch_bench.py [--out FILE] [--tiles] [--only B]      (--only: the wide variant of B alone, e.g. under a trace)
       python tools/wide_batch_bench.py --gemv [--out FILE]
--gemv: the kernels alone, launched by name on the decoder's w1|w3 (28672 x 4096, e2) and w2 (4096 x 14336, e1) at M = 32 and 64,
one launch per layer over the 32 layers (0.9 GB of weights per sweep: nothing stays in the Infinity Cache), mc_wb_gemv_* at each
tile count against ceil(M / 8) launches of mc_b_gemv_*; device-timer means per launch with the HBM and MFMA bounds.  Under
`rocprofv3 --kernel-trace --stats` the same run gives the per-dispatch times."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metalchat_amd as mc

S, PROMPT, STEPS, ROUNDS = 2048, 2028, 20, 5
SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
SIZES = [8, 16, 17, 32, 64]
HBM_TBPS, MFMA_BF16_PFLOPS = 8.0, 2.5   # peaks the bounds are computed with (dense bf16)
BG_THREADS = 512


def decoder(acc):
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **SHAPE)
    dec.init_synthetic(1)
    return dec


def forked(dec, B, wide, tiles=None):
    if tiles:
        os.environ["MC_WB_TILES"] = str(tiles)   # read once, when the batch is created
    batch = mc.Batch(dec, B, wide=wide)
    os.environ.pop("MC_WB_TILES", None)
    for r in range(B):
        batch.fork(r, PROMPT)
    return batch


def steps_bench(out_path):
    acc = mc.HardwareAccelerator()
    dec = decoder(acc)
    rng = np.random.default_rng(0)
    dec.prefill(rng.integers(0, SHAPE["vocab"], PROMPT).astype(np.int32), 0)
    only = int(sys.argv[sys.argv.index("--only") + 1]) if "--only" in sys.argv else None
    sizes = [only] if only else SIZES
    narrow = [] if only else [forked(dec, 8, False) for _ in range(max(sizes) // 8)]
    one = None if only else forked(dec, 1, False)   # the ninth row's batch of B = 17
    first = rng.integers(0, SHAPE["vocab"], 64).astype(np.int32)
    variants = {}

    def add(name, batches):
        def run():
            r0 = 0
            for b in batches:
                b.generate(first[r0:r0 + b.B], PROMPT, STEPS)   # (ends with a host synchronisation)
                r0 += b.B
        variants[name] = run

    for B in sizes:
        add(f"wide_{B}", [forked(dec, B, True)])
        if not only:
            add(f"narrow_{B}", narrow[:B // 8] + ([one] if B % 8 else []))
    if "--tiles" in sys.argv:
        for t in (1, 2, 4, 8):
            add(f"wide_64_tiles{t}", [forked(dec, 64, True, tiles=t)])
    times = {k: [] for k in variants}
    for rnd in range(ROUNDS + 1):
        for name, run in variants.items():
            t0 = time.perf_counter()
            run()
            if rnd:   # (round 0 warms up)
                times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
    rows = {}
    for name, ts in times.items():
        B = int(name.split("_")[1])
        med = statistics.median(ts)
        rows[name] = dict(B=B, ms_per_step=round(med, 4), min=round(min(ts), 4), max=round(max(ts), 4), tokens_per_s=round(B / med * 1e3, 1))
    out = dict(metric="wide_batch_decode", model="llama3-8b-int4-g128-synthetic", S=S, context=PROMPT, steps=STEPS, rounds=ROUNDS,
               rows=rows, device=acc.name())
    if not only:
        w, n = rows["wide_64"], rows["narrow_64"]
        spread = max(w["max"] - w["min"], n["max"] - n["min"])
        out["b64_wide_vs_8_narrow"] = dict(wide_ms=w["ms_per_step"], narrow_ms=n["ms_per_step"], larger_spread_ms=round(spread, 4),
                                           wide_is_faster_by_more_than_the_spread=bool(n["ms_per_step"] - w["ms_per_step"] > spread))
        out["line_16_17"] = dict(b16_ms=rows["wide_16"]["ms_per_step"], b17_ms=rows["wide_17"]["ms_per_step"])
    emit(out, out_path)


def gemv_bench(out_path):
    acc = mc.HardwareAccelerator()
    dec = decoder(acc)
    L = SHAPE["n_layers"]
    rng = np.random.default_rng(1)
    wrap = lambda p: acc.wrap(p, 1 << 40) if p else None
    rows = []
    for which, epi in (("w13", 2), ("w2", 1)):
        ptrs = [dec.weight_ptrs(layer, which) for layer in range(L)]
        _, _, N, K, ng = ptrs[0]
        x = acc.to_device((rng.normal(0, 1, (64, K)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).reshape(-1))
        y = acc.to_device(np.zeros(64 * N, np.uint16))
        ldy = N // 2 if epi == 2 else N
        wbytes = N * K // 2 + N * ng * 2

        def sweep(name, grid, args_of):
            """mean ms of one launch over the layers' matrices, after an untimed sweep"""
            k = acc.load(name)
            tasks = [mc.KernelTask(k, (grid * BG_THREADS, 1, 1), (BG_THREADS, 1, 1), args_of(p)) for p in ptrs]
            for t in tasks:
                t()
            acc.wait()
            acc.timer_begin()
            for t in tasks:
                t()
            return acc.timer_end_ms() / len(tasks)

        for M in (32, 64):
            xb = [(x, 2 * K * r) for r in range(0, M, 8)]      # (buffer, byte offset): eight rows per narrow launch
            yb = [(y, 2 * ldy * r) for r in range(0, M, 8)]
            narrow = sum(sweep(f"mc_b_gemv_i4_bfloat_e{epi}", N // 16,
                               lambda p, i=i: [wrap(p[0]), wrap(p[1]), xb[i], yb[i], np.uint32(K), np.uint32(ng), np.uint32(128), np.uint32(8),
                                               np.uint32(ldy)]) for i in range(M // 8))
            row = dict(matrix=which, N=N, K=K, M=M, kernel=f"mc_wb_gemv_i4_bfloat_e{epi}", narrow_launches=M // 8, narrow_us=round(narrow * 1e3, 2),
                       hbm_bound_us=round(wbytes / (HBM_TBPS * 1e12) * 1e6, 2),
                       mfma_bound_us=round(2.0 * N * K * 16 * ((M + 15) // 16) / (MFMA_BF16_PFLOPS * 1e15) * 1e6, 2))
            for tiles in (1, 2, 4, 8):
                ms = sweep(f"mc_wb_gemv_i4_bfloat_e{epi}", (N // 16 + tiles - 1) // tiles,
                           lambda p: [wrap(p[0]), wrap(p[1]), x, y, np.uint32(K), np.uint32(ng), np.uint32(128), np.uint32(M), np.uint32(N),
                                      np.uint32(ldy)])
                row[f"wide_tiles{tiles}_us"] = round(ms * 1e3, 2)
            rows.append(row)
    emit(dict(metric="wide_batch_gemv", model="llama3-8b-int4-g128-synthetic", hbm_tbps=HBM_TBPS, mfma_bf16_pflops=MFMA_BF16_PFLOPS,
              compute_units=acc.compute_units(), rows=rows, device=acc.name()), out_path)


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    gemv_bench(path) if "--gemv" in sys.argv else steps_bench(path)
