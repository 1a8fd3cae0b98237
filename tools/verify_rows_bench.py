"""Speculative verify (mc_verify_rows) against what a caller has without it, and its head against the batch's own.

Model level (default): Llama-3-8B widths, int4 g128 synthetic weights, B = 8 rows, max_seq_len 2048, chunks of 4, 8 and 16 tokens
behind 1900 keys.  Per chunk length, alternating inside every repetition:
  verify    mc_verify_rows of the chunks (one accepted token + n - 1 drafts per row)
  extend    the same chunks through mc_extend_rows: the difference is what the M-row head, the picks and the acceptance cost
  steps     n ragged steps (mc_ragged_step): what the call replaces when every draft is accepted
  one_step  one ragged step: what the caller gets when none is
A verify call that accepts a drafts yields a + 1 tokens per row, a step yields one: with a draft that costs nothing verifying
beats stepping above  a = verify / one_step - 1  accepted drafts per call (break_even_accepted).  Synthetic weights give a draft
model no agreement with its target, so this reports costs and the break-even, not a speed-up.
Each call ends with a host sync and is timed between two; median, minimum and maximum of REPS after a warm-up round.

Kernel level (--head, under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/verify_rows_bench.py
--head`, a run of its own): the head of that model, 128256 x 4096 int4 g128, for M = 32, 64, 128 rows -- one mc_v_head_i4_bfloat
launch, then ceil(M / 8) launches of mc_b_gemv_i4_bfloat_e0 over the same rows, REPS + 1 times.  --head-trace DIR reads the
trace's kernel_trace csv back (the launches in order) and adds the "head" table to --out.

usage: python tools/verify_rows_bench.py [--reps N] [--out profiles/verify_rows_bench.json] [--head | --head-trace DIR]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metalchat_amd as mc

SHAPE = dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336, n_layers=32, vocab=128256, rope_theta=500000.0,
             attn_scale=128 ** -0.5)
B, S, CTX = 8, 2048, 1900
CHUNKS = (4, 8, 16)
HEAD_M = (32, 64, 128)
HEAD, GEMV = "mc_v_head_i4_bfloat", "mc_b_gemv_i4_bfloat_e0"
HBM_BYTES_PER_S, BF16_FLOPS = 8.0e12, 2.5e15   # MI355X: HBM3E peak, dense bf16 MFMA peak (the spec figures)


def stats(ts):
    return round(float(np.median(ts)), 3), round(float(min(ts)), 3), round(float(max(ts)), 3)


def model_level(a, acc):
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **SHAPE)
    dec.init_synthetic(1)
    batch = mc.Batch(dec, B)
    rng = np.random.default_rng(0)
    ids = lambda n: rng.integers(0, SHAPE["vocab"], n).astype(np.int32)
    for r in range(B):  # the rows' contexts (the cache contents do not matter to the time, the lengths do)
        call = [None] * B
        call[r] = ids(CTX)
        batch.prefill_rows(call)
    ctx = np.full(B, CTX, np.int32)

    def steps(chunks, n):
        for i in range(n):
            batch.step_rows(np.array([c[i] for c in chunks], np.int32), ctx + i)

    variants = (("verify", lambda c, n: batch.verify_rows(c, ctx)), ("extend", lambda c, n: batch.extend_rows(c, ctx)),
                ("steps", steps), ("one_step", lambda c, n: steps(c, 1)))
    results = []
    for n in CHUNKS:
        chunks = [ids(n) for _ in range(B)]
        ts = {label: [] for label, _ in variants}
        for rep in range(a.reps + 1):  # (round 0: the warm-up)
            for label, fn in variants:
                t0 = time.perf_counter()
                fn(chunks, n)
                if rep:
                    ts[label].append((time.perf_counter() - t0) * 1e3)
        row = dict(chunk=n, rows=n * B)
        for label, _ in variants:
            row[label + "_ms"], row[label + "_ms_min"], row[label + "_ms_max"] = stats(ts[label])
        row["head_picks_accept_ms"] = round(row["verify_ms"] - row["extend_ms"], 3)
        row["steps_over_verify"] = round(row["steps_ms"] / row["verify_ms"], 2)
        row["break_even_accepted"] = round(row["verify_ms"] / row["one_step_ms"] - 1, 2)
        print(f"chunk {n:2d}: verify {row['verify_ms']:7.2f} ms   extend {row['extend_ms']:7.2f} ms   {n} steps {row['steps_ms']:7.2f} ms   "
              f"one step {row['one_step_ms']:6.2f} ms   break-even {row['break_even_accepted']:.2f} accepted drafts per call", flush=True)
        results.append(row)
    return dict(model="Llama-3-8B widths, 32 layers, int4 g128, synthetic weights", B=B, max_seq_len=S, context=CTX, device=acc.name(),
                timing="median, min and max of %d calls per variant, the variants alternating, after one warm-up round; each call ends "
                       "with a host sync" % a.reps, results=results)


def head_launches(a, acc):
    """the launches a kernel trace is taken of; nothing is timed here"""
    cfg = dict(SHAPE, n_layers=1)
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=64, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=128, **cfg)
    dec.init_synthetic(1)
    w, s, N, K, ng = dec.weight_ptrs(-1, "output")
    wb, sb = acc.wrap(w, 1 << 40), acc.wrap(s, 1 << 40)
    x = (np.random.default_rng(1).normal(0, 1, (128, K)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    xb, yb = acc.to_device(x.reshape(-1)), acc.alloc(128 * N * 2)
    common = [np.uint32(K), np.uint32(ng), np.uint32(128)]
    for M in HEAD_M:
        for rep in range(a.reps + 1):
            mc.KernelTask(acc.load(HEAD), ((N + 63) // 64 * 512, 1, 1), (512, 1, 1), [wb, sb, xb, yb] + common + [np.uint32(M), np.uint32(N), np.uint32(N)])()
            for r in range(0, M, 8):
                mc.KernelTask(acc.load(GEMV), (N // 16 * 512, 1, 1), (512, 1, 1),
                              [wb, sb, (xb, r * K * 2), (yb, r * N * 2)] + common + [np.uint32(8), np.uint32(N)])()
            acc.wait()
    print(f"head launches done: M {HEAD_M}, {a.reps + 1} rounds each")


def head_table(a):
    files = glob.glob(os.path.join(a.head_trace, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = [r for r in csv.DictReader(open(files[0])) if r["Kernel_Name"].split("(")[0].split(".")[0] in (HEAD, GEMV)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(r["Kernel_Name"].split("(")[0].split(".")[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]
    N, K = SHAPE["vocab"], SHAPE["dim"]
    weight_bytes = N * K // 2 + N * (K // 128) * 2
    out, i = [], 0
    for M in HEAD_M:
        head, gemv = [], []
        for rep in range(a.reps + 1):
            n = (M + 7) // 8
            names = [u[0] for u in us[i:i + 1 + n]]
            assert names == [HEAD] + [GEMV] * n, (M, rep, names)
            if rep:
                head.append(us[i][1])
                gemv.append(sum(u[1] for u in us[i + 1:i + 1 + n]))
            i += 1 + n
        t_hbm, t_mfma = weight_bytes / HBM_BYTES_PER_S * 1e6, 2.0 * M * N * K / BF16_FLOPS * 1e6
        row = dict(M=M, gemv_launches=(M + 7) // 8)
        row["head_us"], row["head_us_min"], row["head_us_max"] = stats(head)
        row["gemv_us"], row["gemv_us_min"], row["gemv_us_max"] = stats(gemv)
        spread = max(row["head_us_max"] - row["head_us_min"], row["gemv_us_max"] - row["gemv_us_min"])
        row["faster_by_more_than_the_spread"] = bool(row["head_us"] < row["gemv_us"] - spread)
        row["bound"], row["bound_us"] = ("HBM", round(t_hbm, 1)) if t_hbm >= t_mfma else ("bf16 MFMA", round(t_mfma, 1))
        row["share_of_bound"] = round(row["bound_us"] / row["head_us"], 3)
        print(f"M {M:3d}: {HEAD} {row['head_us']:8.1f} us ({row['head_us_min']:.1f} - {row['head_us_max']:.1f})   {row['gemv_launches']} x {GEMV} "
              f"{row['gemv_us']:8.1f} us ({row['gemv_us_min']:.1f} - {row['gemv_us_max']:.1f})   bound {row['bound']} {row['bound_us']} us: "
              f"{row['share_of_bound']:.2f} of it", flush=True)
        out.append(row)
    assert i == len(us), (i, len(us))
    return dict(shape=f"{N} x {K} int4 g128", weight_bytes=weight_bytes,
                timing="rocprofv3 --kernel-trace, a run of its own: median, min and max of %d rounds after one warm-up round; gemv_us is the "
                       "sum of a round's launches; bounds: weight bytes / 8 TB/s and 2 M N K / 2.5 PFLOP/s (spec figures)" % a.reps, results=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--head", action="store_true")
    ap.add_argument("--head-trace", default=None)
    a = ap.parse_args()
    if a.head:
        return head_launches(a, mc.HardwareAccelerator())
    doc = {}
    if a.out and os.path.exists(a.out):
        doc = json.load(open(a.out))
    if a.head_trace:
        doc["head"] = head_table(a)
    else:
        doc.update(model_level(a, mc.HardwareAccelerator()))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
