"""QLoRA rows (mc_wide_batch_create, Part 2i): what a step of B rows costs on the checkpoint flavour the reference ships.

Llama-3.2-1B QLoRA widths: dim 2048, 32 / 8 heads of 64, ffn 8192, 16 layers, vocab 128256, int4 linears in groups of 32 with a
rank-16 adaptor each, an int8 embedding table, an int8 head with one scale per row; random weights (one layer's arrays loaded into
every layer: the copies in HBM are distinct), max_seq_len 1024 as the reference's serializers set it.  A 1000-token prompt pass
fills the decoder's cache and is forked into every row.  Per B in 1, 8, 17, 64 three variants:
  batch_B     one mc_batch_generate of 20 lockstep steps on a wide batch of B rows
  decoder_B   (a) B successive mc_decoder_generate calls of 20 tokens on the batch-1 decoder: what a caller has without the batch
  plain_B     (b) the same batch on a second decoder with the same weights and no adaptors loaded: the price of the adaptors
All variants alternate in one process: a warm-up round, then 5 timed rounds, each timed region ending in the call's own host
synchronisation; median, min and max per variant, in ms per step (of all B rows).  Prints one JSON line.

usage: python tools/qlora_batch_bench.py [--out FILE] [--only B]
--only B: batch_B alone (under `rocprofv3 --kernel-trace --stats` it gives the per-dispatch times: B = 8 runs mc_b_gemv_i4_bfloat_e2_l
on w1|w3, B = 17 mc_wb_gemv_i8_bfloat_e0 on the head); the JSON then carries the HBM bounds of those two launches."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metalchat_amd as mc

S, PROMPT, STEPS, ROUNDS = 1024, 1000, 20, 5
SHAPE = dict(dim=2048, n_heads=32, n_kv_heads=8, head_dim=64, ffn_dim=8192, n_layers=16, vocab=128256, rope_theta=500000.0,
             attn_scale=64 ** -0.5)
GROUP, RANK, LORA_SCALE = 32, 16, 2.0
SIZES = [1, 8, 17, 64]
HBM_TBPS = 8.0


def bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def layer_arrays(rng):
    dim, H, KV, hd, ffn = SHAPE["dim"], SHAPE["n_heads"], SHAPE["n_kv_heads"], SHAPE["head_dim"], SHAPE["ffn_dim"]
    shapes = dict(wq=(H * hd, dim), wk=(KV * hd, dim), wv=(KV * hd, dim), wo=(dim, H * hd), w1=(ffn, dim), w3=(ffn, dim), w2=(dim, ffn))
    out = {}
    for name, (o, i) in shapes.items():
        q = rng.integers(-8, 8, size=(o, i), dtype=np.int8)
        s = (rng.uniform(0.5, 1.5, (o, i // GROUP)) / (np.sqrt(i) * 8.0)).astype(np.float32)
        a = bf16(rng.uniform(-1, 1, (RANK, i)) / np.sqrt(i))
        b = bf16(rng.uniform(-1, 1, (o, RANK)) * (0.25 / np.sqrt(RANK)))
        out[name] = (q, s, a, b)
    return out


def decoder(acc, layer, head, adaptors):
    dec = mc.Decoder(acc, dtype=mc.BF16, max_seq_len=S, norm_eps=1e-5, weight_format=mc.WFMT_I4, group_size=GROUP, **SHAPE)
    ones = bf16(np.ones(SHAPE["dim"]))
    for li in range(SHAPE["n_layers"]):
        for name, (q, s, a, b) in layer.items():
            dec.load_linear(li, name, mc.WFMT_I4, q, s, GROUP)
            if adaptors:
                dec.load_lora(li, name, a, b, LORA_SCALE)
        dec.load_vector(li, "attention_norm", ones)
        dec.load_vector(li, "ffn_norm", ones)
    hq, hs, es = head
    dec.load_linear(-1, "tok_embeddings", mc.WFMT_I8, hq, es)
    dec.load_linear(-1, "output", mc.WFMT_I8, hq, hs, 0)
    dec.load_vector(-1, "norm", ones)
    return dec


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    only = int(sys.argv[sys.argv.index("--only") + 1]) if "--only" in sys.argv else None
    acc = mc.HardwareAccelerator()
    rng = np.random.default_rng(0)
    layer = layer_arrays(rng)
    V, dim = SHAPE["vocab"], SHAPE["dim"]
    head = (rng.integers(-128, 128, size=(V, dim), dtype=np.int8), (rng.uniform(0.5, 1.5, (V, 1)) / (np.sqrt(dim) * 128.0)).astype(np.float32),
            (rng.uniform(0.5, 1.5, V) * (0.02 / 64.0)).astype(np.float32))
    prompt = rng.integers(0, V, PROMPT).astype(np.int32)
    first = rng.integers(0, V, 64).astype(np.int32)
    say = lambda text: print(text, file=sys.stderr, flush=True)
    say("weights drawn; loading the decoder with adaptors")
    dec = decoder(acc, layer, head, True)
    dec.prefill(prompt, 0)
    variants = {}

    def forked(d, B):
        b = mc.Batch(d, B, wide=True)
        for r in range(B):
            b.fork(r, PROMPT)
        return b

    def add_batch(name, b):
        variants[name] = lambda: b.generate(first[:b.B], PROMPT, STEPS)            # (ends with a host synchronisation)

    def add_decoder(name, B):
        def run():
            for r in range(B):
                dec.generate(int(first[r]), PROMPT, STEPS)                         # (each ends with a host synchronisation)
        variants[name] = run

    sizes = [only] if only else SIZES
    if not only:
        say("loading the decoder without adaptors")
        plain = decoder(acc, layer, head, False)
        plain.prefill(prompt, 0)
    for B in sizes:
        add_batch(f"batch_{B}", forked(dec, B))
        if not only:
            add_decoder(f"decoder_{B}", B)
            add_batch(f"plain_{B}", forked(plain, B))
    times = {k: [] for k in variants}
    for rnd in range(ROUNDS + 1):
        say(f"round {rnd} of {ROUNDS}")
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
    out = dict(metric="qlora_batch_decode", model="llama3.2-1b-qlora-int4-g32-r16-random", S=S, context=PROMPT, steps=STEPS, rounds=ROUNDS,
               rows=rows, device=acc.name())
    ffn = SHAPE["ffn_dim"]
    out["hbm_bounds_us"] = {   # weights + scales (+ the adaptor's B) of one launch at HBM_TBPS, as in the mc_v_head table
        "mc_b_gemv_i4_bfloat_e2_l w1|w3": round((2 * ffn * dim // 2 + 2 * ffn * (dim // GROUP) * 2 + 2 * ffn * 2 * RANK * 2) / (HBM_TBPS * 1e12) * 1e6, 2),
        "mc_wb_gemv_i8_bfloat_e0 head": round((V * dim + V * 2) / (HBM_TBPS * 1e12) * 1e6, 2)}
    if not only:
        b, d = rows["batch_8"], rows["decoder_8"]
        spread = max(b["max"] - b["min"], d["max"] - d["min"])
        out["b8_batch_vs_8_decoder_steps"] = dict(batch_ms=b["ms_per_step"], decoder_ms=d["ms_per_step"], larger_spread_ms=round(spread, 4),
                                                  batch_is_faster_by_more_than_the_spread=bool(d["ms_per_step"] - b["ms_per_step"] > spread))
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
