"""Records tests/golden/prompt_plans.json on the device from a built checkout of the commit in front of csrc/prefill_plan.h with
prefill_plan_record.patch applied (tools/experiments/README.md):

    python tools/experiments/prefill_plan_record.py <patched checkout> <commit> <output file>

1. every case of that checkout's tests/test_prefill_plan_gpu.py runs under MC_PREFILL_PLAN_RECORD: the GEMM, rope and attention launches as made;
2. every launched GEMM decision is asked again of plan_gemm through mc_prefill_plan_query: the name the query forms is the launched one;
3. plan_gemm / plan_attention are asked at the widths of Llama-3-8B, Gemma-7B, Llama-3.2-1B, TinyLlama (decoders of one block, no weights)."""
import ctypes as C
import json
import os
import sys

PARENT, COMMIT, OUT_FILE = os.path.abspath(sys.argv[1]), sys.argv[2], os.path.abspath(sys.argv[3])
sys.path[:0] = [PARENT, os.path.join(PARENT, "tests")]
REC = OUT_FILE + ".launches.txt"

import metalchat_amd as mc  # noqa: E402
import modelgen as mg  # noqa: E402
import test_prefill_plan_gpu as T  # noqa: E402

assert mc.__file__.startswith(PARENT), mc.__file__

# MC_* switch -> (decoder_options field, value) as read_options reads it
FIELD = {
    ("MC_PF_FOLD", "0"): {"pf_fold_on": 0}, ("MC_PF_FOLD", "1"): {"pf_fold_on": 1}, ("MC_PF_GEMM8", "0"): {"pf_g8_on": 0},
    ("MC_PF_NORM2", "0"): {"pf_norm2": 0}, ("MC_PF_NORM2", "1"): {"pf_norm2": 1},
    ("MC_PF_BLASLT", "1"): {},  # (lib_on of the environment line, no option the plan reads)
    ("MC_PF_ATTN_HEADS", "2"): {"pf_attn_heads": 2}, ("MC_PF_ATTN8_PAIR", "0"): {"pf_attn8_pair": 0},
}


def options_of(env):
    out = {}
    for kv in env.items():
        out.update(FIELD[kv])
    return out


def parse(line, options, source):
    kind, env, args, answer = line.rstrip("\n").split("|")
    return {"kind": kind, "env": [int(x) for x in env.split()], "args": [int(x) for x in args.split()], "options": options, "answer": answer,
            "source": source}


records = []
acc = mc.HardwareAccelerator()
lib = mc.capi()
lib.mc_prefill_plan_query.restype = C.c_int
lib.mc_prefill_plan_query.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]


def query(dec, kind, args):
    buf = C.create_string_buffer(1024)
    a = (C.c_int * 8)(*args)
    assert lib.mc_prefill_plan_query(dec._h, kind, a, buf, 1024) == 0
    return buf.value.decode()


# ---- 1. the launches of every case of test_prefill_plan_gpu.py, as they were made
os.environ["MC_PREFILL_PLAN_RECORD"] = REC
launched = {}
for case in sorted(T.CASES):
    if os.path.exists(REC):
        os.remove(REC)
    names = T.launch_log(acc, case)
    launched[case] = names
    opts = options_of(T.CASES[case][3])
    seen = set()
    for line in open(REC):
        if line not in seen:   # (the blocks of a model repeat their decisions)
            seen.add(line)
            records.append(parse(line, opts, "launch:" + case))
    print(case, len(seen), "decisions", flush=True)
del os.environ["MC_PREFILL_PLAN_RECORD"]
golden_logs = json.load(open(os.path.join(PARENT, "tests", "golden", "prompt_launch_logs.json")))["cases"]
assert launched == golden_logs, "the parent's launch logs are not the recorded ones"


def decoder(cfg_over, env, **kw):
    cfg = mg.tiny_cfg(mg.BF16, **cfg_over)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return mc.Decoder(acc, **mg.decoder_kwargs(cfg, **kw))
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


# ---- 2. every launched GEMM decision asked again of plan_gemm directly: the name the query forms is the name gemm_run launched
n_checked = 0
for case in sorted(T.CASES):
    name, _, _, switches, _ = T.CASES[case]
    cfg, _ = T.model(name)
    dec = decoder({k: cfg[k] for k in cfg if k != "dtype"}, switches, **T.MODELS[name][3]) if cfg["dtype"] == mg.BF16 else None
    for r in [r for r in records if r["kind"] == "gemm" and r["source"] == "launch:" + case]:
        if dec is None:
            continue
        q = parse(query(dec, 0, r["args"][:7]), r["options"], "query")
        want = r["answer"].replace("mc_pf_gemm8_w_", "mc_pf_gemm8_i4_") if r["args"][7] else r["answer"]
        assert q["env"] == r["env"] and q["answer"] == want, (r, q)
        n_checked += 1
    if dec is not None:
        dec.release()
print("launched GEMM decisions confirmed by the query:", n_checked, flush=True)
assert n_checked > 20

# ---- 3. the real shapes the small cases cannot reach: a decoder of that config (one block, a small vocabulary), no weights
SHAPES = {
    "llama3-8b": dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336),
    "tinyllama": dict(dim=2048, n_heads=32, n_kv_heads=4, head_dim=64, ffn_dim=5632),
    "llama32-1b": dict(dim=2048, n_heads=32, n_kv_heads=8, head_dim=64, ffn_dim=8192),
    "gemma-7b": dict(family=1, dim=3072, n_heads=16, n_kv_heads=16, head_dim=256, ffn_dim=24576, rope_sliding_theta=10000.0, sliding_stride=2),
    "hd32": dict(dim=256, n_heads=8, n_kv_heads=2, head_dim=32, ffn_dim=512),
}
ATTN_M = [16, 17, 496, 497, 512, 513, 1023, 1024, 1792, 1793, 1920, 1921, 1984, 1985, 2016, 2017, 2048]   # both sides of every threshold at 256 CUs
GEMM_M = [2, 64, 65, 256, 257, 512, 2048]
I4, I8, BF = (2, 128), (1, 32), (0, 0)  # (fmt, group): int4 g128, int8 g32, plain bfloat16


def linears(s):
    H, KV, hd, dim, ffn = s["n_heads"], s["n_kv_heads"], s["head_dim"], s["dim"], s["ffn_dim"]
    return {"qkv": ((H + 2 * KV) * hd, dim), "wo": (dim, H * hd), "w13": (2 * ffn, dim), "w2": (dim, ffn)}


def gemms(dec, model, s, switches, fmt=I4, lora=0, extra=None, Ms=GEMM_M):
    """epilogue 0 of the four linears at every M; extra: (linear, epilogue) asked too"""
    for which, (out, inn) in linears(s).items():
        for M in Ms:
            for epi in (0,) + ((extra[1],) if extra and extra[0] == which else ()):
                records.append(parse(query(dec, 0, [fmt[0], out, inn, fmt[1], lora, M, epi]), options_of(switches), f"query:{model}"))


for model, s in SHAPES.items():
    over = dict(s, n_layers=1, vocab=512, max_seq_len=4096)
    big = model == "llama3-8b"
    for switches, Ms in [({}, ATTN_M)] + ([({"MC_PF_ATTN_HEADS": "2"}, [497, 1024, 2048]), ({"MC_PF_ATTN8_PAIR": "0"}, [497, 1024, 2048])] if big else []):
        dec = decoder(over, switches, weight_format=2, group_size=128)
        for M in Ms:
            records.append(parse(query(dec, 1, [M]), options_of(switches), "query:" + model))
        dec.release()
    if model in ("tinyllama", "hd32"):
        continue
    dec = decoder(over, {}, weight_format=2, group_size=128)
    gemms(dec, model, s, {}, extra=("w13", 4 if s.get("family") else 3))   # the activation epilogue does not split
    if big:
        gemms(dec, model, s, {}, fmt=I8)
        gemms(dec, model, s, {}, fmt=BF)
        gemms(dec, model, s, {}, lora=16, Ms=[64, 65, 512])
    dec.release()
    dec = decoder(over, {"MC_PF_BLASLT": "1"}, weight_format=2, group_size=128)
    gemms(dec, model, s, {"MC_PF_BLASLT": "1"}, extra=("wo", 1))           # the library takes a plain store, not a residual
    dec.release()
    if big:
        dec = decoder(over, {"MC_PF_GEMM8": "0"}, weight_format=2, group_size=128)
        gemms(dec, model, s, {"MC_PF_GEMM8": "0"})
        dec.release()
    print(model, len(records), "records", flush=True)

envs, optsets = [], []


def index(table, v):
    if v not in table:
        table.append(v)
    return table.index(v)


head = {"recorded_from": COMMIT, "device": acc.name(), "cus": records[0]["env"][3],
        "env_fields": ["tb", "qmode", "family", "cus", "dim", "ffn_dim", "n_heads", "n_kv_heads", "head_dim", "max_seq_len", "lib_on"],
        "args_fields": {"gemm": "fmt out in group lora_cols M epi plain_copy", "attn": "M", "packed": "ntiles", "rope": "M parts batch qk_norm",
                        "extend": "tree"},
        "answer_fields": {"gemm": "family name gx gy splits block ktper bm", "attn": "name gx gy block", "packed": "name gx gy block",
                          "rope": "name gx gy block", "extend": "sums pv reduce heads"},
        "record_fields": ["kind", "env (index)", "options (index)", "args", "answer", "source"]}
rows = [[r["kind"], index(envs, r["env"]), index(optsets, r["options"]), " ".join(str(x) for x in r["args"]), r["answer"], r["source"]]
        for r in records]
with open(OUT_FILE, "w") as f:
    f.write("{\n")
    for k, v in head.items():
        f.write(json.dumps(k) + ": " + json.dumps(v) + ",\n")
    f.write('"envs": ' + json.dumps(envs) + ",\n" + '"options": ' + json.dumps(optsets) + ",\n" + '"records": [\n')
    f.write(",\n".join(json.dumps(r) for r in rows))
    f.write("\n]}\n")
print("recorded", len(records), "records ok")
