"""Records tests/golden/decode_block_plans.json from a built checkout of the commit in front of csrc/block_plan.h with
block_plan_record.patch applied (tools/experiments/README.md):

    python tools/experiments/block_plan_record.py device <patched checkout> <device file>                       (on the MI355X)
    python tools/experiments/block_plan_record.py sweep  <patched checkout> <commit> <device file> <golden>     (no device needed)
    python tools/experiments/block_plan_record.py logs   <any built checkout> <file>                            (on the MI355X)

device: one real decoder per BASELINE shape and context (one block, gemma3 two; vocabulary 512): the inputs of plan_block it actually holds
        (mc_block_plan_inputs: its first block's three linears, nsplit, pv_ranges, the nine occupancy answers, the CU count) and the mc_attn_* launches
        of one eager token with their grids, next to what gemv_kernel_name("attn") says.
sweep:  the MEMBER plan_block asked through mc_block_plan_query -- a decoder without weights, filled with a shape, a model, an environment and a state;
        no HIP call -- for the BASELINE shapes with the device's occupancy answers, every switch of the block at its non-default value, the state
        variants and the edge shapes.  Every device case is asked too and has to name the kernel and the grid that decoder launched.
logs:   the launch log of one eager token and of one generate of 8 tokens for the same decoders -- run on the parent and on the tree under test,
        the two files are compared name by name (profiles/block_plan_dispatch_diff.md)."""
import ctypes as C
import json
import os
import sys

MODE, TREE = sys.argv[1], os.path.abspath(sys.argv[2])
sys.path[:0] = [TREE, os.path.join(TREE, "tests")]

import metalchat_amd as mc  # noqa: E402

assert mc.__file__.startswith(TREE), mc.__file__

I4, I8, BF = dict(weight_format=2, group_size=128), dict(weight_format=1, group_size=32), dict(weight_format=0, group_size=0)
GEMMA = dict(family=1, rope_sliding_theta=10000.0, sliding_stride=2)
SHAPES = {  # the BASELINE shapes: name -> (model widths, weight format, blocks)
    "tinyllama-bf16": (dict(dim=2048, n_heads=32, n_kv_heads=4, head_dim=64, ffn_dim=5632), BF, 1),
    "llama32-1b-bf16": (dict(dim=2048, n_heads=32, n_kv_heads=8, head_dim=64, ffn_dim=8192), BF, 1),
    "llama3-8b-i4": (dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336), I4, 1),
    "llama3-8b-i8": (dict(dim=4096, n_heads=32, n_kv_heads=8, head_dim=128, ffn_dim=14336), I8, 1),
    "gemma-7b-i4": (dict(dim=3072, n_heads=16, n_kv_heads=16, head_dim=256, ffn_dim=24576, **GEMMA), I4, 2),
    "llama3-70b-i4": (dict(dim=8192, n_heads=64, n_kv_heads=8, head_dim=128, ffn_dim=28672), I4, 1),
}
CONTEXTS = (1024, 2048, 4096, 8192)
ANSWER_FIELDS = ["form", "name", "tiles", "vsh", "ns", "grid", "fast", "chain_f", "chain_p", "qkv_gemv", "rope_kv", "wo_gemv", "pv_fold", "pv_ranges",
                 "pv_block", "pv_reduce", "uses_handoffs"]
INPUT_FIELDS = {"shape": "fmt out in group lora_cols of qkv, wo, w13", "model": "family n_heads n_kv_heads head_dim dim max_seq_len",
                "env": "tb qmode cus nsplit n_own granules pv_ranges occ_fused occ_wo occ_wo_w occ_wo_i8 occ_wo_qkn occ_qkv_qkn occ_qkv_only occ_wo_i4_wide occ_w13",
                "state": "attn_fused_on + 2 pending_pn"}


def decoder_cfg(name, S):
    widths, fmt, blocks = SHAPES[name]
    return dict(dtype=0, n_layers=blocks, vocab=512, max_seq_len=S, rope_theta=10000.0, norm_eps=1e-5, attn_scale=float(widths["head_dim"]) ** -0.5,
                use_graph=0, **widths, **fmt)


def lines(text):
    return [x for x in text.split("\n") if x]


def device_cases(with_inputs):
    lib = mc.capi()
    acc = mc.HardwareAccelerator()
    out = {"device": acc.name(), "cus": acc.compute_units(), "cases": {}}
    for name in SHAPES:
        for S in CONTEXTS:
            cfg = decoder_cfg(name, S)
            dec = mc.Decoder(acc, **cfg)
            dec.init_synthetic(7)
            case = {"cfg": cfg, "attn_name": dec.gemv_kernel_name("attn")}
            if with_inputs:
                a = (C.c_int * 37)()
                assert lib.mc_block_plan_inputs(dec._h, a) == 0
                case["shape"], case["env"] = list(a[:15]), list(a[21:37])
            dec.launch_log(True)
            dec.step(1, 0)
            case["step"] = dec.launched()
            if with_inputs:
                buf = C.create_string_buffer(1 << 16)
                assert lib.mc_block_plan_launches(dec._h, buf, 1 << 16) == 0
                case["attn_launches"] = [[t[0]] + [int(x) for x in t[1:]] for t in (x.split() for x in lines(buf.value.decode())) if t[0].startswith("mc_attn_")]
            dec.launch_log(False)
            dec.release()
            if not with_inputs:   # a chained call on a decoder of its own: the second token is captured (and logged), the others replay it
                dec = mc.Decoder(acc, **dict(cfg, use_graph=1))
                dec.init_synthetic(7)
                dec.launch_log(True)
                dec.generate(1, 0, 8)
                case["generate8"] = dec.launched()
                dec.launch_log(False)
                dec.release()
            out["cases"][f"{name}-s{S}"] = case
            print(name, S, case["attn_name"], flush=True)
    return out


if MODE in ("device", "logs"):
    with open(sys.argv[3], "w") as f:
        json.dump(device_cases(MODE == "device"), f, indent=1)
    sys.exit(0)

assert MODE == "sweep", __doc__
COMMIT, DEVICE_FILE, OUT_FILE = sys.argv[3], sys.argv[4], os.path.abspath(sys.argv[5])
with open(DEVICE_FILE) as f:
    DEV = json.load(f)
lib = C.CDLL(mc.library_path())
lib.mc_block_plan_query.restype = C.c_int
lib.mc_block_plan_query.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int]

tables = {"shapes": [], "models": [], "envs": [], "options": [], "answers": []}
records, sources = [], []


def index(table, v):
    t = tables[table]
    if v not in t:
        t.append(v)
    return t.index(v)


def ask(shape, model, env, fused_on, pending, switches, source):
    """one query under the MC_* switches; the record holds the decoder_options fields the query says it read"""
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        buf = C.create_string_buffer(1024)
        a = (C.c_int * 39)(*shape, *model, *env, int(fused_on), int(pending))
        assert lib.mc_block_plan_query(a, buf, 1024) == 0
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    opts, answer = buf.value.decode().split("|")
    rec = [index("shapes", list(shape)), index("models", list(model)), index("envs", list(env)), int(fused_on) + 2 * int(pending), index("options", opts),
           index("answers", answer), index_source(source)]
    if rec not in records:
        records.append(rec)
    return answer.split()


def index_source(s):
    if s not in sources:
        sources.append(s)
    return sources.index(s)


def inputs(name, S, cus=None, pv_ranges=None):
    """(shape, model, env) of a decoder of that BASELINE shape as mc_decoder_create fills them, with the occupancy answers the device gave"""
    widths = SHAPES[name][0]
    dev = DEV["cases"][f"{name}-s2048"]
    env = list(dev["env"])
    env[2] = cus or env[2]
    env[3] = (S + 63) // 64                                                         # nsplit
    env[6] = pv_ranges or (min(16, S // 2048) if S >= 8192 else 1)                  # pv_ranges (MC_PV_RANGES: mc_decoder_create)
    model = [widths.get("family", 0), widths["n_heads"], widths["n_kv_heads"], widths["head_dim"], widths["dim"], S]
    return list(dev["shape"]), model, env


def variants(name):
    return ((0, 1) if name.startswith("gemma") else (0,))


def everywhere(source, switches=None, contexts=CONTEXTS, cus=None, mutate=None, fused_on=1):
    for name in SHAPES:
        for S in contexts:
            for pending in variants(name):
                sw = dict(switches or {})
                shape, model, env = inputs(name, S, cus, int(sw["MC_PV_RANGES"]) if "MC_PV_RANGES" in sw else None)
                if mutate:
                    mutate(shape, env)
                ask(shape, model, env, fused_on, pending, sw, source)


# ---- 1. the device cases: the query names the kernel and the grid each real decoder launched
for case, c in sorted(DEV["cases"].items()):
    cfg = c["cfg"]
    model = [cfg.get("family", 0), cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"], cfg["dim"], cfg["max_seq_len"]]
    for li in range(cfg["n_layers"]):
        ans = ask(c["shape"], model, c["env"], 1, li > 0, {}, "device:" + case)
        launched = [x for x in c["attn_launches"] if not x[0].startswith(("mc_attn_pv_",))][li]
        assert ans[1] == launched[0], (case, ans, launched)
        if ans[0] != "scores_pv":
            assert int(ans[5]) == launched[1] and launched[2:4] == [1, 1], (case, ans, launched)
        else:
            pv = [x for x in c["attn_launches"] if x[0].startswith("mc_attn_pv_")]
            assert pv[0][3] == int(ans[13]) and pv[0][4] == int(ans[14]) and (len(pv) > cfg["n_layers"]) == (ans[15] == "1"), (case, ans, pv)
    first = ask(c["shape"], model, c["env"], 1, 0, {}, "device:" + case)
    assert c["attn_name"] == (first[1] + " + mc_attn_pv_bfloat" if first[0] == "scores_pv" else first[1]), (case, first)
    assert inputs(case.rsplit("-s", 1)[0], cfg["max_seq_len"]) == (c["shape"], model, c["env"]), case   # the sweep's inputs ARE a real decoder's

# ---- 2. the BASELINE shapes (cus = 256 on the recording device), then every switch at its non-default value
assert DEV["cus"] == 256, DEV["cus"]
everywhere("baseline")
SWITCHES = [{"MC_ATTN_FUSED": "0"}, {"MC_ATTN_FUSED_WGS": "1"}, {"MC_ATTN_FUSED_WGS": "4"}, {"MC_ATTN_T2": "0"}, {"MC_ATTN_WO": "0"}, {"MC_ATTN_WO_K4": "1"},
            {"MC_ATTN_QKV": "0"}, {"MC_ATTN_QKV_ONLY": "1"}, {"MC_ATTN_I8": "0"}, {"MC_ATTN_I4_WIDE": "0"}, {"MC_ATTN_QKV_QKN": "0"}, {"MC_ATTN_WO_QKN": "0"},
            {"MC_ATTN_QKN": "0"}, {"MC_KV_VIRTUAL": "0"}, {"MC_CHAIN_W13": "0"}, {"MC_CHAIN_F": "2"}, {"MC_CHAIN_F": "3"}, {"MC_CHAIN_F": "4"},
            {"MC_PV_FOLD": "0"}, {"MC_PV_RANGES": "4"}, {"MC_PV_BLOCK": "512"}, {"MC_HANDOFF_FAST": "0"}, {"MC_GEMV_LIN": "0"}, {"MC_LIN_WAVES": "4"},
            # ... and together, where one switch alone leaves the arm it belongs to unreached
            {"MC_ATTN_QKV": "0", "MC_ATTN_WO": "0"}, {"MC_ATTN_QKV": "0", "MC_ATTN_WO": "0", "MC_ATTN_T2": "0"}, {"MC_ATTN_QKV": "0", "MC_ATTN_WO": "0", "MC_HANDOFF_FAST": "0"},
            {"MC_ATTN_WO_QKN": "0", "MC_ATTN_QKN": "0"}, {"MC_ATTN_QKV": "0", "MC_ATTN_WO_K4": "1"},
            {"MC_ATTN_FUSED": "0", "MC_PV_FOLD": "0"}, {"MC_ATTN_FUSED": "0", "MC_PV_RANGES": "4"}, {"MC_ATTN_FUSED": "0", "MC_PV_FOLD": "0", "MC_PV_RANGES": "4"},
            {"MC_ATTN_FUSED": "0", "MC_PV_BLOCK": "512"}, {"MC_ATTN_FUSED": "0", "MC_PV_FOLD": "0", "MC_PV_BLOCK": "512"}, {"MC_ATTN_FUSED": "0", "MC_GEMV_LIN": "0"}]
for sw in SWITCHES:
    everywhere("switch", sw)

# ---- 3. the state variants
everywhere("state:fallen-back", fused_on=0)
for i in range(9):
    everywhere(f"state:occ{i}=0", mutate=lambda shape, env, i=i: env.__setitem__(7 + i, 0))
everywhere("state:occ-not-asked", mutate=lambda shape, env: env.__setitem__(slice(7, 16), [-1] * 9))
everywhere("state:tb4", mutate=lambda shape, env: (env.__setitem__(0, 4), env.__setitem__(5, 0)))
everywhere("state:n_own255", mutate=lambda shape, env: env.__setitem__(4, 255))
for i, which in enumerate(("qkv", "wo", "w13")):
    everywhere("state:adaptor-" + which, mutate=lambda shape, env, i=i: shape.__setitem__(5 * i + 4, 16))

# ---- 4. the edge shapes: partial ranges, and the CU counts at which the one-workgroup-per-CU gates flip
everywhere("edge:partial-ranges", contexts=(2040, 4040))
everywhere("edge:partial-ranges", {"MC_ATTN_FUSED": "0"}, contexts=(2040, 4040))
for cus in (192, 304):
    everywhere(f"edge:cus{cus}", cus=cus)

head = {"recorded_from": COMMIT, "device": DEV["device"], "cus": DEV["cus"], "input_fields": INPUT_FIELDS, "answer_fields": ANSWER_FIELDS,
        "type_name": "bfloat where tb == 2, else float",
        "record_fields": ["shape (index)", "model (index)", "env (index)", "state", "options (index)", "answer (index)", "source (index)"]}
device = {k: {"cfg": c["cfg"], "attn_name": c["attn_name"], "attn_launches": c["attn_launches"]} for k, c in sorted(DEV["cases"].items())}
with open(OUT_FILE, "w") as f:
    f.write("{\n")
    for k, v in head.items():
        f.write(json.dumps(k) + ": " + json.dumps(v) + ",\n")
    for k, v in tables.items():
        f.write(json.dumps(k) + ": [\n" + ",\n".join(" " + json.dumps(x) for x in v) + "],\n")
    f.write('"sources": ' + json.dumps(sources) + ",\n")
    f.write('"device_cases": {\n' + ",\n".join(" " + json.dumps(k) + ": " + json.dumps(v) for k, v in device.items()) + "},\n")
    f.write('"records": [\n' + ",\n".join(" " + ", ".join(json.dumps(r) for r in records[i:i + 8]) for i in range(0, len(records), 8)) + "\n]}\n")
with open(OUT_FILE) as f:
    json.load(f)
print("recorded", len(records), "records,", len(tables["answers"]), "different answers, forms:", sorted({a.split()[0] for a in tables["answers"]}))
