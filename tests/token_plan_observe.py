"""What a case of tests/golden/decode_token_plans.json launches and computes on a fresh decoder: shared by the recorder
(tools/experiments/token_plan_record.py, on the commit the golden names) and test_token_plan_gpu.py (on this tree)."""
import hashlib
import json
import os

import metalchat_amd as mc
import modelgen as mg

_weights = {}


def make_decoder(acc, c, extra_env):
    """a fresh decoder of the case, created under its switches (read once, at creation)"""
    env = dict(c["env"], **extra_env)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dec = mc.Decoder(acc, **c["cfg"])
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    if c["weights"] is None:
        dec.init_synthetic(7)
    else:
        key = json.dumps([c["cfg"], c["weights"]], sort_keys=True)
        if key not in _weights:
            w = dict(c["weights"])
            if w.get("lora_only"):
                w["lora_only"] = tuple(w["lora_only"])
            full = dict(c["cfg"], layer_begin=0, layer_end=c["cfg"]["n_layers"])
            _weights[key] = mg.make_model(full, **w)
        dec.load_model(_weights[key])
    if c["taps"]:
        dec.set_taps(True)
    if c["sampler"] != "greedy":
        dec.set_sampler(mc.SAMPLER_DEFAULT if c["sampler"] == "default" else mc.SAMPLER_DRAW, top_k=50, temperature=0.6, top_p=0.9)
        dec.set_seeds([[2 * i + 1, 2 * i + 2] for i in range(4)])
    return dec


def observe(acc, c, extra_env=None):
    """what the case launches and computes: {"step0": names, "step1": names [, "generate": names, "tokens": [...], "logits_sha256": hex]}"""
    dec = make_decoder(acc, c, extra_env or {})
    cfg = c["cfg"]
    first, last = cfg["layer_begin"] == 0, cfg["layer_end"] == cfg["n_layers"]
    inbound = None if first else dec.hidden_in_ptr()
    out = {}

    def logged(f):
        dec.launch_log(True)
        r = f()
        names = dec.launched()
        dec.launch_log(False)
        return names, r

    out["step0"], _ = logged(lambda: dec.step(1, 0, inbound))
    out["step1"], _ = logged(lambda: dec.step(-1, 1, inbound))
    if first and last:
        out["generate"], tokens = logged(lambda: dec.generate(3, 0, 4))
        out["tokens"] = [int(t) for t in tokens]
    if last:
        out["logits_sha256"] = hashlib.sha256(dec.logits().tobytes()).hexdigest()
    out["handoff_fallbacks"] = dec.handoff_fallbacks()
    dec.release()
    return out
