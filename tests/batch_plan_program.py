"""tests/cpp/test_batch_plan -- a plain g++ program over metalchat_amd/csrc/batch_plan.h, the header the batch's host units (batch.cc and its
three siblings) take every launch from -- asked from Python: requests as lines, answers as JSON (the formats: the program's header comment)."""
import json
import subprocess

from metalchat_amd import build as b

WFMT_T, WFMT_I8, WFMT_I4 = 0, 1, 2
LINEAR_KEYS = ("fmt", "out", "in", "group", "ngroups", "lora", "lora_cols")


def linear(fmt, out, in_, group=0, lora_cols=0):
    return {"fmt": fmt, "out": out, "in": in_, "group": group, "ngroups": in_ // group if group else 1, "lora": int(lora_cols > 0), "lora_cols": lora_cols}


def words(*items):
    out = []
    for w in items:
        if isinstance(w, dict):
            out += [w[k] for k in LINEAR_KEYS]
        elif isinstance(w, (list, tuple)):
            out += list(w)
        else:
            out.append(w)
    return " ".join(w if isinstance(w, str) else repr(float(w)) if isinstance(w, float) else str(int(w)) for w in out)


def linears_of(cfg, fmt=WFMT_T, group=0, lora_rank=0, head_fmt=None, head_group=None):
    """the five fused matrices of a llama3 decoder of shape cfg in one format (adaptors of lora_rank on every layer linear)"""
    H, KV, hd, dim, ffn = cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"], cfg["dim"], cfg["ffn_dim"]
    return dict(qkv=linear(fmt, (H + 2 * KV) * hd, dim, group, 3 * lora_rank), wo=linear(fmt, dim, H * hd, group, lora_rank),
                w13=linear(fmt, 2 * ffn, dim, group, 2 * lora_rank), w2=linear(fmt, dim, ffn, group, lora_rank),
                output=linear(fmt if head_fmt is None else head_fmt, cfg["vocab"], dim, group if head_group is None else head_group))


def admit(cfg, linears, wide, *, emb_fmt=WFMT_T, weight_format=None, group_size=None, **over):
    """the admission of a decoder: cfg (the shape words of mc_decoder_config), its linears; over: any config word set otherwise"""
    c = dict(family=0, dtype=0, layer_begin=0, layer_end=cfg["n_layers"], n_layers=cfg["n_layers"],
             weight_format=linears["qkv"]["fmt"] if weight_format is None else weight_format,
             group_size=linears["qkv"]["group"] if group_size is None else group_size, qmode=0, head_dim=cfg["head_dim"], n_heads=cfg["n_heads"],
             n_kv_heads=cfg["n_kv_heads"], max_seq_len=cfg["max_seq_len"], dim=cfg["dim"], vocab=cfg["vocab"])
    c.update(over)
    layer = [linears[k] for k in ("qkv", "wo", "w13", "w2")]
    return words("admit", int(wide), *[c[k] for k in ("family", "dtype", "layer_begin", "layer_end", "n_layers", "weight_format", "group_size", "qmode",
                                                     "head_dim", "n_heads", "n_kv_heads", "max_seq_len", "dim", "vocab")],
                 emb_fmt, cfg["n_layers"], *(layer * cfg["n_layers"]), linears["output"])


def gemv(lin, epi, B, cus=256, tiles_env=0):
    return words("gemv", lin, epi, B, cus, tiles_env)


def step(cfg, B, ragged=False, rolling=False):
    return words("step", cfg["dim"], cfg["n_heads"], cfg["n_kv_heads"], cfg["head_dim"], B, (cfg["max_seq_len"] + 63) // 64, int(ragged), int(rolling))


def cand_per_row(vocab):
    """the candidate keys a batch holds per row -- a restatement of the allocation in batch.cc batch_create, not read from the host"""
    return max((vocab + 511) // 512, 1) * 128


def head(vocab, ragged, dec_sampler, rows):
    """dec_sampler, rows[r]: (kind, top_k, temperature, top_p), kind -1 = the row inherits"""
    return words("head", vocab, int(ragged), cand_per_row(vocab), [float(x) if i > 1 else x for i, x in enumerate(dec_sampler)], len(rows),
                 *[[float(x) if i > 1 else x for i, x in enumerate(r)] for r in rows])


def logits(vocab, ragged, rows):
    """rows[r]: (masked, repetition, frequency, presence)"""
    return words("logits", vocab, int(ragged), len(rows), *[[int(r[0]), float(r[1]), float(r[2]), float(r[3])] for r in rows])


def verify(head_linear, cfg, M, nseg, tree):
    return words("verify", head_linear, cfg["vocab"], cfg["n_kv_heads"], cfg["head_dim"], cfg["n_layers"], M, nseg, int(tree))


def ragged(what, positions, tokens, lengths, *, max_seq_len, vocab, rolling=False, n=1):
    assert len(positions) == len(tokens) == len(lengths)
    return words("ragged", what, len(positions), max_seq_len, vocab, int(rolling), n, positions, tokens, lengths)


def settings(who, lens, *, dec_kind=0, kinds=None, logit_rows=None):
    B = len(lens)
    kinds = [-1] * B if kinds is None else kinds
    logit_rows = [(0, 1.0, 0.0, 0.0)] * B if logit_rows is None else logit_rows
    return words("settings", who, B, dec_kind, lens, kinds, *[[int(r[0]), float(r[1]), float(r[2]), float(r[3])] for r in logit_rows])


def ask(lines):
    """the program's answer to each request line"""
    exe = b.build_batch_plan_test()
    out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout
    answers = [json.loads(a) for a in out.split("\n")[:-1]]
    assert len(answers) == len(lines)
    return answers


INHERITS, UNSET = (-1, 0, 0.0, 0.0), (0, 1.0, 0.0, 0.0)


def token(cfg, linears, B, *, cus, tiles_env=0, ragged_call=False, rolling=False, dec_sampler=(0, 50, 0.6, 0.9), row_samplers=(), row_logits=(), logprobs=None,
          tail=False):
    """the request for the ordered launches of ONE token of a step call (tail: of the head behind a prompt pass).
    row_samplers: (row, kind, top_k, temperature, top_p) of the rows that do not inherit; row_logits: (row, masked, rep, freq, pres); logprobs: top_n"""
    srows, lrows = [INHERITS] * B, [UNSET] * B
    for r, *s in row_samplers:
        srows[r] = tuple(s)
    for r, *s in row_logits:
        lrows[r] = tuple(s)
    floats = lambda t, first: [float(x) if i >= first else x for i, x in enumerate(t)]
    return words("tail" if tail else "token", [cfg[k] for k in ("dim", "n_heads", "n_kv_heads", "head_dim", "n_layers", "vocab", "max_seq_len")], B, cus, tiles_env,
                 int(ragged_call), int(rolling), *[linears[n] for n in ("qkv", "wo", "w13", "w2", "output")], floats(dec_sampler, 2),
                 *[floats(r, 2) for r in srows], *[[int(r[0])] + floats(r[1:], 0) for r in lrows], int(logprobs is not None), logprobs or 0)


def token_launches(cfg, linears, B, **kw):
    """the launches of ONE token of a step call as plan_batch_token (batch_call_plan.h) orders them -- the list the batch's executor walks, so a
    comparison with a recording pins what each launch holds (name, grid, block, LDS), the order, and which plan sits at which place (wo against w2)"""
    return ask([token(cfg, linears, B, **kw)])[0]["launches"]


def head_launches(cfg, linears, B, *, cus, tiles_env=0):
    """the head of a rows pass (mc_rows_prefill, mc_extend_rows) as plan_rows_tail orders it: the final norm, the head GEMV and the ragged pick, no
    row settings"""
    return ask([token(cfg, linears, B, cus=cus, tiles_env=tiles_env, tail=True)])[0]["launches"]


_FORMED = []


def formed_names():
    """every kernel name the plans form over {format} x {epilogue} x {adaptor or not} x {B = 8, 64} x {lockstep, ragged, rolling} x {the three
    pick forms} x {logit launch or not} x {verify, tree}"""
    if _FORMED:
        return _FORMED[0]
    cfg = dict(dim=1024, n_heads=8, n_kv_heads=2, head_dim=128, ffn_dim=2048, n_layers=1, vocab=2048, max_seq_len=256)
    sampling, other = (1, 50, 0.6, 0.9), (1, 20, 0.7, 0.8)
    lines = []
    for fmt in (WFMT_T, WFMT_I8, WFMT_I4):
        for lora_cols in (0, 16):
            lin = linear(fmt, 2048, 1024, 32 if fmt != WFMT_T else 0, lora_cols)
            lines += [gemv(lin, epi, B) for epi in (0, 1, 2) for B in (8, 64)]
            lines += [verify(lin, cfg, 8, 2, tree) for tree in (False, True)]
    for B in (8, 64):
        lines += [step(cfg, B, ragged_, rolling) for ragged_, rolling in ((False, False), (True, False), (True, True))]
        for ragged_ in (False, True):
            lines += [head(cfg["vocab"], ragged_, dec, rows) for dec, rows in (((0, 50, 0.6, 0.9), [(-1, 0, 0.0, 0.0)] * B), (sampling, [(-1, 0, 0.0, 0.0)] * B),
                                                                          (sampling, [other] + [(-1, 0, 0.0, 0.0)] * (B - 1)))]
            lines += [logits(cfg["vocab"], ragged_, [(m, 1.0, 0.0, 0.0)] + [(0, 1.0, 0.0, 0.0)] * (B - 1)) for m in (0, 1)]
    names = set()
    for a in ask(lines):
        names |= names_in(a)
    _FORMED.append(frozenset(names))
    return _FORMED[0]


def names_in(answer):
    """the kernel names of an answer: the first word of every launch in it"""
    found = set()

    def walk(v):
        if isinstance(v, list) and len(v) == 6 and isinstance(v[0], str) and all(isinstance(x, int) for x in v[1:]):
            found.add(v[0])
        elif isinstance(v, list):
            for x in v:
                walk(x)
        elif isinstance(v, dict):
            for x in v.values():
                walk(x)

    walk(answer)
    return found
