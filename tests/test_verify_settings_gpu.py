"""Verify calls for sampling, masked and penalised rows (mc_settings_verify_set, include/metalchat_hip.h Part 2m) on the device, SMALL int4 g128
seed 11 and one wide QLoRA-admitted batch at B = 17.

  * switch off: today's refusals; switch on with every row greedy and unprocessed: picks, accepted, K / V, logits and the launch log are
    those of the same call with the switch off;
  * a mixed batch (greedy / default / draw rows, two with a mask, two with penalties and prior counts): every pick is the rule applied to
    the device's OWN verify_logits() row with pair (j * B + r) % n_pairs; accepted / next_tokens are verify_rule's walk over those picks;
    the lengths follow; the counts afterwards are the counts before plus the fed tokens; the unprocessed rows' logits are the switch-off
    call's, bit for bit, and the processed rows logits_rule of them with the counts c + hist(chunk[0 .. j]);
  * equivalence with decoding: the drafts are the row's own generate_rows continuation under the same seed array.  The chunk pass is not
    bit-identical to the step path (the existing tests allow it 2 ulp), so picks are compared only at positions that the ORACLE, fed the
    same tokens, calls stable: the rule's pick from the oracle's logits survives every perturbation of `perturbations` (all logits up /
    down two bfloat16 steps, the picked token against the rest both ways, and random steps in [-2, 2] per logit) -- which moves t away from
    both ends of the picked interval and the candidates away from the top-k and nucleus cuts.  At least half of each row's chain must be
    compared and at least 8 compared draw picks must differ from the argmax (with the oracle's own chain on the CPU: 71 of 96 positions
    stable, 8 to 10 per row, 15 compared draws off the argmax for these seeds); at those positions the picks are the generated tokens, and a row whose
    positions are all stable is accepted whole with the generated next token;
  * a planted wrong draft at index 0 / middle / last gives accepted exactly that index (the plant sits behind a stable prefix);
  * a chain tree equals mc_verify_rows, bit for bit, on a draw row with penalties; a real tree counts its accepted path and draws by depth;
  * placement and company: the same row at another index, in another batch size and other company gives the same bits;
  * four rounds of the loop with fresh pairs per call."""
import numpy as np
import pytest

import draw_rule as dr
import logits_rule as lr
import modelgen as mg
import parity
import tree_rule as tr
import verify_rule as vr
from oracle import mc_oracle as mo
from test_batch_gpu import SMALL, refused, small_decoder
from test_context_gpu import random_cache
from test_rows_prefill_gpu import prompts_of

pytestmark = pytest.mark.gpu
BF16 = 0
GREEDY_K, DEFAULT_K, DRAW_K = 0, 1, 2
GREEDY = (GREEDY_K,)
POS = [5, 7, 16, 40, 63, 3, 64, 20]
N_PAIRS = 37   # a prime: (j * B + r) % n_pairs wraps inside a call
NEW = ["mc_vs_logits_process_bfloat", "mc_vs_topk_candidates_mixed_bfloat", "mc_vs_pick_mixed_bfloat", "mc_vs_count_accepted"]
# the mixed batch: row -> (sampler, a mask or None, penalties or None); a row with penalties starts with the 40 tokens of history_of counted
MIXED = [(GREEDY, None, None), ((DRAW_K, 40, 0.9, 0.95), None, None), ((DEFAULT_K, 5, 1.5, 0.5), None, None), ((DRAW_K, 5, 1.5, 0.5), None, None),
         (GREEDY, "mask", None), ((DRAW_K, 50, 0.8, 0.9), "mask", None), ((DRAW_K, 20, 1.0, 1.0), None, (1.3, 0.25, 0.5)), (GREEDY, None, (1.5, 0.5, 0.0))]


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


def pairs_of(seed, n=N_PAIRS):
    rng = np.random.default_rng(seed)
    return [(int(a), int(b)) for a, b in rng.integers(0, 2 ** 63, (n, 2))]


def pick_rule(bits, sampler, pair):
    """what `sampler` picks from one row of bfloat16 logits with the seed pair `pair`"""
    if sampler[0] == GREEDY_K:
        return lr.first_max(bits)
    if sampler[0] == DEFAULT_K:
        return int(mo.sample_default(BF16, bits, top_k=sampler[1], temperature=sampler[2], top_p=sampler[3], init_state=pair[0], init_seq=pair[1]))
    return int(dr.draw(BF16, bits, sampler[1], sampler[2], sampler[3], pair[0], pair[1]))


def allowed_of(r, vocab):
    """row r's mask: about a quarter of the vocabulary banned"""
    return np.random.default_rng(900 + r).random(vocab) > 0.25


def history_of(r, vocab):
    return np.random.default_rng(950 + r).integers(0, vocab, 40).astype(np.int32)


def apply_settings(batch, settings, vocab):
    for r, (sampler, mask, pen) in enumerate(settings):
        batch.set_row_sampler(r, *sampler)
        if mask is not None:
            batch.set_row_mask(r, allowed_of(r, vocab))
        if pen is not None:
            batch.set_row_penalties(r, *pen)
            batch.count_row_tokens(r, history_of(r, vocab))


def fresh(dec, cfg, positions, seed, settings=None, pairs=None, on=True, wide=False, rows=None):
    """a batch whose row rows[i] holds the random context (positions[i], seed + 100 i + layer); settings per batch row"""
    import metalchat_amd as mc

    rows = list(range(len(positions))) if rows is None else rows
    B = len(settings) if settings is not None else max(rows) + 1
    b = mc.Batch(dec, B, wide=wide)
    for i, (r, p) in enumerate(zip(rows, positions)):
        for layer in range(cfg["n_layers"]):
            b.import_kv(r, layer, *random_cache(cfg, p, seed + 100 * i + layer))
    if settings is not None:
        apply_settings(b, settings, cfg["vocab"])
    if pairs is not None:
        b.set_seeds(pairs)
    if on:
        b.set_verify_settings(True)
    return b


def check_call(batch, settings, call, pos, pairs, result, raw, counts_before, what, parents=None, paths=None):
    """the assertions of one verify call with row settings: `result` = (accepted, next, picks); raw[r]: the rows' unprocessed logits (a
    switch-off call's) or None to skip that comparison; parents[r] / paths: a tree call"""
    accepted, nxt, picks = result
    B, vocab = batch.B, batch.cfg["vocab"]
    vl, logits, lengths = batch.verify_logits(), batch.logits(), batch.lengths()
    for r in range(B):
        if call[r] is None:
            assert accepted[r] == nxt[r] == -1 and picks[r] is None and vl[r] is None, (what, r)
            continue
        sampler, mask, pen = settings[r]
        c = np.asarray(call[r])
        for j in range(len(c)):
            d = j if parents is None else tr.depths(parents[r])[j]
            want = pick_rule(vl[r][j], sampler, pairs[(d * B + r) % len(pairs)])
            assert picks[r][j] == want, (what, r, j, sampler, picks[r][j], want)
            if mask is not None:
                assert allowed_of(r, vocab)[picks[r][j]], (what, r, j, "a banned token was picked")
            if raw is not None:
                fed = c[:j + 1] if parents is None else c[tr.ancestors(parents[r], j)]
                cnt = counts_before[r] + np.bincount(fed, minlength=vocab) if pen is not None else None
                exp = lr.process(raw[r][j], cnt, allowed_of(r, vocab) if mask is not None else None, *(pen or (1.0, 0.0, 0.0)))
                parity.exact(vl[r][j], exp, f"{what} row {r} chunk row {j}: the processed logits against the rule")
                if mask is None and pen is None:
                    parity.exact(vl[r][j], raw[r][j], f"{what} row {r} chunk row {j}: an unprocessed row keeps every bit")
        if parents is None:
            assert (accepted[r], nxt[r]) == vr.accept(c, picks[r]), (what, r, accepted[r], nxt[r])
            fed = c[:accepted[r] + 1]
        else:
            a, n, path = tr.walk(c, parents[r], picks[r])
            assert (accepted[r], nxt[r], list(paths[r])) == (a, n, path), (what, r)
            fed = c[path]
        assert lengths[r] == pos[r] + accepted[r] + 1, (what, r)
        parity.exact(logits[r], vl[r][accepted[r] if parents is None else paths[r][-1]], f"{what} row {r}: the batch's logits are the accepted row's")
        after = batch.row_token_counts(r)
        exp_counts = counts_before[r] + (np.bincount(fed, minlength=vocab) if pen is not None else 0)
        parity.exact(after, exp_counts.astype(np.int32), f"{what} row {r}: the counts are those before plus the fed tokens")


def grow_drafts(make, first, pos, n, rounds):
    """chunks [first[r], drafts ...] of n tokens whose first `rounds` drafts are what the rows themselves pick: round k runs the call on a fresh
    batch and takes pick k -- it depends on chunk[0 .. k] alone.  The rest stays random (rejected for certain: 2047 in 2048 per draft)"""
    rng = np.random.default_rng(77)
    call = [None if f is None else np.concatenate([[f], rng.integers(0, SMALL["vocab"], n[r] - 1)]).astype(np.int32) for r, f in enumerate(first)]
    for k in range(rounds):
        b = make()
        _, _, picks = b.verify_rows(call, pos)
        b.release()
        for r, c in enumerate(call):
            if c is not None and k + 1 < len(c):
                c[k + 1] = picks[r][k]
    return call


# ------------------------------------------------------------------------------------------ 1
def test_switch_off_refuses_and_on_with_greedy_rows_is_the_call_of_before(acc, small):
    cfg, L = SMALL, SMALL["n_layers"]
    dec = small_decoder(acc, cfg, small)
    lens = [2, 16, 5, 16, 9, 3, 16, 12]
    prompts = prompts_of(cfg, lens, 41)
    off = fresh(dec, cfg, POS, 600, on=False)
    assert off.verify_settings() is False
    off.set_row_sampler(1, DRAW_K, 40, 0.9, 0.95)
    dec.launch_log(True)
    refused(lambda: off.verify_rows(prompts, POS), "mc_verify_rows: row 1: the row's sampler is not greedy (accepting sampled drafts needs the draft's probabilities)")
    off.set_row_sampler(1, GREEDY_K)
    off.set_row_mask(2, allowed_of(2, cfg["vocab"]))
    refused(lambda: off.verify_rows(prompts, POS), "mc_verify_rows: row 2: the row has a token mask or penalties (a verify call would need them per chunk row)")
    refused(lambda: off.verify_tree(prompts, [tr.chain(n) for n in lens], POS), "mc_tree_verify: row 2: the row has a token mask or penalties")
    off.set_row_mask(2, None)
    off.set_row_penalties(3, 1.2, 0.0, 0.0)
    refused(lambda: off.verify_rows(prompts, POS), "mc_verify_rows: row 3: the row has a token mask or penalties")
    assert dec.launched() == []
    off.set_row_penalties(3, 1.0, 0.0, 0.0)
    off.set_row_sampler(1, -1)
    # a sampling row and a processed row OUTSIDE the call do not change the launches of a greedy call with the switch on
    on = fresh(dec, cfg, POS, 600)
    assert on.verify_settings() is True
    on.set_verify_settings(False)
    assert on.verify_settings() is False
    on.set_verify_settings(True)
    warm = fresh(dec, cfg, POS, 600, on=False)
    warm.verify_rows(prompts, POS)
    warm.release()
    results, logs = [], []
    for b in (off, on):
        dec.launch_log(True)
        results.append(b.verify_rows(prompts, POS))
        logs.append(dec.launched())
    assert logs[0] == logs[1], (logs[0], logs[1])
    assert not [n for n in logs[1] if n.startswith("mc_vs_")]
    for a, b_, name in zip(results[0][:2], results[1][:2], ("accepted", "next tokens")):
        parity.exact(b_, a, f"switch on, greedy rows: {name}")
    parity.exact(on.logits(), off.logits(), "switch on, greedy rows: logits")
    for r in range(8):
        parity.exact(results[1][2][r], results[0][2][r], f"row {r}: picks")
        parity.exact(on.verify_logits()[r], off.verify_logits()[r], f"row {r}: logits of every chunk row")
        for layer in range(L):
            for a, b_, name in zip(on.export_row_kv(r, layer), off.export_row_kv(r, layer), "KV"):
                parity.exact(a, b_, f"row {r} layer {layer} {name}")
    # ... and with a sampling row and a processed row outside the call
    on2 = fresh(dec, cfg, POS, 600)
    on2.set_row_sampler(0, DRAW_K, 40, 0.9, 0.95)
    on2.set_row_penalties(0, 1.3, 0.1, 0.1)
    some = [None] + prompts[1:]
    dec.launch_log(True)
    on2.verify_rows(some, POS)
    assert not [n for n in dec.launched() if n.startswith("mc_vs_")]
    # every other refusal keeps its text with the switch on
    refused(lambda: on.verify_rows([[1, 2]] + [None] * 7, [250] + [0] * 7), "mc_verify_rows: row 0: position 250 is past the row's length")
    refused(lambda: on.verify_rows([list(range(17))] + [None] * 7, [0] * 8), "mc_verify_rows: row 0: a chunk of 17 tokens is longer than MC_VERIFY_MAX_LEN (16)")
    for b in (off, on, on2):
        b.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("shape", ["small-int4", "qlora-wide-17"])
def test_a_mixed_batch(acc, small, shape):
    from test_qlora_batch_gpu import decoder_of, qlora_model

    cfg, wide = SMALL, shape != "small-int4"
    if wide:
        dec = decoder_of(acc, cfg, qlora_model(SMALL, 28))
        rows, settings = [0, 3, 5, 9, 12, 14, 15, 16], [(GREEDY, None, None)] * 17
        for i, r in enumerate(rows):
            settings[r] = MIXED[i]
    else:
        dec = small_decoder(acc, cfg, small)
        rows, settings = list(range(8)), list(MIXED)
    B, vocab = len(settings), cfg["vocab"]
    pairs = pairs_of(5)
    lens = [6, 16, 5, 9, 12, 3, 16, 7]
    n, first, pos = [0] * B, [None] * B, [0] * B
    for i, r in enumerate(rows):
        n[r], first[r], pos[r] = lens[i], int(np.random.default_rng(i).integers(0, vocab)), POS[i]
    make = lambda: fresh(dec, cfg, POS, 2000, settings, pairs, wide=wide, rows=rows)
    call = grow_drafts(make, first, pos, n, 3)
    # the unprocessed logits: the same call on a batch without settings, switch off
    plain = fresh(dec, cfg, POS, 2000, on=False, wide=wide, rows=rows) if not wide else fresh(dec, cfg, POS, 2000, [(GREEDY, None, None)] * B, on=False, wide=True, rows=rows)
    plain.verify_rows(call, pos)
    raw = plain.verify_logits()
    batch = make()
    counts_before = [batch.row_token_counts(r) for r in range(B)]
    dec.launch_log(True)
    result = batch.verify_rows(call, pos)
    names = dec.launched()
    head = "mc_vhead_i8_bfloat" if wide else "mc_v_head_i4_bfloat"
    cut = names.index(head)
    assert names[cut - 1:] == ["mc_b_rmsnorm_bfloat", head, NEW[0], NEW[1], NEW[2], "mc_v_accept", NEW[3]], names[cut - 1:]
    check_call(batch, settings, call, pos, pairs, result, raw, counts_before, shape)
    accepted = result[0]
    assert all(accepted[r] >= 3 or accepted[r] == n[r] - 1 for r in rows), (accepted, "the grown drafts are accepted")
    plain.release()
    # K / V do not depend on the settings: mc_extend_rows' rows for the same chunks over the verified length
    plain = fresh(dec, cfg, POS, 2000, [(GREEDY, None, None)] * B, on=False, wide=wide, rows=rows)
    plain.extend_rows(call, pos)
    for r in rows:
        m = int(batch.lengths()[r])
        for a, b_, name in zip(batch.export_row_kv(r, 0), plain.export_row_kv(r, 0), "KV"):
            assert a.shape[0] == m
            parity.exact(a, b_[:m], f"{shape} row {r} {name}")
    plain.release()
    batch.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 3, 4
# (narrow top-k: the oracle model's logits are nearly flat, and two bfloat16 steps reorder the candidates of a wide top-k at most positions -- the
# mixed-batch test above keeps top_k 40 / 50, where every pick is held to the device's own logits)
EQ = [((DRAW_K, 2, 1.5, 1.0), None, None), ((DRAW_K, 2, 1.0, 1.0), None, None), ((DEFAULT_K, 5, 1.5, 0.5), None, None), ((DRAW_K, 2, 0.7, 1.0), None, None),
      (GREEDY, None, None), ((DRAW_K, 2, 0.5, 0.9), None, None), ((DRAW_K, 2, 1.0, 1.0), None, (1.3, 0.25, 0.5)), ((DRAW_K, 3, 0.6, 1.0), None, None)]
EQ_N = 12


def shift(bits, steps):
    """bfloat16 bits moved by `steps` representable values (sign-magnitude order, clamped inside the finite range)"""
    b = np.asarray(bits, np.uint16).astype(np.int32)
    key = np.where(b & 0x8000, -(b & 0x7FFF), b) + steps
    key = np.clip(key, -0x7F7F, 0x7F7F)
    return np.where(key < 0, (-key) | 0x8000, key).astype(np.uint16)


def perturbations(bits, pick):
    n = bits.size
    one = np.zeros(n, np.int32)
    one[pick] = 4
    rng = np.random.default_rng(int(pick) + n)
    yield shift(bits, 2)
    yield shift(bits, -2)
    yield shift(bits, one - 2)
    yield shift(bits, 2 - one)
    for _ in range(6):
        yield shift(bits, rng.integers(-2, 3, n))


def stable(bits, pick_fn):
    """the oracle alone: the rule's pick from `bits` survives every perturbation of two bfloat16 steps"""
    base = pick_fn(bits)
    return all(pick_fn(p) == base for p in perturbations(bits, base))


def oracle_rows(cfg, weights, settings, pairs, first, tokens, seed):
    """per row: the oracle behind fresh()'s context, FED the tokens the device generated -- (stable[j], oracle pick[j], argmax[j]) per position"""
    B, vocab = len(settings), cfg["vocab"]
    out = []
    for r, (sampler, mask, pen) in enumerate(settings):
        om = mo.Model(cfg, weights)
        for layer in range(cfg["n_layers"]):
            om.set_kv(layer, *random_cache(cfg, POS[r], seed + 100 * r + layer))
        counts = np.bincount(history_of(r, vocab), minlength=vocab) if pen is not None else None
        fed, rows = [first[r]] + [int(t) for t in tokens[:-1, r]], []
        for j, tok in enumerate(fed):
            _, ol = om.step(tok, POS[r] + j)
            if pen is not None:
                counts[tok] += 1
                ol = lr.process(ol, counts, None, *pen)
            fn = lambda b, s=sampler, p=pairs[(j * B + r) % len(pairs)]: pick_rule(b, s, p)
            rows.append((stable(ol, fn), fn(ol), lr.first_max(ol)))
        om.close()
        out.append(rows)
    return out


@pytest.fixture(scope="module")
def decoded(acc, small):
    """the rows' own continuation: EQ_N tokens of generate_rows under the seed array, and the oracle's view of every position"""
    cfg = SMALL
    dec = small_decoder(acc, cfg, small)
    pairs = pairs_of(11, 16 * 8)
    first = [int(np.random.default_rng(r).integers(0, cfg["vocab"])) for r in range(8)]
    gen = fresh(dec, cfg, POS, 2000, EQ, pairs)
    tokens, made = gen.generate_rows(first, POS, EQ_N)
    assert list(made) == [EQ_N] * 8
    gen.release()
    view = oracle_rows(cfg, small, EQ, pairs, first, tokens, 2000)
    dec.release()
    n_stable = [sum(s for s, _, _ in rows) for rows in view]
    off_argmax = sum(1 for r, rows in enumerate(view) for j, (s, p, a) in enumerate(rows) if s and EQ[r][0][0] == DRAW_K and p != a and tokens[j, r] == p)
    print(f"stable positions per row {n_stable} of {EQ_N}; compared draw picks off the argmax: {off_argmax}")
    assert all(2 * k >= EQ_N for k in n_stable), n_stable
    assert off_argmax >= 8, off_argmax
    return pairs, first, tokens, view


def test_verify_equals_decoding_at_stable_positions(acc, small, decoded):
    cfg = SMALL
    pairs, first, tokens, view = decoded
    dec = small_decoder(acc, cfg, small)
    batch = fresh(dec, cfg, POS, 2000, EQ, pairs)
    counts_before = [batch.row_token_counts(r) for r in range(8)]
    call = [np.concatenate([[first[r]], tokens[:EQ_N - 1, r]]).astype(np.int32) for r in range(8)]
    result = batch.verify_rows(call, POS)
    accepted, nxt, picks = result
    check_call(batch, EQ, call, POS, pairs, result, None, counts_before, "equivalence")
    compared = 0
    for r in range(8):
        for j, (ok, opick, _) in enumerate(view[r]):
            if ok:
                assert tokens[j, r] == opick, (r, j, "the step path left the oracle's pick at a stable position", tokens[j, r], opick)
                assert picks[r][j] == tokens[j, r], (r, j, EQ[r], picks[r][j], tokens[j, r])
                compared += 1
        run = next((j for j, (ok, _, _) in enumerate(view[r]) if not ok), EQ_N)
        assert accepted[r] >= min(run, EQ_N - 1), (r, accepted[r], run)
        if run == EQ_N:
            assert accepted[r] == EQ_N - 1 and nxt[r] == tokens[EQ_N - 1, r], (r, accepted[r], nxt[r])
    print(f"compared {compared} of {8 * EQ_N} positions")
    batch.release()
    dec.release()


@pytest.mark.parametrize("kind", ["first", "middle", "last"])
def test_a_planted_wrong_draft_is_where_acceptance_stops(acc, small, decoded, kind):
    cfg = SMALL
    pairs, first, tokens, view = decoded
    dec = small_decoder(acc, cfg, small)
    batch = fresh(dec, cfg, POS, 2000, EQ, pairs)
    plain = fresh(dec, cfg, POS, 2000, on=False)
    call, plant = [], []
    for r in range(8):
        run = next((j for j, (ok, _, _) in enumerate(view[r]) if not ok), EQ_N)
        j = min({"first": 0, "middle": (EQ_N - 1) // 2, "last": EQ_N - 2}[kind], run)   # drafts 0 .. j - 1 are accepted for certain
        c = np.concatenate([[first[r]], tokens[:EQ_N - 1, r]]).astype(np.int32)
        call.append(c)
        plant.append(j)
    # the wrong token: the id of the device's own LOWEST logit after chunk row j (a greedy call over the same chunk shows it) -- never among
    # the top-k candidates of any row, and the penalties only lower counted logits
    plain.verify_rows(call, POS)
    low = [int(np.argmin(mo.from_bf16(plain.verify_logits()[r][plant[r]]))) for r in range(8)]
    for r in range(8):
        assert call[r][plant[r] + 1] != low[r]
        call[r][plant[r] + 1] = low[r]
    accepted, nxt, picks = batch.verify_rows(call, POS)
    for r in range(8):
        assert accepted[r] == plant[r], (kind, r, accepted[r], plant[r])
        assert nxt[r] == picks[r][plant[r]], (kind, r)
        assert batch.lengths()[r] == POS[r] + plant[r] + 1
    print(f"plant {kind}: accepted {list(accepted)}")
    plain.release()
    batch.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 5
def test_a_chain_tree_is_the_chain_and_a_tree_counts_its_path(acc, small):
    cfg = SMALL
    dec = small_decoder(acc, cfg, small)
    settings = [((DRAW_K, 20, 1.0, 1.0), None, (1.3, 0.25, 0.5)), (GREEDY, None, None), ((DRAW_K, 50, 0.8, 0.9), "mask", (1.2, 0.0, 0.3)), (GREEDY, None, None)]
    pairs = pairs_of(21)
    pos, n, first = POS[:4], [12, 0, 7, 0], [100, None, 1500, None]
    make = lambda: fresh(dec, cfg, pos, 3000, settings, pairs)
    call = grow_drafts(make, first, pos, n, 4)
    chain, tree = make(), make()
    counts_before = [chain.row_token_counts(r) for r in range(4)]
    ra = chain.verify_rows(call, pos)
    dec.launch_log(True)
    rb = tree.verify_tree(call, [tr.chain(len(c)) if c is not None else None for c in call], pos)
    names = dec.launched()
    assert names[names.index("mc_v_head_i4_bfloat"):] == ["mc_v_head_i4_bfloat", NEW[0], NEW[1], NEW[2], "mc_tv_accept", NEW[3], "mc_tv_compact_bfloat"], names
    check_call(chain, settings, call, pos, pairs, ra, None, counts_before, "chain")
    parity.exact(rb[0], ra[0], "a chain tree: accepted")
    parity.exact(rb[1], ra[1], "a chain tree: next tokens")
    assert ra[0][0] >= 4 and ra[0][2] >= 4
    parity.exact(tree.logits(), chain.logits(), "a chain tree: logits")
    for r in (0, 2):
        parity.exact(rb[2][r], ra[2][r], f"a chain tree row {r}: picks")
        parity.exact(tree.verify_logits()[r], chain.verify_logits()[r], f"a chain tree row {r}: logits of every node")
        parity.exact(tree.row_token_counts(r), chain.row_token_counts(r), f"a chain tree row {r}: counts")
        for a, b_, name in zip(tree.export_row_kv(r, 0), chain.export_row_kv(r, 0), "KV"):
            parity.exact(a, b_, f"a chain tree row {r} {name}")
    chain.release()
    tree.release()
    # a real tree on row 0: two branches under the root, the SECOND carries the row's own picks (grown from the chain's call), the first random
    # tokens; siblings share a pair (their depth's), the walk follows the second branch and only ITS tokens are counted
    c0 = call[0]
    tokens = np.array([c0[0], 7, c0[1], 8, c0[2], 9, c0[3], c0[4]], np.int32)
    parents = [-1, 0, 0, 1, 2, 3, 4, 6]
    t = make()
    before = [t.row_token_counts(r) for r in range(4)]
    accepted, nxt, picks, paths = t.verify_tree([tokens, None, None, None], [parents, None, None, None], pos)
    check_call(t, settings, [tokens, None, None, None], pos, pairs, (accepted, nxt, picks), None, before, "tree", parents={0: parents}, paths=paths)
    assert list(paths[0][:5]) == [0, 2, 4, 6, 7] and accepted[0] >= 4, (paths[0], accepted[0])
    # node 2 sits at depth 1: it draws with chunk row 1's pair and sees the root's and its own token counted -- the chain's chunk row 1
    assert picks[0][2] == ra[2][0][1] and picks[0][4] == ra[2][0][2]
    t.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 6
def test_placement_and_company(acc, small):
    """the row under test -- a draw row with a mask, penalties and a history -- at row 5 of 8 in a full call, at row 0 of 3 with one other row, and
    alone in a batch of 1: every call stays at most 64 packed rows (one side of the prompt GEMM's line, test_verify_rows_gpu.py).  Its pairs are
    placed where (j * B + r) % n_pairs finds them in each batch"""
    import metalchat_amd as mc

    cfg, vocab = SMALL, SMALL["vocab"]
    dec = small_decoder(acc, cfg, small)
    mine = ((DRAW_K, 50, 0.8, 0.9), "mask", (1.3, 0.25, 0.5))
    own = pairs_of(31, 16)
    chunk0 = None
    ref = None
    for B, r, company in ((8, 5, {0: 6, 1: 2, 2: 3, 3: 9, 4: 5, 6: 4, 7: 7}), (3, 0, {2: 11}), (1, 0, {}), (8, 2, {7: 16})):
        rng = np.random.default_rng(B * 10 + r)
        pairs = [(int(a), int(b)) for a, b in rng.integers(0, 2 ** 63, (16 * B, 2))]
        for j in range(16):
            pairs[j * B + r] = own[j]
        b = mc.Batch(dec, B)
        b.set_verify_settings(True)
        b.set_seeds(pairs)
        call, pos = [None] * B, [0] * B
        for q in range(B):
            p = 40 if q == r else POS[q]
            b.import_kv(q, 0, *random_cache(cfg, p, 4000 if q == r else 4100 + q))
            pos[q] = p
            if q != r and q in company:
                b.set_row_sampler(q, *[(DRAW_K, 128, 1.0, 1.0), GREEDY, (DEFAULT_K, 7, 0.7, 0.9)][q % 3])
                call[q] = rng.integers(0, vocab, company[q]).astype(np.int32)
        b.set_row_sampler(r, *mine[0])
        b.set_row_mask(r, allowed_of(0, vocab))
        b.set_row_penalties(r, *mine[2])
        b.count_row_tokens(r, history_of(0, vocab))
        if chunk0 is None:
            def make(B=B, r=r, pairs=pairs):
                m = mc.Batch(dec, B)
                m.set_verify_settings(True)
                m.set_seeds(pairs)
                m.import_kv(r, 0, *random_cache(cfg, 40, 4000))
                m.set_row_sampler(r, *mine[0])
                m.set_row_mask(r, allowed_of(0, vocab))
                m.set_row_penalties(r, *mine[2])
                m.count_row_tokens(r, history_of(0, vocab))
                return m
            first = [None] * B
            first[r] = 321
            n = [0] * B
            n[r] = 10
            chunk0 = grow_drafts(make, first, [40 if q == r else 0 for q in range(B)], n, 4)[r]
        call[r] = chunk0
        assert sum(len(c) for c in call if c is not None) <= 64
        accepted, nxt, picks = b.verify_rows(call, pos)
        got = dict(accepted=int(accepted[r]), next=int(nxt[r]), picks=picks[r], verify_logits=b.verify_logits()[r].copy(), logits=b.logits()[r].copy(),
                   counts=b.row_token_counts(r))
        got["K"], got["V"] = b.export_row_kv(r, 0)
        what = f"B {B} row {r} company {company}"
        if ref is None:
            ref = got, what
            assert got["accepted"] >= 4
        else:
            assert (got["accepted"], got["next"]) == (ref[0]["accepted"], ref[0]["next"]), (what, ref[1])
            for name in got:
                parity.exact(got[name], ref[0][name], f"{what} against {ref[1]}: {name}")
        b.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 7
def test_a_loop_of_four_rounds_with_fresh_pairs(acc, small):
    """every round: fresh pairs, the drafts are what a clone of the rows -- the same caches, counts and pairs -- generates by ragged steps (a draft
    model that is the target: most drafts are accepted), then the call; the next round starts at the new lengths with the next tokens"""
    import metalchat_amd as mc

    cfg, vocab = SMALL, SMALL["vocab"]
    dec = small_decoder(acc, cfg, small)
    settings = MIXED[:4] + [MIXED[6]]
    B = len(settings)
    batch = fresh(dec, cfg, POS[:B], 5000, settings)
    pos = np.array(POS[:B], np.int32)
    toks = np.array([11, 222, 333, 1444, 1555], np.int32)
    total = 0
    for rnd in range(4):
        pairs = pairs_of(100 + rnd, 16 * B)
        batch.set_seeds(pairs)
        clone = mc.Batch(dec, B)
        apply_settings(clone, [(s, m, None) for s, m, _ in settings], vocab)
        for r in range(B):
            clone.import_kv(r, 0, *batch.export_row_kv(r, 0))
            if settings[r][2] is not None:
                clone.set_row_penalties(r, *settings[r][2])
                c = batch.row_token_counts(r)
                clone.count_row_tokens(r, np.repeat(np.arange(vocab), c))
        clone.set_seeds(pairs)
        n = [5, 8, 3, 6, 7]
        drafts, _ = clone.generate_rows(toks, pos, max(n))
        clone.release()
        call = [np.concatenate([[toks[r]], drafts[:n[r] - 1, r]]).astype(np.int32) for r in range(B)]
        counts_before = [batch.row_token_counts(r) for r in range(B)]
        result = batch.verify_rows(call, pos)
        check_call(batch, settings, call, pos, pairs, result, None, counts_before, f"round {rnd}")
        accepted, nxt, _ = result
        total += int(accepted.sum())
        pos = pos + accepted + 1
        toks = nxt.copy()
        assert list(batch.lengths()) == list(pos)
    print(f"four rounds: {total} drafts accepted")
    assert total >= 20, total   # (96 drafts offered; the step path and the chunk pass disagree only at unstable positions)
    batch.release()
    dec.release()
