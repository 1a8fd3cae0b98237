"""Speculative verify (mc_verify_rows, include/metalchat_hip.h Part 2f) on the device.

  * the layer pass is mc_extend_rows', bit for bit: K / V over the verify row's length, the last chunk row's logits and pick;
  * every chunk row against a chain of oracle.Model.step (tol(BF16), max_ulp 2: test_rows_extend_gpu.check_rows' bounds), each pick
    the argmax of the device's own logits row, and the oracle's pick where clear_gap calls that unambiguous;
  * acceptance: drafts are the oracle's own greedy continuation with ONE wrong token planted (the id of the oracle's lowest logit at
    that step), each chunk placed -- by looking at the oracle alone -- where the oracle's picks up to the plant are unambiguous, so
    that accepted[r] is known exactly in advance;
  * a row goes on after a rejection exactly like a fresh row that imported the accepted prefix; four rounds in a loop; the launch
    log; placement and company; the refusals, with nothing launched.

The greedy chains: row r starts behind random_cache(cfg, POS[r], 2000 + 100 r + layer) with the token default_rng(r).integers(0, 2048).
With the oracle alone (no device), SMALL int4 g128 seed 11, 24 steps per row: 161 of 192 positions are unambiguous, the longest
unambiguous run is 4 in row 5 and 8 to 18 in the other rows -- a plant at draft index j <= 3 fits every row."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import modelgen as mg
import parity
import verify_rule as vr
from oracle import mc_oracle as mo
from test_batch_gpu import LLAMA32_1B, SMALL, small_decoder
from test_context_gpu import random_cache
from test_prefill_gpu import tol
from test_rows_extend_gpu import check_log, release
from test_rows_prefill_gpu import clear_gap, gemm_launches, prompts_of, setup_rows

pytestmark = pytest.mark.gpu
BF16 = 0
POS = [5, 7, 16, 40, 63, 3, 64, 20]
SEED = 2000


@pytest.fixture(scope="module")
def small():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


@pytest.fixture(scope="module")
def llama1b():
    return mg.make_model(LLAMA32_1B, seed=5)


def argmax(logits_T):
    return int(np.argmax(mo.from_bf16(logits_T)))


def greedy_chain(om, first, p, n):
    """n greedy steps of the oracle from token `first` at position p: g[i] is fed at p + i, g[i + 1] is the pick after it"""
    ch = SimpleNamespace(p=p, g=[int(first)], logits=[], clear=[], low=[])
    for i in range(n):
        otok, ol = om.step(ch.g[i], p + i)
        ch.g.append(int(otok))
        ch.logits.append(ol)
        ch.clear.append(bool(clear_gap(ol)))
        ch.low.append(int(np.argmin(mo.from_bf16(ol))))
    return ch


def chains_of(cfg, weights, positions, n, seed=SEED):
    """per row: an oracle behind setup_rows' random context (the same seeds) and its greedy chain of n steps"""
    oms, chains = [], []
    for r, p in enumerate(positions):
        om = mo.Model(cfg, weights)
        for layer in range(cfg["n_layers"]):
            om.set_kv(layer, *random_cache(cfg, p, seed + 100 * r + layer))
        oms.append(om)
        chains.append(greedy_chain(om, np.random.default_rng(r).integers(0, 2048), p, n))
    return oms, chains


def run_from(clear, s):
    n = 0
    while s + n < len(clear) and clear[s + n]:
        n += 1
    return n


def place(ch, n, kind):
    """(s, n, j): a chunk g[s .. s + n) of the chain whose plant sits at draft index j (None: no plant), the oracle's picks at chunk
    rows 0 .. j unambiguous.  n shrinks until such a place exists; decided from the oracle's logits alone"""
    N = len(ch.clear)
    while n >= 2:
        j = {"first": 0, "middle": (n - 1) // 2, "last": n - 2, "none": None}[kind]
        need = n if j is None else j + 1
        for s in range(0, N - n + 1):
            if run_from(ch.clear, s) >= need:
                return s, n, j
        n -= 1
    raise AssertionError("no unambiguous position in the chain")


def chunk_of(ch, s, n, j):
    c = np.array(ch.g[s:s + n], np.int32)
    if j is not None:
        c[j + 1] = ch.low[s + j]   # the oracle's LOWEST logit after chunk row j: never the device's pick
        assert c[j + 1] != ch.g[s + j + 1]
    return c


def import_prefix(batch, r, om, cfg, n):
    """row r's cache = the oracle's first n cache rows of every layer"""
    for layer in range(cfg["n_layers"]):
        k, v = om.kv(layer)
        batch.import_kv(r, layer, k[:n], v[:n])


def check_verify_row(batch, r, ch, s, n, j, acc, nxt, picks, vlogits, logits, what, rel, max_ulp, frac):
    """test 3's assertions for one row whose chunk is chunk_of(ch, s, n, j) at position ch.p + s"""
    c = chunk_of(ch, s, n, j)
    assert len(picks[r]) == n and vlogits[r].shape[0] == n, what
    for i in range(n):
        assert picks[r][i] == argmax(vlogits[r][i]), (what, i)
    assert (acc[r], nxt[r]) == vr.accept(c, picks[r]), (what, acc[r], nxt[r], list(picks[r]), list(c))
    last = n - 1 if j is None else j
    for i in range(last + 1):
        st = parity.check(BF16, vlogits[r][i], ch.logits[s + i], rel=rel, max_ulp=max_ulp, max_frac=frac, what=f"{what} chunk row {i} logits")
        if ch.clear[s + i]:
            assert picks[r][i] == ch.g[s + i + 1], (what, i, picks[r][i], ch.g[s + i + 1])
    if j is not None:
        assert acc[r] == j, (what, acc[r], j)
        assert nxt[r] == ch.g[s + j + 1], (what, nxt[r], ch.g[s + j + 1])
    elif all(ch.clear[s:s + n]):
        assert acc[r] == n - 1 and nxt[r] == ch.g[s + n], (what, acc[r], nxt[r])
    assert batch.lengths()[r] == ch.p + s + acc[r] + 1, what
    parity.exact(logits[r], vlogits[r][acc[r]], f"{what}: the batch's logits are chunk row {acc[r]}'s")


# ------------------------------------------------------------------------------------------ 1
def test_the_pass_is_extend_rows_pass(acc, small):
    import metalchat_amd as mc

    cfg, L = SMALL, SMALL["n_layers"]
    dec = small_decoder(acc, cfg, small)
    pos = [5, 7, 16, 40, 63, 240, 64, 20]           # 63: ends inside a 64-slot range; 240 + 16: the last cache slot
    lens = [2, 3, 5, 8, 11, 16, 13, 16]
    prompts = prompts_of(cfg, lens, 21)
    ext, oa = setup_rows(dec, cfg, small, pos, SEED)
    ver, ob = setup_rows(dec, cfg, small, pos, SEED)
    epicks = ext.extend_rows(prompts, pos)
    accepted, nxt, picks = ver.verify_rows(prompts, pos)
    el, vl = ext.logits(), ver.verify_logits()
    for r in range(8):
        assert ver.lengths()[r] == pos[r] + accepted[r] + 1 <= ext.lengths()[r] == pos[r] + lens[r]
        parity.exact(vl[r][-1], el[r], f"row {r}: the last chunk row's logits against extend_rows")
        assert picks[r][-1] == epicks[r], (r, picks[r][-1], epicks[r])
        n = int(ver.lengths()[r])
        for layer in range(L):
            for a, b, name in zip(ver.export_row_kv(r, layer), ext.export_row_kv(r, layer), "KV"):
                assert a.shape[0] == n
                parity.exact(a, b[:n], f"row {r} layer {layer} {name} over the verify row's length")
    for om in ob:
        om.close()
    ver.release()
    release(ext, oa, dec)


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("shape", ["small-int4", "llama32-1b-bf16"])
def test_every_chunk_row_against_the_oracle(acc, small, llama1b, shape):
    import metalchat_amd as mc

    cfg, weights = (SMALL, small) if shape == "small-int4" else (LLAMA32_1B, llama1b)
    pos = POS if cfg is SMALL else [9, 7, 64, 20]
    lens = [16, 2, 9, 16, 13, 5, 16, 3][:len(pos)]
    rel, frac = tol(BF16)
    dec = small_decoder(acc, cfg, weights)
    oms, chains = chains_of(cfg, weights, pos, 16)
    batch = mc.Batch(dec, len(pos))
    for r, p in enumerate(pos):
        import_prefix(batch, r, oms[r], cfg, p)
    chunks = [np.array(ch.g[:n], np.int32) for ch, n in zip(chains, lens)]
    accepted, nxt, picks = batch.verify_rows(chunks, pos)
    vl = batch.verify_logits()
    compared = unambiguous = 0
    for r, (ch, n) in enumerate(zip(chains, lens)):
        for i in range(n):
            st = parity.check(BF16, vl[r][i], ch.logits[i], rel=rel, max_ulp=2, max_frac=frac, what=f"{shape} row {r} chunk row {i} logits")
            assert picks[r][i] == argmax(vl[r][i]), (shape, r, i)
            compared += 1
            if ch.clear[i]:
                unambiguous += 1
                assert picks[r][i] == ch.g[i + 1], (shape, r, i, picks[r][i], ch.g[i + 1])
        print(f"{shape} row {r} (pos {pos[r]}, len {n}): last row {st}, accepted {accepted[r]}")
        for layer in sorted({0, cfg["n_layers"] - 1}):
            gk, gv = batch.export_row_kv(r, layer)
            ok, ov = oms[r].kv(layer)
            m = pos[r] + accepted[r] + 1
            assert gk.shape[0] == m
            parity.exact(gk[:pos[r]], ok[:pos[r]], f"{shape} row {r} layer {layer} context K")
            parity.check(BF16, gk[pos[r]:], ok[pos[r]:m], rel=rel, max_ulp=2, max_frac=frac, what=f"{shape} row {r} layer {layer} K")
            parity.check(BF16, gv[pos[r]:], ov[pos[r]:m], rel=rel, max_ulp=2, max_frac=frac, what=f"{shape} row {r} layer {layer} V")
    print(f"{shape}: {unambiguous} of {compared} positions unambiguous")
    assert 2 * unambiguous >= compared, (unambiguous, compared)
    release(batch, oms, dec)


# ------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("kind", ["first", "middle", "last", "none"])
def test_acceptance(acc, small, kind):
    import metalchat_amd as mc

    cfg, L = SMALL, SMALL["n_layers"]
    rel, frac = tol(BF16)
    dec = small_decoder(acc, cfg, small)
    oms, chains = chains_of(cfg, small, POS, 24)
    out = {"first": 7, "middle": 2, "last": 5, "none": 0}[kind]    # the row that is not in the call
    want_n = [4, 6, 9, 16, 12, 5, 8, 7]
    batch = mc.Batch(dec, 8)
    plan, call, pos = {}, [None] * 8, [0] * 8
    for r, ch in enumerate(chains):
        s, n, j = place(ch, want_n[r], kind)
        import_prefix(batch, r, oms[r], cfg, ch.p + s)
        if r != out:
            plan[r], call[r], pos[r] = (s, n, j), chunk_of(ch, s, n, j), ch.p + s
    print(f"plant {kind}: (start, length, plant) per row {plan}")
    before = [batch.export_row_kv(out, layer) for layer in range(L)]
    len_before, logits_before = batch.lengths()[out], batch.logits()[out].copy()
    accepted, nxt, picks = batch.verify_rows(call, pos)
    vl, logits = batch.verify_logits(), batch.logits()
    for r, (s, n, j) in plan.items():
        check_verify_row(batch, r, chains[r], s, n, j, accepted, nxt, picks, vl, logits, f"plant {kind} row {r}", rel, 2, frac)
    exp_acc, exp_next = vr.accept_rows(call, picks)
    parity.exact(accepted, exp_acc, "accepted against the rule")
    parity.exact(nxt, exp_next, "next tokens against the rule")
    assert accepted[out] == -1 and nxt[out] == -1 and picks[out] is None and vl[out] is None
    assert batch.lengths()[out] == len_before
    parity.exact(logits[out], logits_before, f"row {out} (not in the call): logits")
    for layer, (k, v) in enumerate(before):
        gk, gv = batch.export_row_kv(out, layer)
        parity.exact(gk, k, f"row {out} (not in the call) layer {layer} K")
        parity.exact(gv, v, f"row {out} (not in the call) layer {layer} V")
    release(batch, oms, dec)


# ------------------------------------------------------------------------------------------ 4
def test_a_row_goes_on_after_a_rejection(acc, small):
    import metalchat_amd as mc

    cfg, L = SMALL, SMALL["n_layers"]
    dec = small_decoder(acc, cfg, small)
    pos = [30, 5, 64, 17]
    batch, oms = setup_rows(dec, cfg, small, pos, 900)
    drafts = prompts_of(cfg, [16, 9, 2, 12], 31)      # random ids: rejected, and their slots hold real K / V rows
    accepted, nxt, _ = batch.verify_rows(drafts, pos)
    at = np.array(pos) + accepted + 1
    assert list(batch.lengths()) == list(at)
    assert all(accepted[r] < len(drafts[r]) - 1 for r in (0, 1, 3)), accepted   # (2047 in 2048 per draft)
    fresh = mc.Batch(dec, 4)
    for r in range(4):
        for layer in range(L):
            k, v = batch.export_row_kv(r, layer)
            assert k.shape[0] == at[r]
            fresh.import_kv(r, layer, k, v)
    toks = nxt.copy()

    def same(what):
        parity.exact(batch.logits(), fresh.logits(), f"{what}: logits")
        assert list(batch.lengths()) == list(fresh.lengths()), what
        for r in range(4):
            for layer in range(L):
                for a, b, name in zip(batch.export_row_kv(r, layer), fresh.export_row_kv(r, layer), "KV"):
                    parity.exact(a, b, f"{what}: row {r} layer {layer} {name}")

    a, b = batch.step_rows(toks, at), fresh.step_rows(toks, at)
    parity.exact(a, b, "step_rows: picks")
    same("step_rows")
    at = at + 1
    (ta, la), (tb, lb) = batch.generate_rows(a, at, 2), fresh.generate_rows(a, at, 2)
    parity.exact(ta, tb, "generate_rows: tokens")
    parity.exact(la, lb, "generate_rows: produced")
    same("generate_rows")
    at = at + 2
    more = prompts_of(cfg, [5, 17, 2, 33], 32)
    parity.exact(batch.extend_rows(more, at), fresh.extend_rows(more, at), "extend_rows: picks")
    same("extend_rows")
    at = at + np.array([5, 17, 2, 33])
    again = prompts_of(cfg, [7, 16, 3, 2], 33)
    ra, rb = batch.verify_rows(again, at), fresh.verify_rows(again, at)
    parity.exact(ra[0], rb[0], "second verify_rows: accepted")
    parity.exact(ra[1], rb[1], "second verify_rows: next tokens")
    for r, (x, y, u, w) in enumerate(zip(ra[2], rb[2], batch.verify_logits(), fresh.verify_logits())):
        parity.exact(x, y, f"second verify_rows: row {r} picks")
        parity.exact(u, w, f"second verify_rows: row {r} logits of every chunk row")
    same("second verify_rows")
    fresh.release()
    release(batch, oms, dec)


# ------------------------------------------------------------------------------------------ 5
def test_a_loop_of_four_rounds(acc, small):
    """every round continues at positions[r] + accepted[r] + 1 with the oracle's token there, behind a cache the device wrote: the
    project's bounds for that (max_ulp 2 + n_layers, rel 5e-3, test_rows_extend_gpu.test_steps_and_chunks_continue_and_a_rewind)"""
    import metalchat_amd as mc

    cfg, L = SMALL, SMALL["n_layers"]
    dec = small_decoder(acc, cfg, small)
    oms, chains = chains_of(cfg, small, POS, 80)
    batch = mc.Batch(dec, 8)
    for r, ch in enumerate(chains):
        import_prefix(batch, r, oms[r], cfg, ch.p)
    start = [0] * 8
    for rnd in range(4):
        call, pos, plan = [None] * 8, [0] * 8, {}
        for r, ch in enumerate(chains):
            s, run = start[r], run_from(ch.clear, start[r])
            want = (r + 2 * rnd) % 5                  # a different plant per row and round; 4: none
            if want == 4 and run >= 2:
                n, j = min(run, 6), None
            else:
                j = min(want % 4, max(run - 1, 0))    # (an ambiguous first row: the plant at draft 0 is still rejected for certain)
                # prefer a plant behind which the next round starts on an unambiguous position (the oracle alone decides)
                j = next((k for k in range(j, -1, -1) if ch.clear[s + k + 1]), j)
                n = min(16, j + 2 + r % 3)
            plan[r], call[r], pos[r] = (s, n, j), chunk_of(ch, s, n, j), ch.p + s
        print(f"round {rnd}: (start, length, plant) per row {plan}")
        accepted, nxt, picks = batch.verify_rows(call, pos)
        vl, logits = batch.verify_logits(), batch.logits()
        for r, (s, n, j) in plan.items():
            ch, what = chains[r], f"round {rnd} row {r}"
            if j is not None and not ch.clear[s + j]:
                # the oracle's pick at the plant's row is ambiguous: the rejection is certain, the next token is the device's own
                c = chunk_of(ch, s, n, j)
                assert (accepted[r], nxt[r]) == vr.accept(c, picks[r]) and accepted[r] <= j, (what, accepted[r], j)
                assert batch.lengths()[r] == ch.p + s + accepted[r] + 1
                parity.exact(logits[r], vl[r][accepted[r]], f"{what}: the batch's logits")
            else:
                check_verify_row(batch, r, ch, s, n, j, accepted, nxt, picks, vl, logits, what, 5e-3, 2 + L, 0.7)
            start[r] = s + int(accepted[r]) + 1       # the oracle's token g[start] goes in at the row's new length
        parity.exact(accepted, vr.accept_rows(call, picks)[0], f"round {rnd}: accepted against the rule")
    release(batch, oms, dec)


# ------------------------------------------------------------------------------------------ 6
def test_the_launch_log(acc, small):
    import metalchat_amd as mc

    cfg = SMALL
    dec = small_decoder(acc, cfg, small)
    lens = [2, 16, 5, 16, 9, 3, 16, 12]
    prompts = prompts_of(cfg, lens, 41)
    ver, oa = setup_rows(dec, cfg, small, POS, 600)
    ext, ob = setup_rows(dec, cfg, small, POS, 600)
    warm = mc.Batch(dec, 8)
    warm.extend_rows(prompts, [0] * 8)   # (whatever the decoder's first prompt pass prepares once is done before the logs)
    warm.release()
    dec.launch_log(True)
    ver.verify_rows(prompts, POS)
    verify = dec.launched()
    dec.launch_log(True)
    ext.extend_rows(prompts, POS)
    extend = dec.launched()
    assert [n for n in verify if n.startswith("mc_v_")] == ["mc_v_head_i4_bfloat", "mc_v_argmax_bfloat", "mc_v_accept"], verify
    assert not [n for n in verify if n.startswith("mc_b_gemv_")], verify
    assert gemm_launches(verify) == gemm_launches(extend), (verify, extend)
    # the layer pass is the same list of launches: the two calls differ behind the gather only
    cut = verify.index("mc_pp_gather_last_bfloat")
    assert verify[:cut + 1] == extend[:cut + 1], (verify, extend)
    assert verify[cut + 1:] == ["mc_b_rmsnorm_bfloat", "mc_v_head_i4_bfloat", "mc_v_argmax_bfloat", "mc_v_accept"], verify
    check_log(extend, cfg["head_dim"])
    # an extend_rows call on the batch that verified: no mc_v_* launch
    dec.launch_log(True)
    ver.extend_rows([p[:2] for p in prompts], ver.lengths())
    after = dec.launched()
    assert not [n for n in after if n.startswith("mc_v_")], after
    check_log(after, cfg["head_dim"])
    for om in ob:
        om.close()
    ext.release()
    release(ver, oa, dec)


# ------------------------------------------------------------------------------------------ 7
# (batch size, {batch row: chunk index}) of one call; the chunks' lengths are COMPANY_LENS, their contexts POS
COMPANY_LENS = [2, 16, 5, 16, 9, 3, 16, 12]
COMPANY_CALLS = [
    # more than 64 packed rows
    (8, {r: r for r in range(8)}),                                  # 79 rows
    (8, {5: 0, 2: 1, 7: 2, 0: 3, 3: 4, 6: 5, 1: 6, 4: 7}),          # 79: every chunk in another batch row
    (5, {0: 6, 1: 1, 2: 3, 3: 4, 4: 7}),                            # 69: a smaller batch, other company
    (8, {1: 3, 2: 6, 4: 1, 6: 7, 7: 4, 0: 5}),                      # 72: two rows of the batch not in the call
    # at most 64 packed rows
    (3, {0: 6, 1: 1, 2: 4}),                                        # 41
    (3, {2: 4}),                                                    # 9: alone in the call
    (8, {5: 6}),                                                    # 16: alone in a batch of 8
    (2, {0: 4, 1: 6}),                                              # 25
    (4, {3: 1, 0: 7, 1: 6}),                                        # 44
]


@pytest.mark.parametrize("shape", ["small-int4", "llama32-1b-bf16"])
def test_placement_and_company(acc, small, llama1b, shape):
    """A chunk's picks, accepted, next token, logits of every chunk row and K / V do not depend on its batch row, on B or on which
    other rows are in the call -- "as in Part 2e", whose pass this is.  Part 2e's pass has ONE place where the call as a whole reaches
    a row's bits: with int4 g128 weights the decoder multiplies a prompt pass of at most 64 rows by its weight-streaming GEMM
    (mc_pf2_gemm_i4_*, prefill.cc pf2_ok) and a longer one by the tiled GEMM, which add the K ranges in another order.  Both sides of
    that line lie inside a verify call's 2 .. 128 rows, so with int4 weights the calls are compared among those on the same side
    (and the launch log must show that the sides are what this test takes them for); with plain bfloat16 weights there is no such
    line below 128 rows and every call is compared with every other."""
    import metalchat_amd as mc

    cfg, weights = (SMALL, small) if shape == "small-int4" else (LLAMA32_1B, llama1b)
    L, int4 = cfg["n_layers"], shape == "small-int4"
    dec = small_decoder(acc, cfg, weights)
    prompts = prompts_of(cfg, COMPANY_LENS, 51)
    ref = {}
    for B, rows in COMPANY_CALLS:
        M = sum(COMPANY_LENS[i] for i in rows.values())
        side = "short" if int4 and M <= 64 else "long"
        batch = mc.Batch(dec, B)
        call, pos = [None] * B, [0] * B
        for r, i in rows.items():
            call[r], pos[r] = prompts[i], POS[i]
            for layer in range(L):
                batch.import_kv(r, layer, *random_cache(cfg, POS[i], 700 + 100 * i + layer))
        dec.launch_log(True)
        accepted, nxt, picks = batch.verify_rows(call, pos)
        streamed = any(n.startswith("mc_pf2_gemm") for n in dec.launched())
        assert streamed == (side == "short"), (shape, B, rows, M, sorted(set(gemm_launches(dec.launched()))))
        vl, logits = batch.verify_logits(), batch.logits()
        for r in range(B):
            if r not in rows:
                assert accepted[r] == nxt[r] == -1 and picks[r] is None and vl[r] is None, (B, rows, r)
                continue
            i, what = rows[r], f"{shape} B {B} rows {rows} ({M} packed rows): chunk {rows[r]}"
            got = dict(accepted=int(accepted[r]), next=int(nxt[r]), picks=picks[r], verify_logits=vl[r].copy(), logits=logits[r].copy())
            for layer in range(L):
                got[f"K{layer}"], got[f"V{layer}"] = batch.export_row_kv(r, layer)
            if (side, i) not in ref:
                ref[side, i] = got, what
                continue
            exp, first = ref[side, i]
            assert (got["accepted"], got["next"]) == (exp["accepted"], exp["next"]), (what, first)
            for name in got:
                parity.exact(got[name], exp[name], f"{what} against {first}: {name}")
        batch.release()
    # every chunk was compared at least once on each side it occurs on
    assert {i for _, i in ref} == set(range(8))
    dec.release()


# ------------------------------------------------------------------------------------------ 8
def test_refusals(acc, small):
    import metalchat_amd as mc

    S = SMALL["max_seq_len"]
    dec = small_decoder(acc, SMALL, small)
    batch = mc.Batch(dec, 4)
    lib = mc.capi()
    ptr = C.POINTER(C.c_int32)
    dec.launch_log(True)
    assert lib.mc_verify_get_logits(batch._h, np.zeros(8, np.uint16).ctypes.data_as(C.c_void_p)) == 1
    assert lib.mc_last_error().decode().startswith("mc_verify_get_logits: no mc_verify_rows call"), lib.mc_last_error()
    assert dec.launched() == []
    batch.extend_rows([[1, 2, 3], None, None, None], [0, 0, 0, 0])  # row 0: length 3

    def call(tokens, lens, positions, words):
        t = np.ascontiguousarray(np.asarray(list(tokens) + [0], np.int32))
        ln = np.ascontiguousarray(lens, np.int32)
        p = np.ascontiguousarray(positions, np.int32)
        a, out, picks = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(len(t), np.int32)
        dec.launch_log(True)
        st = lib.mc_verify_rows(batch._h, t.ctypes.data_as(ptr), ln.ctypes.data_as(ptr), p.ctypes.data_as(ptr), a.ctypes.data_as(ptr),
                                out.ctypes.data_as(ptr), picks.ctypes.data_as(ptr))
        assert st == 1, words
        msg = lib.mc_last_error().decode()
        assert msg.startswith("mc_verify_rows: "), msg
        assert words in msg, (words, msg)
        assert dec.launched() == [], words
        assert list(batch.lengths()) == [3, 0, 0, 0], words

    # every case of test_rows_extend_gpu.test_refusals
    call([], [0, 0, 0, 0], [0, 0, 0, 0], "no row in the call")
    call([1, 2], [2, -1, 0, 0], [0, 0, 0, 0], "row 1: length below 0")
    call([1, 2, 3], [2, 1, 0, 0], [0, 0, 0, 0], "row 1: a one-token chunk is a step")
    call([1, 2], [0, 0, 2, 0], [0, 0, -1, 0], "row 2: position below 0")
    call([1, 2], [2, 0, 0, 0], [4, 0, 0, 0], "row 0: position 4 is past the row's length 3")
    call(list(range(S - 2)), [S - 2, 0, 0, 0], [3, 0, 0, 0], "row 0: position + length")
    call([1, SMALL["vocab"]], [0, 0, 0, 2], [0, 0, 0, 0], "row 3: token id outside the vocabulary")
    call([1, -5], [0, 0, 0, 2], [0, 0, 0, 0], "row 3: token id outside the vocabulary")
    call(list(range(S)) + [1, 2], [S - 100, 100, 2, 0], [0, 0, 0, 0], "add up to 258, more than max_seq_len")
    # a chunk of 17
    call(list(range(2 + 17)), [2, 0, 17, 0], [0, 0, 0, 0], "row 2: a chunk of 17 tokens is longer than MC_VERIFY_MAX_LEN (16)")
    # the default sampler set on the decoder
    dec.set_sampler(mc.SAMPLER_DEFAULT, top_k=40, temperature=0.6, top_p=0.9)
    call([1, 2], [2, 0, 0, 0], [0, 0, 0, 0], "greedy")
    dec.set_sampler(mc.SAMPLER_GREEDY)
    accepted, nxt, picks = batch.verify_rows([[1, 2, 3], None, None, None], [3, 0, 0, 0])
    assert accepted[0] >= 0 and batch.lengths()[0] == 3 + accepted[0] + 1
    batch.release()
    dec.release()
