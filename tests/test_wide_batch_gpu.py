"""Wide batches (mc_wide_batch_create, include/metalchat_hip.h Part 2h) on the device: up to 64 rows per step over one decoder's
weights, every call of Parts 2b - 2g on the handle at more than 8 rows.

  * rows against their own oracle.Model with run_lockstep's bounds;
  * a row of a wide batch is the same row of a mc_batch_create batch of 8, bit for bit: lockstep, ragged with stop ids and idle
    rows, the default sampler, the packed passes, verify over chains and trees -- the rows dealt over ceil(B / 8) narrow batches on
    the same decoder;
  * the launch changes at 16 rows and nowhere else; the new refusal of a verify call above MC_VERIFY_MAX_ROWS; mc_batch_create as it was.
"""
import numpy as np
import pytest

import modelgen as mg
import parity
import tree_rule as tr
from oracle import mc_oracle as mo
from test_batch_gpu import BF16, LLAMA32_1B, SMALL, refused, small_decoder
from test_context_gpu import random_cache

pytestmark = pytest.mark.gpu
NAN = 0x7FC0


@pytest.fixture(scope="module")
def small_i4():
    return mg.make_model(SMALL, seed=11, quant="i4", group=128)


@pytest.fixture(scope="module")
def small_w():
    return mg.make_model(SMALL, seed=12)


@pytest.fixture(scope="module")
def llama1b():
    return mg.make_model(LLAMA32_1B, seed=5)


def weights_of(fmt, small_i4, small_w):
    return small_i4 if fmt == "i4" else small_w


def deal(B):
    """the rows of a wide batch over ceil(B / 8) narrow batches: [(first row, rows)]"""
    return [(r0, min(8, B - r0)) for r0 in range(0, B, 8)]


def narrow_batches(dec, B):
    import metalchat_amd as mc

    return [(r0, n, mc.Batch(dec, n)) for r0, n in deal(B)]


def import_rows(batch, r0, caches, layers=1):
    """caches[r]: [(k, v) per layer] or None"""
    for i in range(batch.B):
        if caches[r0 + i] is not None:
            for layer in range(layers):
                batch.import_kv(i, layer, *caches[r0 + i][layer])


# ------------------------------------------------------------------------------------------ 1. against the oracle
ORACLE_ROWS = [0, 15, 16, 17, 31, 32, 39]


@pytest.mark.parametrize("shape", ["small-i4", "llama1b-w"])
def test_rows_against_the_oracle(acc, small_i4, llama1b, shape):
    """B = 40, every row its own random cache of 60 positions, 6 lockstep steps (across the 64-slot boundary); the rows at the
    ends of the column groups against their own oracle.Model with run_lockstep's bounds"""
    import metalchat_amd as mc

    cfg, weights = (SMALL, small_i4) if shape == "small-i4" else (LLAMA32_1B, llama1b)
    L, B, n_inject, n_steps = cfg["n_layers"], 40, 60, 6
    dec = small_decoder(acc, cfg, weights)
    batch = mc.Batch(dec, B, wide=True)
    assert batch.size() == B
    oms = {r: mo.Model(cfg, weights) for r in ORACLE_ROWS}
    for r in range(B):
        for layer in range(L):
            k, v = random_cache(cfg, n_inject, 1000 * r + layer)
            batch.import_kv(r, layer, k, v)
            if r in oms:
                oms[r].set_kv(layer, k, v)
    toks = np.array([7 + 13 * r for r in range(B)], np.int32)
    for i in range(n_steps):
        pos = n_inject + i
        picks = batch.step(toks, pos)
        logits = batch.logits()
        nxt = picks.copy()
        for r in range(B):
            assert picks[r] == int(np.argmax(mo.from_bf16(logits[r]))), (shape, r, pos)
        for r, om in oms.items():
            otok, ologits = om.step(int(toks[r]), pos)
            parity.check(BF16, logits[r], ologits, rel=5e-3, max_ulp=2 + L, max_frac=0.7, what=f"{shape} row {r} pos {pos} logits")
            nxt[r] = otok
        toks = nxt
    for r, om in oms.items():
        for layer in range(L):
            gk, gv = batch.export_kv(r, layer)
            ok, ov = om.kv(layer)
            assert gk.shape == ok.shape == (n_inject + n_steps, cfg["n_kv_heads"], cfg["head_dim"])
            parity.exact(gk[:n_inject], ok[:n_inject], f"{shape} row {r} layer {layer} injected K rows")
            parity.exact(gv[:n_inject], ov[:n_inject], f"{shape} row {r} layer {layer} injected V rows")
            parity.check(BF16, gk[n_inject:], ok[n_inject:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{shape} row {r} computed K")
            parity.check(BF16, gv[n_inject:], ov[n_inject:], rel=3.9e-3, max_ulp=2, max_frac=0.7, what=f"{shape} row {r} computed V")
        om.close()
    batch.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 2. a row is the narrow batch's row
def lockstep(batch, r0, contents, n_steps, pos0):
    """contents[r] = (token, [(k, v)]); returns per row of the batch (logits[n_steps], picks[n_steps], K, V)"""
    import_rows(batch, r0, [c[1] for c in contents])
    toks = np.array([contents[r0 + i][0] for i in range(batch.B)], np.int32)
    logits, picks = [], []
    for i in range(n_steps):
        toks = batch.step(toks, pos0 + i)
        logits.append(batch.logits())
        picks.append(toks.copy())
    out = []
    for i in range(batch.B):
        k, v = batch.export_kv(i, 0)
        out.append((np.stack([lg[i] for lg in logits]), np.array([p[i] for p in picks]), k, v))
    return out


@pytest.fixture(scope="module")
def narrow_lockstep_rows():
    """the 64 rows of test 2 in narrow batches of 8, computed once per format (a narrow batch's rows do not depend on its size:
    test_batch_gpu.test_rows_are_independent_bit_for_bit)"""
    return {}


@pytest.mark.parametrize("B", [9, 16, 17, 33, 64])
@pytest.mark.parametrize("fmt", ["i4", "w"])
def test_a_row_is_the_narrow_batchs_row(acc, small_i4, small_w, narrow_lockstep_rows, fmt, B):
    import metalchat_amd as mc

    weights = weights_of(fmt, small_i4, small_w)
    dec = small_decoder(acc, SMALL, weights)
    contents = [(3 + 29 * r, [random_cache(SMALL, 40, 500 + r)]) for r in range(64)]
    if fmt not in narrow_lockstep_rows:
        ref = []
        for r0, n in deal(64):
            nb = mc.Batch(dec, n)
            ref += lockstep(nb, r0, contents, 4, 40)
            nb.release()
        narrow_lockstep_rows[fmt] = ref
    ref = narrow_lockstep_rows[fmt]
    wide = mc.Batch(dec, B, wide=True)
    got = lockstep(wide, 0, contents, 4, 40)
    wide.release()
    if B % 8:  # the last narrow batch of the deal is a smaller one: its rows are the batch-of-8 rows as well
        r0, n = deal(B)[-1]
        nb = mc.Batch(dec, n)
        for i, row in enumerate(lockstep(nb, r0, contents, 4, 40)):
            for x, y, name in zip(row, ref[r0 + i], ("logits", "picks", "K", "V")):
                assert np.array_equal(x, y), f"{fmt}: narrow batch of {n}, row {r0 + i}: {name} differ"
        nb.release()
    for r in range(B):
        for x, y, name in zip(got[r], ref[r], ("logits", "picks", "K", "V")):
            assert np.array_equal(x, y), f"{fmt} B={B} row {r}: {name} differ from the narrow batch's"
    dec.release()


# ------------------------------------------------------------------------------------------ 3. the launch log
@pytest.mark.parametrize("fmt", ["i4", "w"])
def test_the_launch_log(acc, small_i4, small_w, fmt):
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, weights_of(fmt, small_i4, small_w))
    before = dec.derived_weight_bytes()
    tok0 = dec.step(9, 0)
    narrow = {f"mc_b_gemv_{fmt}_bfloat_e{e}" for e in (0, 1, 2)}
    wide = {f"mc_wb_gemv_{fmt}_bfloat_e{e}" for e in (0, 1, 2)}
    for B, want, never in ((12, narrow, "mc_wb_"), (16, narrow, "mc_wb_"), (17, wide, "mc_b_gemv_"), (40, wide, "mc_b_gemv_")):
        batch = mc.Batch(dec, B, wide=True)
        dec.launch_log(True)
        batch.step(np.arange(B, dtype=np.int32), 0)
        batch.generate_rows(np.arange(B, dtype=np.int32), np.ones(B, np.int32), 2)
        names = set(dec.launched())
        dec.launch_log(False)
        assert want <= names, (B, sorted(names))
        assert not [n for n in names if n.startswith(never) or n.startswith("mc_gemv_")], (B, sorted(names))
        batch.release()
    assert dec.derived_weight_bytes() == before
    assert dec.step(9, 0) == tok0
    dec.release()


# ------------------------------------------------------------------------------------------ 4. ragged
@pytest.mark.parametrize("fmt", ["i4", "w"])
def test_ragged_rows(acc, small_i4, small_w, fmt):
    import metalchat_amd as mc

    B, n, IDLE = 40, 6, (3, 11, 19, 27, 35)
    dec = small_decoder(acc, SMALL, weights_of(fmt, small_i4, small_w))
    pos = np.array([20 + (r * 180) // (B - 1) for r in range(B)], np.int32)      # 20 .. 200
    first = np.array([5 + 41 * r for r in range(B)], np.int32)
    caches = [[random_cache(SMALL, int(pos[r]), 900 + r)] for r in range(B)]
    pos[23], first[23], caches[23] = pos[7], first[7], caches[7]                 # two rows with one content: they stop together
    guard = np.full((50, SMALL["n_kv_heads"], SMALL["head_dim"]), NAN, np.uint16)
    for r in IDLE:
        pos[r], caches[r] = -1, [(guard, guard)]

    def run(stop):
        """(tokens[n][B], lengths[B], cache lengths[B], K / V per row) of the wide batch and of the narrow batches"""
        out = []
        for batches in ([(0, B, mc.Batch(dec, B, wide=True))], narrow_batches(dec, B)):
            toks, lens, clens, kv = np.zeros((n, B), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32), []
            for r0, m, b in batches:
                import_rows(b, r0, caches)
                toks[:, r0:r0 + m], lens[r0:r0 + m] = b.generate_rows(first[r0:r0 + m], pos[r0:r0 + m], n, stop)
                clens[r0:r0 + m] = b.lengths()
                kv += [b.export_row_kv(i, 0) for i in range(m)]
                b.release()
            out.append((toks, lens, clens, kv))
        return out

    (free, _, _, _), _ = run(())
    stop = int(free[2, 7])                                                        # what rows 7 and 23 produce at step 2
    wide, narrow = run((stop,))
    assert 1 <= wide[1][7] == wide[1][23] <= 3, wide[1]
    assert np.array_equal(wide[0], narrow[0]), "tokens differ from the narrow batches'"
    assert np.array_equal(wide[1], narrow[1]) and np.array_equal(wide[2], narrow[2]), (wide[1], narrow[1], wide[2], narrow[2])
    for r in range(B):
        for x, y, name in zip(wide[3][r], narrow[3][r], "KV"):
            assert np.array_equal(x, y), f"{fmt} row {r}: {name} differ from the narrow batch's"
        if r in IDLE:
            assert np.all(wide[0][:, r] == -1) and wide[1][r] == 0 and wide[2][r] == 50
            assert np.all(wide[3][r][0] == NAN) and np.all(wide[3][r][1] == NAN), f"idle row {r}'s cache was written"
        else:
            assert wide[2][r] == pos[r] + wide[1][r]
    dec.release()


# ------------------------------------------------------------------------------------------ 5. the default sampler
def test_the_default_sampler(acc, small_i4):
    import metalchat_amd as mc

    B, pos0, pair = 40, 30, (1234567, 89)
    dec = small_decoder(acc, SMALL, small_i4)
    dec.set_sampler(mc.SAMPLER_DEFAULT, top_k=40, temperature=0.9, top_p=0.95)
    caches = [[random_cache(SMALL, pos0, 700 + r)] for r in range(B)]
    first = np.array([5 + 37 * r for r in range(B)], np.int32)
    wide = mc.Batch(dec, B, wide=True)
    wide.set_seeds([pair])
    import_rows(wide, 0, caches)
    got = wide.generate(first, pos0, 3)
    last = wide.step(got[2], pos0 + 3)
    logits = wide.logits()
    for r in range(B):  # the reference's make_default_sampler on the device's own logits
        want = mo.sample_default(BF16, logits[r], top_k=40, temperature=0.9, top_p=0.95, init_state=pair[0], init_seq=pair[1])
        assert last[r] == want, (r, last[r], want)
    for r0, m, nb in narrow_batches(dec, B):
        nb.set_seeds([pair])
        import_rows(nb, r0, caches)
        assert np.array_equal(nb.generate(first[r0:r0 + m], pos0, 3), got[:, r0:r0 + m]), f"rows {r0}.. sampled tokens"
        assert np.array_equal(nb.step(got[2, r0:r0 + m], pos0 + 3), last[r0:r0 + m])
        assert np.array_equal(nb.logits(), logits[r0:r0 + m])
        nb.release()
    wide.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 6. the packed passes
def prompt_gemms(names):
    return sorted({n for n in names if n.startswith("mc_pf") and "gemm" in n})


@pytest.mark.parametrize("call", ["prefill_rows", "extend_rows"])
@pytest.mark.parametrize("fmt", ["i4", "w"])
def test_packed_passes(acc, small_i4, small_w, fmt, call):
    import metalchat_amd as mc

    B = 40
    dec = small_decoder(acc, SMALL, weights_of(fmt, small_i4, small_w))
    rng = np.random.default_rng(17)
    lens_big = [2] * B
    for r in (5, 18, 33):
        lens_big[r] = 0
    lens_big[39], lens_big[16], lens_big[17] = 33, 17, 16
    lens_big[0] = lens_big[20] = lens_big[31] = 9                                  # 155 packed rows
    lens_small = [0] * B
    lens_small[39], lens_small[16], lens_small[0], lens_small[7] = 33, 17, 9, 2    # 61: the other side of int4's 64-row line
    ctx = [(r * 37) % 151 if call == "extend_rows" else 0 for r in range(B)]       # contexts of 0 .. 150
    caches = [[random_cache(SMALL, ctx[r], 300 + r)] if ctx[r] else None for r in range(B)]
    chunks = [rng.integers(0, SMALL["vocab"], 33).astype(np.int32) for _ in range(B)]
    alone = mc.Batch(dec, 8)
    compared = []
    for lens in (lens_big, lens_small):
        prompts = [chunks[r][:lens[r]] if lens[r] else None for r in range(B)]
        wide = mc.Batch(dec, B, wide=True)
        import_rows(wide, 0, caches)
        dec.launch_log(True)
        nxt = getattr(wide, call)(prompts, ctx)
        gemms = prompt_gemms(dec.launched())
        logits, lengths = wide.logits(), wide.lengths()
        for r in range(B):
            if not lens[r]:
                assert nxt[r] == -1 and lengths[r] == ctx[r]
                continue
            assert lengths[r] == ctx[r] + lens[r]
            # the row alone in a batch of 8, at index r % 8
            i = r % 8
            if caches[r]:
                alone.import_kv(i, 0, *caches[r][0])
            one, pos1 = [None] * 8, [0] * 8
            one[i], pos1[i] = prompts[r], ctx[r]
            dec.launch_log(True)
            nxt1 = getattr(alone, call)(one, pos1)
            if fmt == "i4" and prompt_gemms(dec.launched()) != gemms:
                continue   # the 64-packed-row line of mc_pf2_gemm_i4_* (DESIGN.md "Company, precisely"): another order of sums
            compared.append((sum(lens), r))
            what = f"{call} {fmt} row {r} of {sum(lens)} packed rows"
            assert nxt1[i] == nxt[r], what
            assert np.array_equal(alone.logits()[i], logits[r]), f"{what}: last-row logits"
            for x, y, name in zip(wide.export_row_kv(r, 0), alone.export_row_kv(i, 0), "KV"):
                assert np.array_equal(x, y), f"{what}: {name}"
        dec.launch_log(False)
        wide.release()
    alone.release()
    dec.release()
    if fmt == "w":
        assert len(compared) == 37 + 4, compared
    else:
        assert [c for c in compared if c[0] == 61], "int4: the call of 61 packed rows shares the rows' prompt GEMM"


# ------------------------------------------------------------------------------------------ 7. verify on a wide batch
def test_verify_on_a_wide_batch(acc, small_w):
    """20 rows x 6 tokens = 120 packed rows through verify_rows and as chain trees through verify_tree, against the same rows in
    narrow batches (plain bfloat weights: no prompt GEMM depends on the call's size); a non-chain tree on row 39 against
    tree_rule.walk; 22 x 6 = 132 rows refused"""
    import metalchat_amd as mc

    B, n, pos0 = 40, 6, 50
    dec = small_decoder(acc, SMALL, small_w)
    rows = list(range(0, 40, 2))[:19] + [39]                                       # 20 rows, both sides of every column group
    caches = [[random_cache(SMALL, pos0, 100 + r)] for r in range(B)]
    first = np.array([9 + 31 * r for r in range(B)], np.int32)
    # what every row produces by itself: the drafts are that, wrong from a depth of the row's own
    truth = np.zeros((n, B), np.int32)
    for r0, m, nb in narrow_batches(dec, B):
        import_rows(nb, r0, caches)
        truth[:, r0:r0 + m] = nb.generate(first[r0:r0 + m], pos0, n)
        nb.release()
    prompts = [None] * B
    for j, r in enumerate(rows):
        c = np.concatenate([[first[r]], truth[:n - 1, r]]).astype(np.int32)
        wrong = 1 + j % n                                                          # (n: every draft right)
        if wrong < n:
            c[wrong] = (c[wrong] + 1) % SMALL["vocab"]
        prompts[r] = c
    pos = [pos0] * B

    def both(call, extra):
        out = []
        for batches in ([(0, B, mc.Batch(dec, B, wide=True))], narrow_batches(dec, B)):
            acc_, nxt, picks, lengths = np.zeros(B, np.int32), np.zeros(B, np.int32), [], np.zeros(B, np.int32)
            for r0, m, b in batches:
                import_rows(b, r0, caches)
                if any(p is not None for p in prompts[r0:r0 + m]):
                    res = getattr(b, call)(prompts[r0:r0 + m], *[e[r0:r0 + m] for e in extra], pos[r0:r0 + m])
                    acc_[r0:r0 + m], nxt[r0:r0 + m] = res[0], res[1]
                    picks += list(res[2])
                else:
                    acc_[r0:r0 + m], nxt[r0:r0 + m] = -1, -1
                    picks += [None] * m
                lengths[r0:r0 + m] = b.lengths()
                b.release()
            out.append((acc_, nxt, picks, lengths))
        return out

    chains = [tr.chain(n) if p is not None else None for p in prompts]
    for call, extra in (("verify_rows", []), ("verify_tree", [chains])):
        wide, narrow = both(call, extra)
        assert np.array_equal(wide[0], narrow[0]), (call, wide[0], narrow[0])
        assert np.array_equal(wide[1], narrow[1]) and np.array_equal(wide[3], narrow[3]), call
        for j, r in enumerate(rows):
            assert wide[0][r] == min(j % n, n - 1), (call, r, wide[0])             # the drafts in front of the wrong one
            assert np.array_equal(wide[2][r], narrow[2][r]), f"{call} row {r}: picks"
            assert wide[3][r] == pos0 + wide[0][r] + 1
        for r in range(B):
            if prompts[r] is None:
                assert wide[0][r] == -1 and wide[1][r] == -1 and wide[2][r] is None and wide[3][r] == pos0

    # a tree that is no chain on row 39: a decoy under the root in front of the true child, the true chain below it, a decoy leaf
    t = truth[:, 39]
    toks = np.array([first[39], (t[0] + 1) % SMALL["vocab"], t[0], t[1], (t[2] + 1) % SMALL["vocab"], t[2], t[1]], np.int32)
    par = np.array([-1, 0, 0, 2, 3, 3, 1], np.int32)
    wide = mc.Batch(dec, B, wide=True)
    import_rows(wide, 0, caches)
    trees, parents = [None] * B, [None] * B
    trees[39], parents[39] = toks, par
    a, nx, picks, paths = wide.verify_tree(trees, parents, pos)
    wa, wnx, wpath = tr.walk(toks, par, picks[39])
    assert (a[39], nx[39], list(paths[39])) == (wa, wnx, list(wpath)), (a[39], nx[39], paths[39], wa, wnx, wpath)
    # (the root's pick is the chain's, bit for bit: the decoy in front of the true child is passed over, the match under it never counts)
    assert list(paths[39][:2]) == [0, 2] and 6 not in list(paths[39]), (paths[39], nx[39], t)
    assert wide.lengths()[39] == pos0 + a[39] + 1

    # 22 rows x 6 = 132 packed rows: more than mc_v_head_* holds
    many = [prompts[rows[0]] if r < 22 else None for r in range(B)]
    before = wide.lengths()
    for call in (lambda: wide.verify_rows(many, list(before)), lambda: wide.verify_tree(many, [tr.chain(n) if m is not None else None for m in many], list(before))):
        dec.launch_log(True)
        refused(call, "the chunks add up to 132 rows, more than MC_VERIFY_MAX_ROWS (128): split the call by rows")
        assert dec.launched() == []
        assert np.array_equal(wide.lengths(), before)
    dec.launch_log(False)
    wide.release()
    dec.release()


# ------------------------------------------------------------------------------------------ 8. mc_batch_create is untouched
def test_batch_create_keeps_its_bound(acc, small_i4):
    import metalchat_amd as mc

    dec = small_decoder(acc, SMALL, small_i4)
    refused(lambda: mc.Batch(dec, 9), "mc_batch_create: batch must lie in [1, 8]")
    refused(lambda: mc.Batch(dec, 65, wide=True), "mc_wide_batch_create: batch must lie in [1, 64]")
    b = mc.Batch(dec, 64, wide=True)
    assert b.size() == 64
    b.release()
    dec.release()
