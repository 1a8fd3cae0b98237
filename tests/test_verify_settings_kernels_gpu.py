"""Kernel-level check of the launches a verify call adds for rows with settings (verify_kernels.hip: mc_vs_topk_candidates_mixed_bfloat,
mc_vs_pick_mixed_bfloat, mc_vs_count_accepted; logit_kernels.hip: mc_vs_logits_process_bfloat; include/metalchat_hip.h Part 2m), launched BY
NAME through the Part-1 seam on hand-made bfloat16 logits [23][1300] -- three candidate lists, the last one ragged (276 logits) -- for
segments on rows (5, 0, 2) of B = 8 with lens (2, 16, 5):

  * every picks[m] is what the packed row's sampler picks from ITS logits row with pair (j * 8 + r) % 5: a greedy row the first index
    of the maximum (planted twice), a default row the oracle's make_default_sampler, a drawing row tests/draw_rule.py; top_k 1 / 50 /
    128, temperatures 0.25 / 4, top_p 0 / 1.  n_pairs = 5, so that indexing the pairs by m, by j alone or by r alone gives other pairs
    (asserted on the host); nothing outside picks[0, M) is written;
  * the picks do not depend on the call's kpad: with the top_k = 128 rows set to top_k = 3 the lists shrink from 128 to 64 keys and
    every other row picks the same token;
  * the process launch against tests/logits_rule.py, bit for bit, with the counts c + hist(path): a token repeated on a path, a tree
    `anc` that skips siblings, a token of the slot's history on the path, an unprocessed row untouched (-0.0 included); counts, masks
    and every guard stay as they are;
  * the count launch adds exactly the accepted path -- a chain's rows 0 .. a, a tree's paths[row][0 .. a] -- counts a duplicate twice,
    and leaves rows without penalties and every other word alone."""
import numpy as np
import pytest

import draw_rule as dr
import logits_rule as lr
import parity
import rows_tables as rt
import tree_rule as tr
from oracle import mc_oracle as mo
from test_batch_kernels_gpu import bf, f, first_max

pytestmark = pytest.mark.gpu
BF16 = 0
B, N, CAP, M = 8, 1300, 4096, 23
GREEDY, DEFAULT, DRAW = 0, 1, 2
MASK, PENALTY = 1, 2
NAN, CGUARD, MGUARD, GUARD = 0x7FC0, -77, 0xA5A5A5A5, 64
LENS = [16, 0, 5, 0, 0, 2, 0, 0]
SEGS = [(0, 0, 16), (2, 16, 5), (5, 21, 2)]   # (batch row, first packed row, length), packed in row order
SEEDS = np.array([[0, 0], [123456789, 987654321], [5, 6], [77, 1], [2 ** 40 + 3, 9]], np.uint64)
VR = np.dtype([("kind", np.int32), ("k", np.uint32), ("inv_temp", np.float32), ("top_p", np.float32), ("seed", np.uint32), ("anc", np.uint32),
               ("row", np.int32), ("off", np.int32)])   # kernels/abi.h verify_row
RL = np.dtype([("flags", np.uint32), ("rep", np.float32), ("inv_rep", np.float32), ("freq", np.float32), ("pres", np.float32),
               ("pad", np.uint32, (3,))])   # kernels/abi.h row_logits
# the sampler of each PACKED row (the kernels read the table per packed row): (kind, top_k, temperature, top_p), cycled over the rows
SETTINGS = [(GREEDY, 0, 0.0, 0.0), (DEFAULT, 1, 0.6, 0.9), (DRAW, 128, 0.9, 0.95), (DRAW, 50, 0.6, 0.0), (DEFAULT, 50, 1.3, 1.0),
            (DRAW, 40, 0.25, 0.9), (DRAW, 40, 4.0, 0.95), (DRAW, 50, 1.0, 1.0), (DRAW, 1, 0.8, 0.9), (DEFAULT, 128, 4.0, 1.0)]


def settings_of(m, small=False):
    s = SETTINGS[m % len(SETTINGS)]
    return (s[0], 3, s[2], s[3]) if small and s[1] == 128 else s


def rt_(v):
    return float(f(bf(np.array([v], np.float32)))[0])


def logits_rows():
    """23 rows, |x| <= 9.5 so that exp(x / 0.25) stays finite.  Planted: the maximum twice in different lists (the first wins), rows
    rounded to halves (long runs of equal values), a run of 40 equal logits across the first list boundary, the maximum in the ragged
    last list"""
    rng = np.random.default_rng(2300)
    x = np.clip(rng.normal(0, 2, (M, N)), -9.0, 8.0).astype(np.float32)
    for m in range(M):
        if m % 5 == 0:
            x[m, [900, 17 + m, 1299]] = 9.5
        if m % 5 == 1:
            x[m, 1290 - m] = 9.0
        if m % 5 == 3:
            x[m] = np.round(x[m] * 2) / 2
        if m % 5 == 4:
            x[m, 492:532] = 6.0
    return bf(x)


def vrows(small=False, anc=None):
    t = np.zeros(M, VR)
    for r, off, n in SEGS:
        for j in range(n):
            m = off + j
            kind, top_k, temperature, top_p = settings_of(m, small)
            t[m]["kind"] = kind
            if kind != GREEDY:   # as mc_row_sampler_set forms them
                t[m]["k"], t[m]["inv_temp"], t[m]["top_p"] = min(top_k, N), rt_(1.0 / rt_(temperature)), rt_(top_p)
            t[m]["seed"], t[m]["anc"], t[m]["row"], t[m]["off"] = (j * B + r) % len(SEEDS), (2 << j) - 1 if anc is None else anc[m], r, off
    return t


def test_the_seed_indices_tell_the_indexings_apart():
    seeds = list(vrows()["seed"])
    jr = [(j, r) for r, off, n in SEGS for j in range(n)]
    assert seeds == [(j * B + r) % 5 for j, r in jr]
    assert seeds != [m % 5 for m in range(M)] and seeds != [j % 5 for j, r in jr] and seeds != [r % 5 for j, r in jr]


@pytest.fixture(scope="module")
def wanted():
    """the expected pick of every packed row under SETTINGS and with the top_k = 128 rows at top_k = 3 -- computed once"""
    x = logits_rows()
    seeds = vrows()["seed"]

    def want(m, small):
        kind, top_k, temperature, top_p = settings_of(m, small)
        if kind == GREEDY:
            return first_max(x[m])
        s0, s1 = (int(v) for v in SEEDS[seeds[m]])
        if kind == DEFAULT:
            return mo.sample_default(BF16, x[m], top_k=top_k, temperature=temperature, top_p=top_p, init_state=s0, init_seq=s1)
        return dr.draw(BF16, x[m], top_k=top_k, temperature=temperature, top_p=top_p, seed0=s0, seed1=s1)

    picks = [[want(m, small) for m in range(M)] for small in (False, True)]
    assert picks[0][0] == 17 and picks[0][10] == 27 and picks[0][1] == 1289   # greedy: the first maximum; top_k = 1: the maximum
    drawn = [m for m in range(M) if settings_of(m)[0] == DRAW and picks[0][m] != first_max(x[m])]
    assert len(drawn) >= 4, drawn   # the draws are not all the argmax: the pairs matter
    return x, picks


def test_packed_rows_pick_as_their_own_sampler(acc, wanted):
    import metalchat_amd as mc

    x, picks = wanted
    lb = acc.to_device(x.reshape(-1))
    seeds = acc.to_device(SEEDS.reshape(-1))
    for small, kpad_want in ((False, 128), (True, 64)):
        kpad = 1
        while kpad < max(settings_of(m, small)[1] for m in range(M)):
            kpad *= 2
        assert kpad == kpad_want
        lists = -(-N // 512)
        assert lists == 3
        tb = acc.to_device(vrows(small).view(np.uint8))
        cand = acc.alloc(M * lists * 128 * 8)
        pb = acc.to_device(np.full(GUARD + M + GUARD, -7, np.int32))
        mc.KernelTask(acc.load("mc_vs_topk_candidates_mixed_bfloat"), (lists * 64, M, 1), (64, 1, 1),
                      [lb, np.uint32(N), np.uint32(kpad), cand, np.uint32(512), tb])()
        mc.KernelTask(acc.load("mc_vs_pick_mixed_bfloat"), (1024, M, 1), (1024, 1, 1),
                      [lb, np.uint32(N), cand, tb, np.uint32(lists), np.uint32(kpad), np.uint32(CAP), seeds, np.uint32(len(SEEDS)), (pb, GUARD * 4)],
                      lds_bytes=CAP * 8)()
        acc.wait()
        got = pb.download(np.int32, GUARD + M + GUARD)
        for m in range(M):
            assert got[GUARD + m] == picks[small][m], f"kpad {kpad} packed row {m} {settings_of(m, small)}: picked {got[GUARD + m]}, expected {picks[small][m]}"
            if settings_of(m)[1] != 128:
                assert picks[small][m] == picks[0][m]
        exp = np.full(GUARD + M + GUARD, -7, np.int32)
        exp[GUARD:GUARD + M] = picks[small]
        parity.exact(got, exp, f"kpad {kpad}: picks and the words around them")
    parity.exact(lb.download(np.uint16, M * N).reshape(M, N), x, "the logits")


# the processors of the batch rows: row 0 a mask and all three penalties, row 2 nothing, row 5 penalties alone
PROC = {0: (True, 1.25, 0.25, 2.0 ** -8), 2: (False, 1.0, 0.0, 0.0), 5: (False, 1.5, 2.0 ** -8, 0.5)}
#   row 0's chunk as a tree of 16 nodes: two branches under the root that skip each other's nodes, a chain under each
PARENTS0 = [-1, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]


def rl_table():
    t = np.zeros(B, RL)
    for r, (masked, rep, freq, pres) in PROC.items():
        pen = not (rep == 1.0 and freq == 0.0 and pres == 0.0)
        t[r]["flags"] = (MASK if masked else 0) | (PENALTY if pen else 0)
        if pen:
            t[r]["rep"], t[r]["inv_rep"], t[r]["freq"], t[r]["pres"] = rep, np.float32(1.0) / np.float32(rep), freq, pres
    return t


def guarded(acc, body, guard_value):
    g = np.full(GUARD, guard_value, body.dtype)
    host = np.concatenate([g, body.reshape(-1), g])
    return acc.to_device(host), host, GUARD * body.dtype.itemsize


def process_inputs(n):
    rng = np.random.default_rng(n + 23)
    x = bf(np.clip(rng.normal(0, 3, (M, n)), -9.0, 9.0))
    x[:, 9] = 0x8000          # -0.0
    x[:, 11] = bf(np.float32(2.0))
    counts = np.where(rng.random((B, n)) < 0.1, rng.integers(1, 5, (B, n)), 0).astype(np.int32)
    counts[:, 9] = 0
    allowed = rng.random((B, n)) < 0.5
    allowed[:, [9, 11]] = True
    # the chunk tokens: row 0's both branches repeat token 40 (nodes 1, 3, 5 on one path, 2 on the other), carry a token of the slot's history
    # (11, counted 2 already) and the row's last token n - 1; row 5's chain feeds token 7 twice
    tokens = rng.integers(0, n, M).astype(np.int32)
    tokens[[1, 3, 5, 2]] = 40
    tokens[7] = 11
    tokens[15] = n - 1
    tokens[8] = 8             # (inside the first 16-byte piece of an aligned row)
    counts[0, 11] = 2
    counts[0, 40] = 0
    tokens[21:23] = 7
    counts[5, 7] = 1
    return x, counts, allowed, tokens


@pytest.mark.parametrize("n", [1300, 2056])
def test_processed_packed_rows_equal_the_rule(acc, n):
    """n = 1300: one chunk, 2600-byte rows, so the odd packed rows start off a 16-byte boundary (elements in front of the first whole piece and behind
    the last); n = 2056: two chunks, the second of 8 logits"""
    import metalchat_amd as mc

    x, counts, allowed, tokens = process_inputs(n)
    anc = np.zeros(M, np.uint32)
    anc[:16] = tr.anc_masks(PARENTS0)
    for r, off, ln in SEGS[1:]:
        anc[off:off + ln] = [(2 << j) - 1 for j in range(ln)]
    assert anc[5] == 0b101011 and anc[6] == 0b1010101   # the branches skip each other's nodes
    words = np.stack([lr.mask_words(allowed[r]) for r in range(B)])
    lb, lhost, loff = guarded(acc, x, np.uint16(NAN))
    cb, chost, coff = guarded(acc, counts, np.int32(CGUARD))
    mb, mhost, moff = guarded(acc, words, np.uint32(MGUARD))
    kb, khost, koff = guarded(acc, tokens, np.int32(n + 5))
    vt = vrows(anc=anc)
    gx = -(-n // 2048)
    mc.KernelTask(acc.load("mc_vs_logits_process_bfloat"), (gx * 256, M, 1), (256, 1, 1),
                  [(lb, loff), np.uint32(n), acc.to_device(vt.view(np.uint8)), acc.to_device(rl_table().view(np.uint8)), (mb, moff), (cb, coff), (kb, koff)])()
    acc.wait()
    what = f"n {n}"
    parity.exact(cb.download(np.int32, chost.size), chost, f"{what}: the counts and their guards are only read")
    parity.exact(mb.download(np.uint32, mhost.size), mhost, f"{what}: the masks and their guards")
    parity.exact(kb.download(np.int32, khost.size), khost, f"{what}: the tokens")
    got_l = lb.download(np.uint16, lhost.size)
    parity.exact(got_l[:GUARD], lhost[:GUARD], f"{what}: the guard in front of the logits")
    parity.exact(got_l[GUARD + M * n:], lhost[GUARD + M * n:], f"{what}: the guard behind the logits")
    got = got_l[GUARD:GUARD + M * n].reshape(M, n)
    for r, off, ln in SEGS:
        masked, rep, freq, pres = PROC[r]
        for j in range(ln):
            m = off + j
            path = [off + i for i in range(16) if (int(anc[m]) >> i) & 1]
            assert path[-1] == m and (r == 0 or path == list(range(off, m + 1)))
            c = counts[r] + np.bincount(tokens[path], minlength=n)
            exp = lr.process(x[m], c if (rep, freq, pres) != (1.0, 0.0, 0.0) else None, allowed[r] if masked else None, rep, freq, pres)
            parity.exact(got[m], exp, f"{what}: packed row {m} (row {r}, node {j}, path {path})")
            if r == 2:
                parity.exact(got[m], x[m], f"{what}: packed row {m} of the unprocessed row keeps every bit")
                assert got[m, 9] == 0x8000
    # what the plants became.  Node 5 of row 0 has token 40 three times on its path (nodes 1, 3, 5) and not the other branch's (node 2);
    # node 6 has it once (node 2)
    c5 = counts[0] + np.bincount(tokens[[0, 1, 3, 5]], minlength=n)
    c6 = counts[0] + np.bincount(tokens[[0, 2, 4, 6]], minlength=n)
    assert c5[40] == 3 and c6[40] == 1
    assert c5[11] == 2 and (counts[0] + np.bincount(tokens[[0, 1, 3, 5, 7]], minlength=n))[11] == 3   # history + the path
    assert (counts[5] + np.bincount(tokens[[21, 22]], minlength=n))[7] == 3                               # a token fed twice by a chain


def test_the_count_launch_adds_the_accepted_path(acc):
    import metalchat_amd as mc

    n = 1300
    _, counts, _, tokens = process_inputs(n)
    segs = rt.segments(LENS, [3, 0, 40, 0, 0, 7, 0, 0])
    assert [(row, off, ln) for row, _, off, ln in segs] == SEGS
    tab = acc.to_device(rl_table().view(np.uint8))
    sb = acc.to_device(rt.words(segs, 4).reshape(-1))
    kb = acc.to_device(tokens)
    # a chain: rows 0 .. a.  Row 0 accepts 5 drafts (tokens 1, 3, 5 are all 40: counted three times, node 2's 40 a fourth time), row 2 has no
    # penalties, row 5 accepts everything (token 7 twice)
    accepted = np.array([5, -1, 4, -1, -1, 1, -1, -1], np.int32)
    # a tree: row 0 walks the branch 0 - 1 - 3 - 5 - 7 (token 40 three times, node 2 is NOT on the path), row 5 stops at its root
    paths = np.full((B, 16), -1, np.int32)
    paths[0, :5], paths[2, :3], paths[5, :1] = [0, 1, 3, 5, 7], [0, 1, 2], [0]
    tree_accepted = np.array([4, -1, 2, -1, -1, 0, -1, -1], np.int32)
    for what, acc_host, path_host in (("chain", accepted, None), ("tree", tree_accepted, paths)):
        cb, chost, coff = guarded(acc, counts, np.int32(CGUARD))
        ab = acc.to_device(acc_host)
        pb = acc.to_device(path_host.reshape(-1)) if path_host is not None else None
        mc.KernelTask(acc.load("mc_vs_count_accepted"), (len(segs) * 64, 1, 1), (64, 1, 1), [sb, kb, ab, pb, tab, (cb, coff), np.uint32(n)])()
        acc.wait()
        exp = counts.copy()
        for r, off, ln in SEGS:
            if r == 2:
                continue   # no penalties: its counts are not touched
            nodes = range(acc_host[r] + 1) if path_host is None else path_host[r, :acc_host[r] + 1]
            for node in nodes:
                exp[r, tokens[off + node]] += 1
        assert exp[0, 40] - counts[0, 40] == (4 if path_host is None else 3), what
        assert exp[5, 7] - counts[5, 7] == (2 if path_host is None else 1), what
        assert exp.sum() - counts.sum() == ((6 + 2) if path_host is None else (5 + 1))
        exp_host = chost.copy()
        exp_host[GUARD:GUARD + B * n] = exp.reshape(-1)
        parity.exact(cb.download(np.int32, chost.size), exp_host, f"{what}: the counts and their guards")
        parity.exact(ab.download(np.int32, B), acc_host, f"{what}: accepted")
