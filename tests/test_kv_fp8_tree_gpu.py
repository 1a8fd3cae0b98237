"""mc_tree_verify on an fp8 batch (mc_kv_tree_set, include/metalchat_hip.h Part 2q) through the public calls, on the small synthetic decoder of
test_batch_gpu.py with int4 and with plain weights.  What can be pinned bit for bit: a chain tree is verify_rows on a twin fp8 batch; layer 0's
K / V depend on no cache, so after a branching tree the row's export is that of a twin fed the accepted tokens by extend_rows -- the compaction moved
bytes and exponents, nothing was quantised again -- and the ragged step behind it computes the twin's bits; a row's bits do not depend on its
company.  The one statement about accuracy is measured against the bfloat16 batch making the same call."""
import numpy as np
import pytest

import parity
import tree_rule as tr
from oracle import mc_oracle as mo
from test_batch_gpu import SMALL, refused
from test_kv_fp8_batch_gpu import prompt as toks, weights  # noqa: F401 (the module's fixture: int4 and plain weights of SMALL)
from test_kv_fp8_rows_gpu import dec, rel_l2  # noqa: F401 (the fixture: a decoder per weight kind)
from test_kv_fp8_tree_kernels_gpu import PATH, TREE16

pytestmark = pytest.mark.gpu
POS = 33                    # the context fills the first 32-key block and one key more; the tree's slots are 33 .. 48
VOCAB = SMALL["vocab"]


def batch(dec, B, kv="fp8", tree=True):
    import metalchat_amd as mc

    b = mc.Batch(dec, B, wide=True, kv=kv)
    b.set_kv_packed(True)
    b.set_kv_tree(tree)
    return b


def argmax(logits):
    return int(np.argmax(mo.from_bf16(logits)))


def test_the_tree_switch_alone_admits_the_tree(dec):
    f8, b16 = batch(dec, 2, tree=False), batch(dec, 2, kv="bf16", tree=False)
    chunk, tree = [toks(3, 1), None], [np.array([-1, 0, 0], np.int32), None]
    assert not f8.kv_tree and f8.kv_packed
    refused(lambda: f8.verify_tree(chunk, tree, [0, -1]), "mc_tree_verify: the batch holds an fp8 cache")
    parity.exact(f8.lengths(), np.zeros(2, np.int32), "the lengths after the refused call")
    for b in (f8, b16):                                   # (a bfloat16 batch accepts the switch, which changes nothing)
        b.set_kv_tree(True)
        assert b.kv_tree
        acc_ = b.verify_tree(chunk, tree, [0, -1])[0]
        parity.exact(b.lengths(), np.array([acc_[0] + 1, 0], np.int32), "the lengths after the admitted call")
    refused(lambda: f8.verify_tree(chunk, [np.array([-1, 2, 0], np.int32), None], [0, -1]), "mc_tree_verify")   # (its own checks hold)
    for b in (f8, b16):
        b.release()


def test_a_chain_tree_is_verify_rows_bit_for_bit(dec):
    ctx, drafts = [toks(n, 40 + n) for n in (POS, 16)], [toks(16, 60), toks(5, 61)]
    tree, rows = batch(dec, 2), batch(dec, 2)
    for b in (tree, rows):
        b.prefill_rows(ctx)
    drafts[0][1] = rows.verify_rows(drafts, [POS, 16])[2][0][0]         # row 0's first draft is what the target picks: accepted
    got, want = tree.verify_tree(drafts, [tr.chain(16), tr.chain(5)], [POS, 16]), rows.verify_rows(drafts, [POS, 16])
    assert got[0][0] >= 1
    for g, w, name in zip(got[:2], want[:2], ("accepted", "next tokens")):
        parity.exact(g, w, f"a chain tree: {name}")
    for r in range(2):
        parity.exact(got[2][r], want[2][r], f"a chain tree: row {r}'s picks")
        parity.exact(tree.verify_logits()[r], rows.verify_logits()[r], f"a chain tree: row {r}'s logits after every node")
        for x, y, name in zip(tree.export_row_kv(r, 0), rows.export_row_kv(r, 0), ("K", "V")):
            parity.exact(x, y, f"a chain tree: row {r}'s layer-0 {name}")
    parity.exact(tree.logits(), rows.logits(), "a chain tree: the accepted rows' logits")
    parity.exact(tree.lengths(), rows.lengths(), "a chain tree: the lengths")
    for b in (tree, rows):
        b.release()


def greedy(dec, ctx, root, n):
    """the target's n greedy tokens behind ctx + [root], by verify_rows on a scratch fp8 batch (a draft behind the probe is never seen)"""
    b, chain = batch(dec, 1), [int(root)]
    b.prefill_rows([ctx])
    for _ in range(n):
        chain.append(int(b.verify_rows([np.array(chain + [0], np.int32)], [len(ctx)])[2][0][len(chain) - 1]))
    b.release()
    return chain[1:]


def branching(dec, ctx, root):
    """TREE16 whose true path is PATH = 0 -> 2 -> 5 -> 11: the greedy tokens on it, and everywhere else a token no pick of the path equals"""
    g = greedy(dec, ctx, root, 4)
    tokens = np.array([root] + [(max(g) + 1 + i) % VOCAB for i in range(1, 16)], np.int32)
    assert not set(tokens[1:]) & set(g)
    tokens[PATH[1:]] = g[:3]
    return tokens, np.array(TREE16, np.int32), g


def test_a_branching_tree_leaves_the_cache_of_the_accepted_tokens(dec):
    ctx, other, root = toks(POS, 70), toks(16, 71), 7
    tokens, parents, g = branching(dec, ctx, root)
    f8, alone = batch(dec, 4), batch(dec, 2)
    f8.prefill_rows([other, None, None, ctx])
    alone.prefill_rows([None, ctx])
    acc_, nxt, picks, paths = f8.verify_tree([toks(5, 72), None, None, tokens], [np.array([-1, 0, 0, 1, 3], np.int32), None, None, parents], [16, -1, -1, POS])
    a1, n1, p1, _ = alone.verify_tree([None, tokens], [None, parents], [-1, POS])
    assert acc_[3] == 3 and list(paths[3]) == PATH and nxt[3] == g[3] == picks[3][PATH[3]], (acc_, paths[3], nxt, g)
    parity.exact(f8.lengths()[3:], np.array([POS + 4], np.int32), "the length is pos + accepted + 1")
    # a row computes the same bits alone as among other rows
    assert (a1[1], n1[1]) == (acc_[3], nxt[3])
    parity.exact(p1[1], picks[3], "the row's picks alone and among other rows")
    parity.exact(alone.verify_logits()[1], f8.verify_logits()[3], "the row's logits after every node alone and among other rows")
    # the twin: the accepted tokens by extend_rows; a twin per prefix says what the target picks after it
    for d in range(1, 4):
        twin = batch(dec, 1)
        twin.prefill_rows([ctx])
        twin.extend_rows([np.array([root] + g[:d], np.int32)], [POS])
        assert picks[3][PATH[d]] == argmax(twin.logits()[0]), f"the pick after the path's node at depth {d}"
        if d < 3:
            twin.release()
    for b, r in ((f8, 3), (alone, 1)):
        for x, y, name in zip(b.export_row_kv(r, 0), twin.export_row_kv(0, 0), ("K", "V")):
            assert x.shape[0] == POS + 4
            parity.exact(x, y, f"layer-0 {name} over the new length is the twin's: the path's vectors moved unchanged")
    # a ragged step continues: the caches hold the same bytes and exponents, so the step computes the twin's bits
    t = f8.step_rows(np.array([1, 0, 0, nxt[3]], np.int32), [int(f8.lengths()[0]), -1, -1, POS + 4])
    tt = twin.step_rows(np.array([nxt[3]], np.int32), [POS + 4])
    assert t[3] == tt[0] >= 0 and t[0] >= 0
    parity.exact(f8.logits()[3], twin.logits()[0], "the ragged step behind the call against the twin's")
    for b in (f8, alone, twin):
        b.release()


# relative L2 error of the fp8 batch's logits after every node of the call against the bfloat16 batch's making the same verify_tree call (a
# branching tree of 16 nodes behind 33 tokens and one of 5 behind 16), as measured on an MI355X with these weights.  The assertion allows twice
# that, the margin of Parts 2o and 2p.
MEASURED = {"i4": 6.75576e-3, "w": 6.06202e-3}


def test_logits_stay_close_to_the_bfloat16_batch(dec, request):
    fmt = request.node.callspec.params["dec"]
    ctx, root = [toks(POS, 70), toks(16, 71)], 7
    tokens, parents, _ = branching(dec, ctx[0], root)
    f8, b16 = batch(dec, 2), batch(dec, 2, kv="bf16")
    for b in (f8, b16):
        b.prefill_rows(ctx)
        b.verify_tree([tokens, toks(5, 72)], [parents, np.array([-1, 0, 0, 1, 3], np.int32)], [POS, 16])
    err = rel_l2(np.concatenate(f8.verify_logits()), np.concatenate(b16.verify_logits()))
    print(f"kv fp8 tree closeness {fmt}: relative L2 error of the logits after every node: {err}")
    assert err <= 2 * MEASURED[fmt], (fmt, err, MEASURED[fmt])
    for b in (f8, b16):
        b.release()
