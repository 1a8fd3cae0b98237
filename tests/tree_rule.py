"""The rules of mc_tree_verify (include/metalchat_hip.h Part 2g), restated in Python for the CPU and GPU tests.

A row's chunk is a tree of n <= 16 nodes in topological order: tokens[0] is the row's last accepted token (the root, parent -1),
nodes 1 .. n - 1 are drafts and parents[i] < i names node i's parent.  pick[i] is the target's greedy pick after node i.

  depths / ancestor masks   depth(0) = 0, depth(i) = depth(parent) + 1; bit j of anc(i): node j is an ancestor of i, or i itself
                            (the host's tv_node table, kernels/abi.h)
  the walk                  cur = 0; among cur's children in ascending index the first j with tokens[j] == pick[cur] becomes cur;
                            stop when there is none.  accepted = depth(cur), next token = pick[cur], path = the nodes root -> cur
  the compaction            during the pass node i's K / V sit in cache slot pos + i; afterwards slot pos + d holds the K / V of
                            path[d] for d <= accepted -- a permutation-like move of slots, every other slot untouched
  trie                      candidate continuations of one last token merged into (tokens, parents)

This is a RESTATEMENT of kernels/tree_kernels.hip (mc_tv_accept, mc_tv_compact_bfloat) and of csrc/rows_plan.h tree_nodes;
test_tree_kernels_gpu.py binds the kernels to it on the device, test_rows_tables_cpu.py and test_tree_verify_cpu.py bind depths / anc_masks to
the host's tree_nodes on the CPU (tests/cpp/test_rows_plan, a plain g++ program over that header)."""
import numpy as np

MAX_NODES = 16


def check_parents(parents):
    parents = [int(p) for p in parents]
    assert 1 <= len(parents) <= MAX_NODES and parents[0] == -1
    assert all(0 <= p < i for i, p in enumerate(parents) if i), parents
    return parents


def depths(parents):
    parents = check_parents(parents)
    d = [0] * len(parents)
    for i in range(1, len(parents)):
        d[i] = d[parents[i]] + 1
    return d


def anc_masks(parents):
    """anc[i]: bit j set when node j is an ancestor of node i or i itself"""
    parents = check_parents(parents)
    a = [1] * len(parents)
    for i in range(1, len(parents)):
        a[i] = a[parents[i]] | (1 << i)
    return a


def ancestors(parents, i):
    """the path root -> i as node indices (ascending)"""
    m = anc_masks(parents)[i]
    return [j for j in range(len(parents)) if (m >> j) & 1]


def chain(n):
    """the parents of a chain of n nodes: mc_verify_rows' chunk as a tree"""
    return np.arange(-1, n - 1, dtype=np.int32)


def walk(tokens, parents, picks):
    """(accepted, next token, path) of one row"""
    tokens, picks, parents = [int(t) for t in tokens], [int(t) for t in picks], check_parents(parents)
    assert len(tokens) == len(picks) == len(parents)
    cur, path = 0, [0]
    while True:
        nxt = next((j for j in range(cur + 1, len(tokens)) if parents[j] == cur and tokens[j] == picks[cur]), None)
        if nxt is None:
            return len(path) - 1, picks[cur], path
        cur = nxt
        path.append(cur)


def walk_rows(tokens, parents, picks):
    """per batch row (None: not in the call) -> accepted[B], next_tokens[B], paths[B][16]; -1 for a row not in the call and
    behind a path's end"""
    B = len(tokens)
    acc, nxt, paths = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.full((B, MAX_NODES), -1, np.int32)
    for r in range(B):
        if tokens[r] is not None:
            acc[r], nxt[r], path = walk(tokens[r], parents[r], picks[r])
            paths[r, :len(path)] = path
    return acc, nxt, paths


def compact(slots, pos, path):
    """the cache after the call: `slots` is indexed by cache slot along axis 0 (any trailing shape); slot pos + d takes what slot
    pos + path[d] held, d = 1 .. len(path) - 1, everything else stays.  path is strictly ascending with path[d] >= d, so moving in
    ascending d never reads a slot that was overwritten -- the copy below and the in-place loop of the kernel agree."""
    path = [int(p) for p in path]
    assert path[0] == 0 and all(a < b for a, b in zip(path, path[1:])) and all(p >= d for d, p in enumerate(path))
    out = np.array(slots, copy=True)
    for d in range(1, len(path)):
        out[pos + d] = slots[pos + path[d]]
    return out


def trie(last, candidates, max_nodes=MAX_NODES):
    """(tokens, parents) int32 arrays in topological order: node 0 is `last`, the candidate continuations (token lists, best
    first) are merged by common prefix.  Nodes are added candidate by candidate, a candidate's new nodes in order of depth, so a
    parent always precedes its children and earlier candidates get the lower indices (they win among equal siblings -- there are
    none here: equal siblings are merged).  A candidate is cut where the tree is full."""
    tokens, parents, children = [int(last)], [-1], [{}]
    for cand in candidates:
        cur = 0
        for t in cand:
            t = int(t)
            if t not in children[cur]:
                if len(tokens) >= max_nodes:
                    break
                children[cur][t] = len(tokens)
                tokens.append(t)
                parents.append(cur)
                children.append({})
            cur = children[cur][t]
    return np.array(tokens, np.int32), np.array(parents, np.int32)
