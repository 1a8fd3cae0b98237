"""tests/cpp/test_rows_plan -- a plain g++ program over metalchat_amd/csrc/rows_plan.h, the header batch_rows.cc builds the tables of a rows pass
with -- asked from Python: what the C++ rules make of a call, for the tests that hold rows_tables.py and tree_rule.py to them."""
import json
import subprocess

from metalchat_amd import build as b

RULE = -1   # keys: MC_PX_KEYS not given (rows_plan.h PX_KEYS_RULE)


def call(lens, positions, max_seq_len, *, who="mc_extend_rows", lengths=None, tokens=None, parents=None, vocab=512, keys=RULE, slots=0, verify=False,
         n_heads=8, head_dim=128):
    """one call as a line of the program's input.  lengths: the rows' valid cache positions (default: the positions, every row continues where it
    ends); tokens: the packed ids (default: zeros); parents: the packed parents of a tree call; slots 0: what the host sizes for the heads"""
    total = sum(n for n in lens if n > 0)
    lengths = list(positions) if lengths is None else lengths
    tokens = [0] * total if tokens is None else tokens
    assert len(lens) == len(positions) == len(lengths) and len(tokens) == total and (parents is None or len(parents) == total)
    words = [who, len(lens), max_seq_len, vocab, keys, slots, int(verify or parents is not None), int(parents is not None), n_heads, head_dim,
             *lens, *positions, *lengths, *tokens, *(parents if parents is not None else [])]
    return " ".join(str(int(w)) if not isinstance(w, str) else w for w in words)


def ask(lines):
    """the program's answer to each line: {"refused": text} or the tables of the call"""
    exe = b.build_rows_plan_test()
    out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True).stdout
    answers = [json.loads(a) for a in out.split("\n")[:-1]]
    assert len(answers) == len(lines)
    return answers


def tables(answer):
    """(segs, tiles, ranges, groups) of an admitted call in the shapes rows_tables.py gives them"""
    assert "refused" not in answer, answer
    return ([tuple(g) for g in answer["segs"]], [tuple(t) for t in answer["tiles"]], [tuple(x) for x in answer["ranges"]],
            [tuple(g) for g in answer["groups"]])
