"""The state of a rolling row (include/metalchat_hip.h Part 2j) restated in Python: what mc_b_rows_begin_rolling derives from a row's
position alone, a literal replay of the batch-1 decoder's derive_state (decode_kernels.hip) to hold it to, and the logical view a
rolled row exports.  The CPU test compares the two; the GPU tests hold the device to them."""


def pre_len(S):
    """nn::sink_cache's default: bit_width(max_seq_len) - 1 (nn/cache.h:125-127)"""
    return S.bit_length() - 1


def state(p, S, pre=None):
    """(ring_base, write_slot, kv_len) of a row whose step sits at position p"""
    pre = pre_len(S) if pre is None else pre
    if p < S:
        return 0, p, p + 1
    post = S - pre
    ring_base = (p - S + 1) % post
    return ring_base, pre + (post - 1 + ring_base) % post, S


def replay(n, S, pre=None):
    """derive_state stepped through positions 0 .. n - 1 from a fresh cache: the (ring_base, write_slot, kv_len) of every step"""
    pre = pre_len(S) if pre is None else pre
    post = S - pre
    ring_base, out = 0, []
    for pos in range(n):
        if pos >= S:
            ring_base = (ring_base + 1) % post
            write_slot = pre + (post - 1 + ring_base) % post
            kv_len = S
        else:
            write_slot = pos if pos < pre else pre + (pos - pre + ring_base) % post
            kv_len = pos + 1
        out.append((ring_base, write_slot, kv_len))
    return out


def positions_held(length, S, pre=None):
    """the absolute position behind each logical row of a row of `length` positions: [0, length) while linear, else the sink rows
    and the last S - pre positions"""
    pre = pre_len(S) if pre is None else pre
    if length <= S:
        return list(range(length))
    return list(range(pre)) + list(range(length - (S - pre), length))
