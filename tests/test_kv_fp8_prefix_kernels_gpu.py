"""The shared-prefix attention kernels of an fp8 batch (kv8_prefix_kernels.hip, Part 2s) by name, with test_prefix_kernels_gpu.py's row set -- four
attached rows at kv_len shared + 1, + 32, + 33, + 65, an ordinary row between them, an idle row -- against the per-row _f8_rows kernels on planes
that hold a byte copy of the prefix, bit for bit, at 1, 2 and 4 groups per P.V workgroup, and against the float64 oracle on the deq values within
test_attention_f8_is_the_bfloat16_attention_on_deq's bounds.  What must never be read holds NaN bytes (0x7f) under exponent -128: an attached
row's own slots [0, shared), the prefix planes behind shared, every row's slots at and past kv_len."""
import numpy as np
import pytest

import kv_fp8_rule as kr
import parity
from test_attn_kernels_gpu import oracle_attention
from test_batch_kernels_gpu import BF16, NAN, PB, ST_POS, bf, f, state_at, states
from test_kv_fp8_kernels_gpu import G as GUARD8, guarded8

pytestmark = pytest.mark.gpu
# S, H, KV, hd: n_rep 4 with a second round of k-steps; n_rep 8; G = 1 (six groups) and the clamped V load at max_seq - 8; n_rep 3 (G n_rep = 15 < 16)
SHAPES = [(2240, 32, 8, 128), (1000, 32, 4, 64), (104, 16, 1, 128), (256, 6, 2, 64)]
CASES = [(*s, sh, 1) for s in SHAPES for sh in sorted({64, (s[0] - 2) // 64 * 64})]
# the row set three times over at n_rep 4 (18 rows, five groups), the middle copy not attached: a last workgroup with fewer than GW groups, and
# group 2 without an attached row beside groups that have some
CASES.append((256, 32, 8, 128, 64, 3))
_reference = {}


def planes(vecs, S, lens, transposed, hide=()):
    """fp8 planes [B, KV, S, hd] (transposed: [B, KV, hd, S]) and exponents [B, KV, S] of vecs[r] [n, KV, hd]; NaN bytes under -128 past n and in
    the slots hide[r] = (0, shared)"""
    B, (KV, hd) = len(vecs), vecs[0].shape[1:]
    q, x = np.full((B, KV, S, hd), 0x7F, np.uint8), np.full((B, KV, S), -128, np.int8)
    for r, v in enumerate(vecs):
        qb, qe = kr.quant(v)
        q[r, :, :len(v)], x[r, :, :len(v)] = qb.transpose(1, 0, 2), qe.T
    for r, (a, b) in hide:
        q[r, :, a:b], x[r, :, a:b] = 0x7F, -128
    return (np.ascontiguousarray(q.transpose(0, 1, 3, 2)) if transposed else q), x


def reference(acc, S, H, KV, hd, shared, times):
    """the inputs and, computed once per shape, what the per-row _f8_rows kernels give on full copies"""
    key = (S, H, KV, hd, shared, times)
    if key in _reference:
        return _reference[key]
    import metalchat_amd as mc

    nsplit, n_rep = (S + PB - 1) // PB, H // KV
    att = [min(S, shared + d) for d in (1, 32, 33, 65)]
    lens = [att[0], att[1], min(S, 70), att[2], att[3], -1] * times
    attached = [c != 1 and a for c in range(times) for a in (True, True, False, True, True, False)]
    B = len(lens)
    rng = np.random.default_rng(S + shared + times)
    q = bf(rng.normal(0, 1, (B, H, hd)))
    vec = lambda n, sd: bf(rng.normal(0, sd, (n, KV, hd)) * np.exp2(rng.integers(-3, 3, (n, KV, 1))))
    pk, pv = vec(shared, 0.4), vec(shared, 0.5)
    ks, vs = [vec(max(n, 0), 0.4) for n in lens], [vec(max(n, 0), 0.5) for n in lens]
    for r in range(B):
        if attached[r]:
            ks[r][:shared], vs[r][:shared] = pk, pv
    hide = [(r, (0, shared)) for r in range(B) if attached[r]]
    scale = float(f(bf(np.array([hd ** -0.5])))[0])
    st = states(B)
    for r, n in enumerate(lens):
        if n > 0:
            st[r] = state_at(n)
        st[r, ST_POS] = n - 1 if n > 0 else -1
    d = dict(B=B, lens=lens, attached=attached, nsplit=nsplit, n_rep=n_rep, scale=scale, q=q, st=acc.to_device(st.reshape(-1)), qb=acc.to_device(q.reshape(-1)),
             sentinel=np.full(B * H * S, -7.0, np.float32), deq=[(kr.roundtrip(k), kr.roundtrip(v)) for k, v in zip(ks, vs)],
             own=planes(ks, S, lens, False, hide) + planes(vs, S, lens, True, hide), prefix=planes([pk], S, [shared], False) + planes([pv], S, [shared], True))
    d["tail"] = [np.uint32(n_rep), np.uint32(hd), np.uint32(S)]
    d["strides"] = [np.uint64(KV * S * hd + GUARD8), np.uint64(KV * S + GUARD8)]
    kq, kx, vq, vx = (acc.to_device(guarded8(p.reshape(B, -1).view(np.uint8)).reshape(-1)) for p in planes(ks, S, lens, False) + planes(vs, S, lens, True))
    expv, psum, out = outputs(acc, d, H, hd)
    mc.KernelTask(acc.load("mc_b_attn_scores_f8_rows_bfloat"), (nsplit * 256, KV, B), (256, 1, 1),
                  [d["qb"], kq, kx, expv, psum, d["st"], *d["tail"], np.float32(scale), np.uint32(nsplit), *d["strides"]])()
    mc.KernelTask(acc.load("mc_b_attn_pv_f8_rows_bfloat"), (hd // 16 * 1024, KV, B), (1024, 1, 1),
                  [expv, psum, vq, vx, out, d["st"], *d["tail"], np.uint32(nsplit), *d["strides"]])()
    acc.wait()
    d["ref"] = download(expv, psum, out, B, H, S, nsplit, hd)
    _reference[key] = d
    return d


def outputs(acc, d, H, hd):
    return acc.to_device(d["sentinel"]), acc.to_device(np.zeros(d["B"] * H * d["nsplit"], np.float32)), acc.to_device(np.full(d["B"] * H * hd, NAN, np.uint16))


def download(expv, psum, out, B, H, S, nsplit, hd):
    return expv.download(np.float32, B * H * S).reshape(B, H * S), psum.download(np.float32, B * H * nsplit), out.download(np.uint16, B * H * hd).reshape(B, H, hd)


@pytest.mark.parametrize("GW", [1, 2, 4])
@pytest.mark.parametrize("S,H,KV,hd,shared,times", CASES)
def test_attached_rows_compute_the_per_row_f8_kernels_bits(acc, S, H, KV, hd, shared, times, GW):
    import metalchat_amd as mc

    d = reference(acc, S, H, KV, hd, shared, times)
    B, nsplit, n_rep, lens = d["B"], d["nsplit"], d["n_rep"], d["lens"]
    G = 16 // n_rep
    bufs = [(acc.to_device(guarded8(p.reshape(n, -1).view(np.uint8)).reshape(-1)), n, p[0].size) for p, n in [(p, B) for p in d["own"]] + [(p, 1) for p in d["prefix"]]]
    (kq, kx, vq, vx, pkq, pkx, pvq, pvx) = (b for b, _, _ in bufs)
    spl = acc.to_device(np.array([shared if a else 0 for a in d["attached"]], np.int32))
    expv, psum, out = outputs(acc, d, H, hd)
    mc.KernelTask(acc.load("mc_sp8_attn_scores_bfloat"), (nsplit * 256, KV, B + 1), (256, 1, 1),
                  [d["qb"], kq, kx, pkq, pkx, expv, psum, d["st"], spl, *d["tail"], np.float32(d["scale"]), np.uint32(nsplit), *d["strides"], np.uint32(B),
                   np.uint32(G), np.uint32(shared)])()
    groups = (B + G - 1) // G
    mc.KernelTask(acc.load("mc_sp8_attn_pv_bfloat"), (hd // 16 * 1024, KV, (groups + GW - 1) // GW), (1024, 1, 1),
                  [expv, psum, vq, vx, pvq, pvx, out, d["st"], spl, *d["tail"], np.uint32(nsplit), *d["strides"], np.uint32(B), np.uint32(G), np.uint32(GW),
                   np.uint32(shared)])()
    acc.wait()
    (got_e, got_p, got_o), (ref_e, ref_p, ref_o) = download(expv, psum, out, B, H, S, nsplit, hd), d["ref"]
    what = f"S{S} H{H} KV{KV} hd{hd} shared {shared} B{B} GW{GW}"
    parity.exact(got_e.view(np.uint32), ref_e.view(np.uint32), f"{what}: expv")
    parity.exact(got_p.view(np.uint32), ref_p.view(np.uint32), f"{what}: psum")
    parity.exact(got_o, ref_o, f"{what}: output")
    for r, n in enumerate(lens):
        if n < 0:
            parity.exact(got_o[r], np.zeros((H, hd), np.uint16), f"{what}: the idle row's output is +0.0")
            parity.exact(got_e[r], d["sentinel"][:H * S], f"{what}: the idle row's expv slice")
            continue
        parity.check(BF16, got_o[r], oracle_attention(d["q"][r], *d["deq"][r], n_rep, d["scale"]), rel=2e-3, max_ulp=1, max_frac=0.03, scale_aware=True,
                     what=f"{what} row {r} kv_len {n}")
    for buf, n, size in bufs:
        g = buf.download(np.uint8, n * (size + GUARD8)).reshape(n, -1)[:, size:]
        parity.exact(g, np.full(g.shape, 0x7F, np.uint8), f"{what}: the guards behind the planes")
