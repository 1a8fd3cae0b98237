"""The shared-prefix attention kernels (prefix_kernels.hip, Part 2r) by name: six rows in one launch -- four attached at kv_len shared + 1, + 32,
+ 33, + 65, an ordinary row between them, an idle row -- against the per-row kernels on planes that hold a copy of the prefix, bit for bit, and
against the float64 oracle within test_b_attention_per_row's bounds.  An attached row's own slots [0, shared) hold garbage that must not matter."""
import numpy as np
import pytest

import parity
from test_attn_kernels_gpu import oracle_attention
from test_batch_kernels_gpu import BF16, GUARD, NAN, PB, ST_POS, attn_rows, bf, f, guarded, state_at, states

pytestmark = pytest.mark.gpu
# S, H, KV, hd: n_rep 4 with a second round of k-steps; n_rep 8; G = 1 and the clamped V load at max_seq - 8; n_rep 3 (G n_rep = 15 < 16)
SHAPES = [(2240, 32, 8, 128), (1000, 32, 4, 64), (104, 16, 1, 128), (256, 6, 2, 64)]
CASES = [(*s, sh) for s in SHAPES for sh in sorted({64, (s[0] - 2) // 64 * 64})]


@pytest.mark.parametrize("S,H,KV,hd,shared", CASES)
def test_attached_rows_compute_the_per_row_kernels_bits(acc, S, H, KV, hd, shared):
    import metalchat_amd as mc

    nsplit, n_rep = (S + PB - 1) // PB, H // KV
    G = 16 // n_rep
    scale = float(f(bf(np.array([hd ** -0.5])))[0])
    cstride = KV * S * hd + GUARD
    att = [min(S, shared + d) for d in (1, 32, 33, 65)]
    lens = [att[0], att[1], min(S, 70), att[2], att[3], -1]
    attached = [True, True, False, True, True, False]
    B = len(lens)
    rng = np.random.default_rng(S + shared)
    q, kc, vt, ks, vs = attn_rows(S, H, KV, hd, lens, seed=S + shared + 1)
    pk, pv = bf(rng.normal(0, 0.4, (shared, KV, hd))), bf(rng.normal(0, 0.5, (shared, KV, hd)))
    pkc, pvt = bf(rng.normal(0, 30, (1, KV, S, hd))), bf(rng.normal(0, 30, (1, KV, hd, S)))   # the prefix planes: garbage behind `shared`
    pkc[0, :, :shared], pvt[0, :, :, :shared] = pk.transpose(1, 0, 2), pv.transpose(1, 2, 0)
    kc_own, vt_own = kc.copy(), vt.copy()
    for r in range(B):
        if attached[r]:
            kc[r, :, :shared], vt[r, :, :, :shared] = pkc[0, :, :shared], pvt[0, :, :, :shared]   # the reference: a full copy
            ks[r][:shared], vs[r][:shared] = pk, pv
            kc_own[r, :, :shared] = bf(rng.normal(0, 30, (KV, shared, hd)))                        # under test: never read
            vt_own[r, :, :, :shared] = bf(rng.normal(0, 30, (KV, hd, shared)))
    st = states(B)
    for r, n in enumerate(lens):
        if n > 0:
            st[r] = state_at(n)
        st[r, ST_POS] = n - 1 if n > 0 else -1
    sb = acc.to_device(st.reshape(-1))
    qb = acc.to_device(q.reshape(-1))
    sentinel = np.full(B * H * S, -7.0, np.float32)

    def run(sp):
        kb, vb = acc.to_device(guarded(kc_own if sp else kc, B)), acc.to_device(guarded(vt_own if sp else vt, B))
        expv, psum = acc.to_device(sentinel), acc.to_device(np.zeros(B * H * nsplit, np.float32))
        out = acc.to_device(np.full(B * H * hd, NAN, np.uint16))
        tail = [np.uint32(n_rep), np.uint32(hd), np.uint32(S)]
        bufs = [(kb, B), (vb, B)]
        if sp:
            pkb, pvb = acc.to_device(guarded(pkc, 1)), acc.to_device(guarded(pvt, 1))
            spl = acc.to_device(np.array([shared if a else 0 for a in attached], np.int32))
            bufs += [(pkb, 1), (pvb, 1)]
            mc.KernelTask(acc.load("mc_sp_attn_scores_bfloat"), (nsplit * 256, KV, B + 1), (256, 1, 1),
                          [qb, kb, pkb, expv, psum, sb, spl, *tail, np.float32(scale), np.uint32(nsplit), np.uint64(cstride), np.uint32(B), np.uint32(G),
                           np.uint32(shared)])()
            mc.KernelTask(acc.load("mc_sp_attn_pv_bfloat"), (hd // 16 * 1024, KV, (B + G - 1) // G), (1024, 1, 1),
                          [expv, psum, vb, pvb, out, sb, spl, *tail, np.uint32(nsplit), np.uint64(cstride), np.uint32(B), np.uint32(G)])()
        else:
            mc.KernelTask(acc.load("mc_b_attn_scores_rows_bfloat"), (nsplit * 256, KV, B), (256, 1, 1),
                          [qb, kb, expv, psum, sb, *tail, np.float32(scale), np.uint32(nsplit), np.uint64(cstride)])()
            mc.KernelTask(acc.load("mc_b_attn_pv_rows_bfloat"), (hd // 16 * 1024, KV, B), (1024, 1, 1),
                          [expv, psum, vb, out, sb, *tail, np.uint32(nsplit), np.uint64(cstride)])()
        acc.wait()
        guards = [buf.download(np.uint16, n * cstride).reshape(n, cstride)[:, -GUARD:] for buf, n in bufs]
        return (expv.download(np.float32, B * H * S).reshape(B, H * S), psum.download(np.float32, B * H * nsplit),
                out.download(np.uint16, B * H * hd).reshape(B, H, hd), guards)

    ref_e, ref_p, ref_o, _ = run(False)
    got_e, got_p, got_o, guards = run(True)
    what = f"S{S} H{H} KV{KV} hd{hd} shared {shared}"
    parity.exact(got_e.view(np.uint32), ref_e.view(np.uint32), f"{what}: expv")
    parity.exact(got_p.view(np.uint32), ref_p.view(np.uint32), f"{what}: psum")
    parity.exact(got_o, ref_o, f"{what}: output")
    for r, n in enumerate(lens):
        if n < 0:
            parity.exact(got_o[r], np.zeros((H, hd), np.uint16), f"{what}: the idle row's output is +0.0")
            parity.exact(got_e[r], sentinel[:H * S], f"{what}: the idle row's expv slice")
            continue
        parity.check(BF16, got_o[r], oracle_attention(q[r], ks[r], vs[r], n_rep, scale), rel=2e-3, max_ulp=1, max_frac=0.03, scale_aware=True,
                     what=f"{what} row {r} kv_len {n}")
    for g in guards:
        parity.exact(g, np.full(g.shape, NAN, np.uint16), f"{what}: the guards behind the planes")
