"""The fp8 KV cache kernels (metalchat_amd/csrc/kernels/kv8_kernels.hip; include/metalchat_hip.h Part 2o), each launched BY NAME through the
Part-1 seam as test_batch_kernels_gpu.py launches the bfloat16 ones.  The format is a storage format, so every check is bit for bit:
the write kernels against the rule (tests/kv_fp8_rule.py) applied to what the bfloat16 write kernels store, attention against the
bfloat16 attention kernels on a cache that holds deq of the same bytes (and against the float64 oracle of those values), the quantising
and dequantising copies against the rule.  Every plane of every row ends in a guard of NaN bytes (0x7f) that must survive."""
import numpy as np
import pytest

import kv_fp8_rule as kr
import parity
from test_attn_kernels_gpu import oracle_attention
from test_batch_kernels_gpu import BF16, GUARD, NAN, PB, ST_POS, bf, f, guarded, packed_partners, rope_table, state_at, states

pytestmark = pytest.mark.gpu
S = 192
G = 64                     # guard bytes behind each byte / exponent plane
SHAPES = [(8, 2, 128), (4, 4, 64)]


def guarded8(per_row):
    """[B, n] uint8 planes, each followed by G NaN bytes"""
    return np.concatenate([per_row, np.full((per_row.shape[0], G), 0x7F, np.uint8)], axis=1)


def task(acc, name, grid, block, args):
    import metalchat_amd as mc

    mc.KernelTask(acc.load(name), grid, block, args)()
    acc.wait()


# ------------------------------------------------------------------------------------------ the write kernels
@pytest.mark.parametrize("H,KV,hd", SHAPES)
def test_rope_kv_f8_writes_the_rule_of_the_bfloat16_write(acc, H, KV, hd):
    half, theta = hd // 2, 500000.0
    cb, sb, _, _ = rope_table(acc, S, hd, theta)
    positions = [0, 63, 64, S - 1, -1]            # -1: idle (rows form only)
    B = len(positions)
    rng = np.random.default_rng(hd)
    qn, kn, vn = (bf(rng.normal(0, 1, (B, n, hd)) * np.exp2(rng.integers(-6, 6, (B, n, 1)))) for n in (H, KV, KV))
    kn[0, 0] = vn[0, 0] = 0                       # a zero vector
    vn[1, 0] = bf(np.linspace(-1, 1, hd) * 2.0 ** -3)
    vn[1, 0, 3] = bf(np.array([-448.0 * 2.0 ** -3]))[0]   # amax on an exponent edge
    ties = np.array([17.0, -19.0, 1.0625, 0.001953125 * 1.5, 200.0, 2.0 ** -10, 400.0])   # midpoints of the e4m3 grid at e = 0
    vn[2, 1, :len(ties)] = bf(ties)
    vn[2, 1, hd - 1] = bf(np.array([448.0]))[0]
    qkv = np.concatenate([np.stack([packed_partners(x[r]) for r in range(B)]).reshape(B, -1) for x in (qn, kn)] + [vn.reshape(B, -1)], axis=1)
    cstride, xstride = KV * S * hd + G, KV * S + G
    init = [rng.integers(0, 256, (B, n), dtype=np.uint8) for n in (KV * S * hd, KV * S * hd, KV * S, KV * S)]

    def run(sfx, st, Bn):
        qb = acc.to_device(np.ascontiguousarray(qkv[:Bn]).reshape(-1))
        sbuf = acc.to_device(st.reshape(-1))
        tail = [np.uint32(H), np.uint32(KV), np.uint32(hd), np.uint32(S)]
        # the bfloat16 kernel on zeroed caches: what it stores is what the rule reads
        kb, vb = (acc.to_device(guarded(np.zeros((Bn, KV * S * hd), np.uint16), Bn)) for _ in range(2))
        q0 = acc.to_device(np.full(Bn * H * hd, NAN, np.uint16))
        task(acc, "mc_b_rope_kv" + sfx, ((H + 2 * KV) * half, Bn, 1), (half, 1, 1), [qb, q0, kb, vb, cb, sb, sbuf] + tail + [np.uint64(KV * S * hd + GUARD)])
        kc = kb.download(np.uint16, Bn * (KV * S * hd + GUARD)).reshape(Bn, -1)[:, :KV * S * hd].reshape(Bn, KV, S, hd)
        vt = vb.download(np.uint16, Bn * (KV * S * hd + GUARD)).reshape(Bn, -1)[:, :KV * S * hd].reshape(Bn, KV, hd, S)
        bufs = [acc.to_device(guarded8(p[:Bn]).reshape(-1)) for p in init]
        q1 = acc.to_device(np.full(Bn * H * hd, NAN, np.uint16))
        task(acc, "mc_b_rope_kv_f8" + sfx, ((H + 2 * KV) * half, Bn, 1), (half, 1, 1),
             [qb, q1] + bufs + [cb, sb, sbuf] + tail + [np.uint64(cstride), np.uint64(xstride)])
        got = [b.download(np.uint8, Bn * (p.shape[1] + G)).reshape(Bn, -1) for b, p in zip(bufs, init)]
        return q0.download(np.uint16, Bn * H * hd), q1.download(np.uint16, Bn * H * hd), kc, vt, got

    def check(sfx, st, pos_of_row):
        Bn = len(pos_of_row)
        q0, q1, kc, vt, got = run(sfx, st, Bn)
        parity.exact(q1, q0, f"{sfx}: q is the bfloat16 kernel's")
        exp = [guarded8(p[:Bn]) for p in init]
        for r, pos in enumerate(pos_of_row):
            if pos < 0:
                continue
            kbytes, ke = kr.quant(kc[r, :, pos])                      # [KV, hd], [KV]
            vbytes, ve = kr.quant(vt[r, :, :, pos])
            exp[0][r, :KV * S * hd].reshape(KV, S, hd)[:, pos] = kbytes
            exp[1][r, :KV * S * hd].reshape(KV, hd, S)[:, :, pos] = vbytes
            exp[2][r, :KV * S].reshape(KV, S)[:, pos] = ke.view(np.uint8)
            exp[3][r, :KV * S].reshape(KV, S)[:, pos] = ve.view(np.uint8)
        for g, e, name in zip(got, exp, ("K bytes", "V bytes", "kexp", "vexp")):
            parity.exact(g, e, f"{sfx} {pos_of_row}: {name} (the written slot, nothing else, the guards)")

    for pos in (0, 63, 64, S - 1):
        check("_bfloat", state_at(pos + 1), [pos] * (B - 1))
    rows = states(B)
    for r, pos in enumerate(positions):
        rows[r] = state_at(pos + 1) if pos >= 0 else rows[r]
        rows[r, ST_POS] = pos
    check("_rows_bfloat", rows, positions)


# ------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("H,KV,hd", SHAPES)
def test_attention_f8_is_the_bfloat16_attention_on_deq(acc, H, KV, hd, ragged):
    nsplit, n_rep = (S + PB - 1) // PB, H // KV
    scale = float(f(bf(np.array([hd ** -0.5])))[0])
    sfx = "_rows_bfloat" if ragged else "_bfloat"
    lens_all = [1, 63, 64, 65, S - 1, S]
    runs = [lens_all + [-1]] if ragged else [[n, n] for n in lens_all]
    for i, lens in enumerate(runs):
        B = len(lens)
        rng = np.random.default_rng(1000 * hd + 10 * i + ragged)
        q = bf(rng.normal(0, 1, (B, H, hd)))
        # slots past a row's kv_len: NaN bytes under random exponents in the fp8 planes, finite garbage in the bfloat16 caches
        kq, vq = (np.full((B, KV, S, hd), 0x7F, np.uint8), np.full((B, KV, hd, S), 0x7F, np.uint8))
        kx, vx = (rng.integers(-128, 128, (B, KV, S), dtype=np.int8) for _ in range(2))
        kc, vt = bf(rng.normal(0, 30, (B, KV, S, hd))), bf(rng.normal(0, 30, (B, KV, hd, S)))
        kd, vd = [], []
        for r, n in enumerate(lens):
            n = max(n, 0)
            k = bf(rng.normal(0, 0.4, (n, KV, hd)) * np.exp2(rng.integers(-3, 3, (n, KV, 1))))
            v = bf(rng.normal(0, 0.5, (n, KV, hd)) * np.exp2(rng.integers(-3, 3, (n, KV, 1))))
            (kb, ke), (vb, ve) = kr.quant(k), kr.quant(v)
            kq[r, :, :n], kx[r, :, :n] = kb.transpose(1, 0, 2), ke.T
            vq[r, :, :, :n], vx[r, :, :n] = vb.transpose(1, 2, 0), ve.T
            kd.append(kr.deq(kb, ke))
            vd.append(kr.deq(vb, ve))
            kc[r, :, :n], vt[r, :, :, :n] = kd[r].transpose(1, 0, 2), vd[r].transpose(1, 2, 0)
        if ragged:
            st = states(B)
            for r, n in enumerate(lens):
                if n > 0:
                    st[r] = state_at(n)
                st[r, ST_POS] = n - 1 if n > 0 else -1
        else:
            st = state_at(lens[0])
        qb, sb = acc.to_device(q.reshape(-1)), acc.to_device(st.reshape(-1))
        outs = []
        for fp8 in (False, True):
            expv, psum = acc.to_device(np.full(B * H * S, -7.0, np.float32)), acc.to_device(np.zeros(B * H * nsplit, np.float32))
            out = acc.to_device(np.full(B * H * hd, NAN, np.uint16))
            if fp8:
                kb_, vb_, kxb, vxb = (acc.to_device(guarded8(p.reshape(B, -1).view(np.uint8)).reshape(-1)) for p in (kq, vq, kx, vx))
                strides = [np.uint64(KV * S * hd + G), np.uint64(KV * S + G)]
                kargs, vargs, name = [kb_, kxb], [vb_, vxb], "_f8" + sfx
            else:
                kb_, vb_ = acc.to_device(guarded(kc, B)), acc.to_device(guarded(vt, B))
                strides = [np.uint64(KV * S * hd + GUARD)]
                kargs, vargs, name = [kb_], [vb_], sfx
            tail = [np.uint32(n_rep), np.uint32(hd), np.uint32(S)]
            task(acc, "mc_b_attn_scores" + name, (nsplit * 256, KV, B), (256, 1, 1),
                 [qb] + kargs + [expv, psum, sb] + tail + [np.float32(scale), np.uint32(nsplit)] + strides)
            task(acc, "mc_b_attn_pv" + name, (hd // 16 * 1024, KV, B), (1024, 1, 1), [expv, psum] + vargs + [out, sb] + tail + [np.uint32(nsplit)] + strides)
            outs.append(out.download(np.uint16, B * H * hd).reshape(B, H, hd))
        ref, got = outs
        for r, n in enumerate(lens):
            what = f"{'rows' if ragged else 'lockstep'} hd{hd} row {r} kv_len {n}"
            if n < 0:
                parity.exact(got[r], np.zeros((H, hd), np.uint16), f"{what}: the idle row's output is +0.0")
                continue
            parity.exact(got[r], ref[r], f"{what}: against the bfloat16 kernels on deq")
            parity.check(BF16, got[r], oracle_attention(q[r], kd[r], vd[r], n_rep, scale), rel=2e-3, max_ulp=1, max_frac=0.03, scale_aware=True, what=what)


# ------------------------------------------------------------------------------------------ the quantising and dequantising copies
@pytest.mark.parametrize("n", [1, 63, 65, S])
@pytest.mark.parametrize("H,KV,hd", SHAPES)
def test_kv_quant_and_dequant_f8(acc, H, KV, hd, n):
    rng = np.random.default_rng(n + hd)
    k = bf(rng.normal(0, 1, (KV, n, hd)) * np.exp2(rng.integers(-8, 8, (KV, n, 1))))       # K [kv][n][hd]
    v = bf(rng.normal(0, 1, (KV, n, hd)) * np.exp2(rng.integers(-8, 8, (KV, n, 1))))
    k[0, 0] = 0
    init = [rng.integers(0, 256, (1, m), dtype=np.uint8) for m in (KV * S * hd, KV * S * hd, KV * S, KV * S)]
    bufs = [acc.to_device(guarded8(p).reshape(-1)) for p in init]
    vt_src = np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(-1)                         # Vt [kv * hd][n]
    task(acc, "mc_kv_quant_f8", ((n + 63) // 64 * 256, KV, 1), (256, 1, 1),
         [acc.to_device(k.reshape(-1)), acc.to_device(vt_src), np.uint32(n)] + bufs + [np.uint32(n), np.uint32(hd), np.uint32(S)])
    (kb, ke), (vb, ve) = kr.quant(k), kr.quant(v)
    exp = [guarded8(p) for p in init]
    exp[0][0, :KV * S * hd].reshape(KV, S, hd)[:, :n] = kb
    exp[1][0, :KV * S * hd].reshape(KV, hd, S)[:, :, :n] = vb.transpose(0, 2, 1)
    exp[2][0, :KV * S].reshape(KV, S)[:, :n] = ke.view(np.uint8)
    exp[3][0, :KV * S].reshape(KV, S)[:, :n] = ve.view(np.uint8)
    for b, e, name in zip(bufs, exp, ("K bytes", "V bytes", "kexp", "vexp")):
        parity.exact(b.download(np.uint8, e.size), e.reshape(-1), f"quant n {n}: {name}")
    st = np.zeros(12, np.int32)
    st[2] = n                                                                               # kv_len; the ring has not turned
    ko, vo = (acc.to_device(np.full(n * KV * hd, NAN, np.uint16)) for _ in range(2))
    task(acc, "mc_kv_dequant_f8", (512 * 256, 1, 1), (256, 1, 1), bufs + [ko, vo, acc.to_device(st), np.uint32(KV), np.uint32(hd), np.uint32(S), np.uint32(4)])
    parity.exact(ko.download(np.uint16, n * KV * hd).reshape(n, KV, hd), kr.roundtrip(k).transpose(1, 0, 2), f"dequant n {n}: K is deq(quant(K))")
    parity.exact(vo.download(np.uint16, n * KV * hd).reshape(n, KV, hd), kr.roundtrip(v).transpose(1, 0, 2), f"dequant n {n}: V is deq(quant(V))")
