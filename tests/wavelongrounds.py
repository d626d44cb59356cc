"""The launch shape and the data flow of ONE workgroup of the tempering rounds of long chains inside a wave launch
(csrc/nlmc_wave_long_rounds.h: k_rounds_waves_long; csrc/nlmc_wave_shape.h: nlmc_wave_long_rounds_shape) restated in Python / NumPy on
the functions of tests/wavefields.py and tests/waverounds.py.  P whole ladders = Q = P L chains on W waves, wave w owning chains w,
w + W, .. below Q and running them in turn within a round; every chain has a region of its own with a copy of its fields X and its
spins, the fields built ONCE per chain (the prologue) and from then on only corrected, every correction written through to the
region, so that a wave parks nothing between its turns and starts a turn by reading the chain's fields back; the energies left in an
array for the swap round; lane t of wave 0 deciding pair t mod n_pairs of ladder t // n_pairs; chains that never move while two byte
maps exchange entries.  It shares with the oracle only leaf functions, so tests/test_wave_long_rounds_cpu.py can hold it against the
oracle double round by round without a GPU.  No test in here."""
import numpy as np

import oracle
import wavefields
import waverounds
from oracle import pt as opt

LDS_MAX = 158 * 1024


def up16(x):
    return (x + 15) // 16 * 16


def layout(n, n_pad, Q, W):
    """nlmc_wave_long_rounds_layout: per chain X [64 R] int32 | spins [n_pad], per wave thresholds [4 ceil(n / 4)] float, energies [Q]
    int64, maps 2 Q bytes; each part 16-byte aligned."""
    g = {"s_off": 256 * (8 if n <= 512 else 16)}
    g["chain_bytes"] = g["s_off"] + up16(n_pad)
    g["w_bytes"] = 16 * ((n + 3) // 4)
    g["w_off"] = Q * g["chain_bytes"]
    g["e_off"] = g["w_off"] + W * g["w_bytes"]
    g["map_off"] = g["e_off"] + up16(8 * Q)
    g["total"] = g["map_off"] + up16(2 * Q)
    return g


def waves_of(Q):
    C = (Q + 15) // 16
    return C, (Q + C - 1) // C


def launch_shape(n, n_pad, L, ladders, n_cu, knob=0):
    """nlmc_wave_long_rounds_shape -> dict(R, P, C, W, blocks, lds), or None where the library refuses.  The rule: the compute units
    first, then as many ladders as fit 16 waves with a chain each (the knob: up to 64 chains), then as many as the LDS holds."""
    if not (257 <= n <= 1024) or n_pad < n or not (1 <= L <= 64) or ladders < 1:
        return None
    R = 8 if n <= 512 else 16
    if n_pad > 64 * R:
        return None
    cu = n_cu if n_cu > 0 else 1
    p = knob if knob > 0 else (ladders + cu - 1) // cu
    cap = 64 // L if knob > 0 else max(16 // L, 1)
    p = max(1, min(p, cap, ladders))
    while True:
        C, W = waves_of(p * L)
        total = layout(n, n_pad, p * L, W)["total"]
        if total <= LDS_MAX:
            return {"R": R, "P": p, "C": C, "W": W, "blocks": (ladders + p - 1) // p, "lds": total}
        if p == 1:
            return None
        p -= 1


def workgroup_rounds(J, h, spins, slots, efix, betas, L, P, ladder0, chain0, n_rounds, T, n_pairs, seed, sweep0=0, round0=0):
    """Generator: the state of the workgroup's Q = P L chains after every round -> (spins [Q, n] int8, slot_of_chain [Q], efix [Q]
    int64, pairs [P, n_pairs, 2], acc [P, n_pairs], field rebuilds so far).  spins / slots / efix: of the workgroup's chains at the
    start; ladder0 / chain0: global index of its first ladder / chain (Philox keys)."""
    Q = P * L
    C, W = waves_of(Q)
    assert Q <= 64 and W <= 16
    csr = oracle.Csr(J)
    qs, es = oracle.field_scale(csr, h)
    Jd, hq = wavefields.dense_matrix(J, h, qs)
    n = Jd.shape[0]
    inv = 2.0 ** -es
    soc = np.asarray(slots, dtype=np.uint8).copy()             # the two maps, bytes
    cos = np.zeros(Q, dtype=np.uint8)
    for ch in range(Q):
        cos[ch // L * L + soc[ch]] = ch
    owned = [[w + t * W for t in range(C) if w + t * W < Q] for w in range(W)]
    assert sorted(ch for o in owned for ch in o) == list(range(Q))
    lds_X, lds_s = np.zeros((Q, n), dtype=np.int64), np.zeros((Q, n), dtype=np.int64)       # the chains' regions
    el = np.asarray(efix, dtype=np.int64).copy()               # the energy array of the swap round
    builds = 0
    # prologue: once per chain and launch, by the wave that owns the chain
    for w in range(W):
        for ch in owned[w]:
            lds_s[ch] = spins[ch]
            X = hq.copy()
            for i in range(n):
                X += Jd[i] * lds_s[ch, i]
            lds_X[ch] = X
            builds += 1
    # ---- barrier
    for r in range(n_rounds):
        for w in range(W):
            for ch in owned[w]:                                # chains in turn: the wave's registers take the chain's fields from its region
                reg_X = lds_X[ch].copy()
                slot = int(soc[ch])
                cb = oracle.cb_pair(betas[slot])[0]
                for t in range(T):
                    # (the sweep corrects the registers and writes every correction through: reg_X and the region stay equal)
                    el[ch] += waverounds.sweep_resident(Jd, qs, es - qs, lds_s[ch], reg_X, cb, (sweep0 + r * T + t) & 0xFFFFFFFF, chain0 + ch, seed)
                    lds_X[ch] = reg_X
        # ---- barrier: wave 0 decides, one lane per pair, on the maps and energies of before the round's swaps
        lo, hi = int(seed) & 0xFFFFFFFF, int(seed) >> 32
        rnd = (round0 + r) & 0xFFFFFFFF
        pairs, acc = np.zeros((P, n_pairs, 2), dtype=np.int32), np.zeros((P, n_pairs), dtype=np.uint8)
        assert P * n_pairs < 64
        reads = []
        for lane in range(P * n_pairs):                        # every lane reads ...
            lw, p = lane // n_pairs, lane % n_pairs
            i = waverounds.planned_pairs(L, n_pairs, rnd, ladder0 + lw, seed)[p]
            ca, cb_ = int(cos[lw * L + i]), int(cos[lw * L + i + 1])
            reads.append((lw, p, i, ca, cb_, float(el[ca]) * inv, float(el[cb_]) * inv))
        for lw, p, i, ca, cb_, Ea, Eb in reads:                # ... before any lane writes (selected pairs are disjoint)
            wd = oracle.philox(p, rnd, ladder0 + lw, opt.TAG_SWAP, lo, hi)
            u = ((int(wd[0]) >> 5) * 67108864.0 + (int(wd[1]) >> 6)) / 9007199254740992.0
            z = ((betas[i + 1] - betas[i]) * (Eb - Ea)) * opt.LOG2E
            ok = u < opt.lib().nlo_exp2_f64(z)
            if ok:
                cos[lw * L + i], cos[lw * L + i + 1] = cb_, ca
                soc[ca], soc[cb_] = i + 1, i
            pairs[lw, p], acc[lw, p] = (i, i + 1), int(ok)
        # ---- barrier
        yield lds_s.astype(np.int8), soc.astype(np.int32), el.copy(), pairs, acc, builds
