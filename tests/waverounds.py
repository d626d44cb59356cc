"""The data flow of ONE workgroup of the tempering rounds inside a wave launch (csrc/nlmc_wave_rounds.h: k_rounds_waves) restated in
NumPy on the functions of tests/wavefields.py: P whole ladders = Q = P L chains on W waves, wave w owning chains w, w + W, .. below Q
and running them in turn within a round; the fields X built ONCE per chain (the prologue) and from then on only corrected, parked
next to the spins between a wave's turns; the energies left in an array for the swap round; lane t of wave 0 deciding pair t mod
n_pairs of ladder t // n_pairs; chains that never move while two byte maps, chain_of_slot[ladder][slot] and slot_of_chain[chain],
exchange entries.  It shares with the oracle only leaf functions (oracle.philox, oracle.threshold, oracle.field_scale, oracle.cb_pair,
the exp2 of the acceptance test), so tests/test_wave_rounds_cpu.py can hold it against the oracle double round by round without a
GPU.  No test in here."""
import numpy as np

import oracle
import wavefields
from oracle import pt as opt


def launch_shape(L, P):
    """(Q, C, W) of a workgroup of P ladders: csrc/nlmc_wave_shape.h, nlmc_wave_rounds_shape."""
    Q = P * L
    assert 1 <= Q <= 64
    C = (Q + 15) // 16
    W = (Q + C - 1) // C
    assert W <= 16
    return Q, C, W


def planned_pairs(L, n_pairs, rnd, ladder, seed):
    """The lower slots of the n_pairs disjoint pairs of `ladder` (global index) in round rnd: the selection nlmc_pt_plan makes."""
    lo, hi = int(seed) & 0xFFFFFFFF, int(seed) >> 32
    avail, sel = list(range(L - 1)), []
    for p in range(n_pairs):
        r = int(oracle.philox(p, rnd, ladder, opt.TAG_PAIR, lo, hi)[0])
        i = avail[(r * len(avail)) >> 32]
        sel.append(i)
        avail = [q for q in avail if abs(q - i) > 1]
    return sel


def sweep_resident(Jd, qs, eshift, s, X, cb, tt, chain_id, seed):
    """One sweep of one chain on resident fields, in place: wavefields.sweeps' loop body without its prologue.  -> energy delta."""
    n = Jd.shape[0]
    lo, hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    Wt = np.empty(4 * ((n + 3) // 4), dtype=np.float32)        # lane l makes the Philox call of block l
    for b in range((n + 3) // 4):
        r = oracle.philox(b, tt, chain_id, wavefields.TAG_UNIFORM, lo, hi)
        Wt[4 * b:4 * b + 4] = [oracle.threshold(int(r[q])) for q in range(4)]
    cbq = np.float32(np.ldexp(np.float32(cb), -qs))
    dE = 0
    for k in wavefields.visiting_order(n, tt, 0, seed):
        z = np.float32(cbq * np.float32(int(X[k])))
        so, sn = int(s[k]), (1 if z < Wt[k] else -1)
        if sn != so:
            dE += (int(X[k]) - int(Jd[k, k]) * so) * ((so - sn) << eshift)
            s[k] = sn
            X += (sn - so) * Jd[k]
            assert np.all(np.abs(X) < 2 ** 31)
    return dE


def workgroup_rounds(J, h, spins, slots, efix, betas, L, P, ladder0, chain0, n_rounds, T, n_pairs, seed, sweep0=0, round0=0):
    """Generator: the state of the workgroup's Q = P L chains after every round -> (spins [Q, n] int8, slot_of_chain [Q], efix [Q]
    int64, pairs [P, n_pairs, 2], acc [P, n_pairs]).  spins / slots / efix: of the workgroup's chains at the start; ladder0 / chain0:
    global index of its first ladder / chain (Philox keys)."""
    Q, C, W = launch_shape(L, P)
    csr = oracle.Csr(J)
    qs, es = oracle.field_scale(csr, h)
    Jd, hq = wavefields.dense_matrix(J, h, qs)
    n = Jd.shape[0]
    inv = 2.0 ** -es
    # the two maps, bytes
    soc = np.asarray(slots, dtype=np.uint8).copy()
    cos = np.zeros(Q, dtype=np.uint8)
    for ch in range(Q):
        cos[ch // L * L + soc[ch]] = ch
    owned = [[w + t * W for t in range(C) if w + t * W < Q] for w in range(W)]
    assert sorted(ch for o in owned for ch in o) == list(range(Q))
    park_X, park_s = np.zeros((Q, n), dtype=np.int64), np.zeros((Q, n), dtype=np.int8)      # the LDS region of waves with several chains
    reg_X, reg_s = [None] * W, [None] * W                                                  # what a wave's registers hold
    el = np.asarray(efix, dtype=np.int64).copy()                                           # the energy array of the swap round
    # prologue: once per chain and launch
    for w in range(W):
        for ch in owned[w]:
            s = np.asarray(spins[ch], dtype=np.int64).copy()
            X = hq.copy()
            for i in range(n):
                X += Jd[i] * s[i]
            reg_X[w], reg_s[w] = X, s
            if len(owned[w]) > 1:
                park_X[ch], park_s[ch] = X, s
    for r in range(n_rounds):
        for w in range(W):
            for ch in owned[w]:                                # chains in turn
                if len(owned[w]) > 1:
                    reg_X[w], reg_s[w] = park_X[ch].copy(), park_s[ch].astype(np.int64)
                slot = int(soc[ch])
                cb = oracle.cb_pair(betas[slot])[0]
                for t in range(T):
                    el[ch] += sweep_resident(Jd, qs, es - qs, reg_s[w], reg_X[w], cb, (sweep0 + r * T + t) & 0xFFFFFFFF, chain0 + ch, seed)
                if len(owned[w]) > 1:
                    park_X[ch], park_s[ch] = reg_X[w], reg_s[w]
        # ---- barrier: wave 0 decides, one lane per pair, on the maps and energies of before the round's swaps
        lo, hi = int(seed) & 0xFFFFFFFF, int(seed) >> 32
        rnd = (round0 + r) & 0xFFFFFFFF
        pairs, acc = np.zeros((P, n_pairs, 2), dtype=np.int32), np.zeros((P, n_pairs), dtype=np.uint8)
        assert P * n_pairs < Q
        reads = []
        for lane in range(P * n_pairs):                        # every lane reads ...
            lw, p = lane // n_pairs, lane % n_pairs
            i = planned_pairs(L, n_pairs, rnd, ladder0 + lw, seed)[p]
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
        out_s = np.stack([(park_s[ch] if len(owned[ch % W]) > 1 else reg_s[ch % W]).astype(np.int8) for ch in range(Q)])
        yield out_s, soc.astype(np.int32), el.copy(), pairs, acc
