"""A context of M K ladders as M independent APT systems (include/nlmc.h: nlmc_apt_systems), restated on the oracle.

The one definition: system s owns ladders s K .. s K + K - 1 (chains s K L .. (s + 1) K L - 1).  Per system s and slot r the K ladders of
that system are ordered by the keys philox(j, round, r, ICM_PAIR), j the GLOBAL ladder id, ties to the smaller j; ranks 2 i and 2 i + 1
form pair i, an odd K leaves the last rank out; pairs and info rows come in the order (system, slot, i).  The pick of a pair is keyed by
the two global chain ids.  The move changes the tracked energies by the exact integer deltas of the engine's fixed-point model (what the
kernels do; OracleEngine recomputes them from the true couplings, which is the same number on dyadic instances only).  Everything else is
OracleEngine's."""
import numpy as np

import oracle
from oracle import pt as opt
from fake_engine import OracleEngine

TAG_ICM_PAIR = 6


def n_pairs_of(L):
    return max(1, L // 3)                # greedy selection never runs out: a pick removes at most 3 of the L - 1 pairs


class SystemsOracleEngine(OracleEngine):
    n_systems = 1

    def pt_init(self, betas):
        super().pt_init(betas)
        self.n_systems = 1

    def set_spins(self, s, efix=None):
        """efix: the tracked start energies in units of 2^-escale where the caller has the engine's own (its fp64 sum of a start
        energy may differ from the oracle's in the last bit; every later change is an exact integer)."""
        super().set_spins(s)
        if efix is not None:
            self.efix = np.asarray(efix, np.int64).reshape(self.n_chains).copy()

    def apt_systems(self, n_systems):
        if not hasattr(self, "L"):
            raise RuntimeError("apt_systems: pt_init first")
        if n_systems < 1 or (self.G // self.L) % n_systems != 0:
            raise ValueError("apt_systems: n_systems must divide the number of ladders")
        if n_systems > 1 and self.rng_stride:
            raise NotImplementedError("apt_systems: slot-keyed random numbers know one system")
        self.n_systems = int(n_systems)

    def apt_shard(self, beta_global, world, rank):
        if self.n_systems > 1:
            raise NotImplementedError("apt_shard: the context is divided into several systems")
        super().apt_shard(beta_global, world, rank)

    def pairing(self, rnd, seed):
        """[(system, slot, i, chain a, chain b)] in the order of the info rows, from the current slot maps."""
        lo, hi = int(seed) & 0xFFFFFFFF, int(seed) >> 32
        L, M = self.L, self.n_systems
        K, cos = self.n_chains // L // M, self._chain_of_slot()
        out = []
        for s in range(M):
            for r in range(L):
                lad = range(s * K, (s + 1) * K)
                key = {j: int(oracle.philox(j, rnd, r, TAG_ICM_PAIR, lo, hi)[0]) for j in lad}
                sh = sorted(lad, key=lambda j: (key[j], j))
                for i in range(K // 2):
                    out.append((s, r, i, int(cos[sh[2 * i] * L + r]), int(cos[sh[2 * i + 1] * L + r])))
        return out

    def icm_round_ladders(self, rnd, seed, katzgraber=True, want_info=False):
        if self.n_systems == 1 and self.rng_stride:
            return super().icm_round_ladders(rnd, seed, katzgraber, want_info)
        lo, hi = int(seed) & 0xFFFFFFFF, int(seed) >> 32
        info = []
        for (_, _, _, a, b) in self.pairing(rnd, seed):
            cl = oracle.clusters(self.csr, self.spins[a], self.spins[b])
            if not cl:
                info.append((0, 0))
                continue
            pick = (int(oracle.philox(self.chain_base + a, rnd, self.chain_base + b, opt.TAG_ICM, lo, hi)[0]) * len(cl)) >> 32
            members = cl[pick]
            info.append((len(cl), len(members)))
            Jq, hq, shift = self._fixed_point()
            if katzgraber and len(members) > self.n // 2:
                self.efix[a] += (2 * int(hq @ self.spins[a].astype(np.int64))) << shift        # the field term changes sign
                self.spins[a] = -self.spins[a]
            else:
                sa, sb = self.spins[a].astype(np.int64), self.spins[b].astype(np.int64)
                out = np.ones(self.n, bool)
                out[members] = False                           # only bonds that leave the cluster count (the diagonal stays inside)
                for c, s in ((a, sa), (b, sb)):
                    f = hq[members] + Jq[members][:, out] @ s[out]
                    self.efix[c] += (2 * int(s[members] @ f)) << shift
                self.spins[a, members], self.spins[b, members] = sb[members].astype(np.int8), sa[members].astype(np.int8)
        return np.array(info, np.int32).reshape(-1, 2) if want_info else None

    def _fixed_point(self):
        """(Jq [n, n], hq [n], escale - qs): the integers of the engine's fixed-point model, Jq = rint(J 2^qs), hq = rint(h 2^qs)
        (oracle/nlo.c: nlo_field_scale).  The Houdayer step moves the tracked energies by exact deltas of THIS model in both
        precisions (csrc/nlmc_pt_icm.h: k_icm_round), so the helper does too: the swap round reads them."""
        if not hasattr(self, "_fp"):
            qs = oracle.field_scale(self.csr, self.h)[0]
            Jq = np.zeros((self.n, self.n), np.int64)
            rows = np.repeat(np.arange(self.n), np.diff(self.csr.indptr))
            Jq[rows, self.csr.indices] = np.rint(np.ldexp(np.asarray(self.csr.data, np.float64), qs)).astype(np.int64)
            hq = np.rint(np.ldexp(np.asarray(self.h, np.float64).reshape(-1), qs)).astype(np.int64)
            self._fp = (Jq, hq, self.esc - qs)
        return self._fp


def oracle_rounds(inst, M, K, L, T, rounds, precision, betas, m0, seed, pairs, katz=True, efix0=None):
    """The run of the GPU cases on the helper: rounds of T sweeps + Houdayer step + swap round from the state m0.
    -> dict(spins, efix, energy, slots, info [rounds, M L (K // 2), 2], pairs, acc)."""
    G = M * K * L
    o = SystemsOracleEngine(inst, G, 0, G)
    o.pt_init(betas)
    o.apt_systems(M)
    o.set_spins(m0, efix0)
    infos, lp, la = [], [], []
    for r in range(rounds):
        o.sweep_philox(T, seed, sweep0=r * T, precision=precision)
        infos.append(o.icm_round_ladders(r, seed, katz, want_info=True))
        if pairs > 0:
            p, a = o.pt_swap_philox(r, seed, pairs)
            lp.append(np.asarray(p).reshape(M * K, pairs, 2))
            la.append(np.asarray(a).reshape(M * K, pairs))
    NP = M * L * (K // 2)
    return {"spins": o.get_spins(), "efix": o.efix.copy(), "energy": o.energy_tracked(), "slots": o.pt_slots(),
            "info": np.stack(infos).reshape(rounds, NP, 2),
            "pairs": np.stack(lp) if lp else None, "acc": np.stack(la) if la else None}


def conditions(info, acc, M, n, katz=True):
    """The conditions under which an equality case says something: every system has a pair with components over the rounds, a swap was
    accepted, a moved pair was not a global flip.  -> list of the conditions that fail (empty: all hold)."""
    info = np.asarray(info)
    per = info.reshape(info.shape[0], M, -1, 2)
    bad = []
    if not all((per[:, s, :, 0] > 0).any() for s in range(M)):
        bad.append("a system never had a pair with components")
    if acc is None or not np.asarray(acc).sum() > 0:
        bad.append("no swap accepted")
    size = info[..., 1]
    if not ((size > 0) & ((size <= n // 2) | (not katz))).any():
        bad.append("every moved pair was a global flip")
    return bad


# ---- the cases the CPU and the GPU tests share -----------------------------------------------------------------------------------------
SEED = 0xC35A0000 + (0x91 << 32)         # high bits set; test_apt_systems_cpu checks that the helper alone meets `conditions` on every case
ROUNDS, SWEEPS = 4, 2


def instance(P, name):
    """-> (J, h, betas(L))"""
    import os
    import scipy.sparse as sp
    from conftest import GOLDEN
    inst = os.path.join(GOLDEN, "instances")
    if name == "wishart10":
        W, _ = P.instances.txt_to_A_wishart(os.path.join(inst, "wishart_N10_a0.50__wishart_planting_N_10_alpha_0.50_inst_1.txt"))
        J = (-W).toarray()
        return J / float(np.max(np.abs(J))), np.zeros(J.shape[0]), lambda L: np.geomspace(0.3, 1.5, L)
    if name == "chimera128":
        W, h = P.instances.txt_to_A_droplet(os.path.join(inst, "chimera128__001.txt"))
        J = -sp.csr_matrix(W).astype(np.float64)
        s = np.max(np.abs(J.data))
        return (J / s).tocsr(), -np.asarray(h, dtype=np.float64).ravel() / s, lambda L: np.linspace(1.0, 1.2, L)        # close temperatures: swaps of 128-spin chains are accepted within four rounds
    raise KeyError(name)


# name -> (instance, M, K, L, rounds, precision): the round-by-round cases against the helper ...
ORACLE_CASES = {
    "wishart10_M3_K4_L3_f32": ("wishart10", 3, 4, 3, ROUNDS, "f32"),
    "wishart10_M3_K4_L3_f64": ("wishart10", 3, 4, 3, ROUNDS, "f64"),
    "wishart10_M2_K5_L6_f32": ("wishart10", 2, 5, 6, ROUNDS, "f32"),       # odd K: a ladder per (system, slot) sits out
    "chimera128_M2_K4_L3_f32": ("chimera128", 2, 4, 3, ROUNDS, "f32"),
    "wishart10_M2_K258_L2_f32": ("wishart10", 2, 258, 2, 1, "f32"),        # K above the workgroup's 256 threads: k_icm_pair_ladders
}
# ... and the in-launch cases (the kernel against the round-by-round route; the helper only has to meet the conditions)
LAUNCH_CASES = {
    "wishart10_M3_K4_L3": ("wishart10", 3, 4, 3, ROUNDS, "f32"),
    "wishart10_M2_K12_L6": ("wishart10", 2, 12, 6, ROUNDS, "f32"),         # two waves per system (P = 10 ladders a wave), tail lanes
    "wishart10_M300_K2_L3": ("wishart10", 300, 2, 3, ROUNDS, "f32"),       # more workgroups than compute units
}

_ORACLE = {}


def oracle_case(P, case, efix0=None):
    """oracle_rounds of a case tuple from init_spins, computed once (efix0: the engine's own start energies, see set_spins)."""
    from helpers import init_spins
    key = (case, efix0 is not None)
    if key not in _ORACLE:
        name, M, K, L, rounds, prec = case
        J, h, betas = instance(P, name)
        inst = P.Instance(J, h)
        _ORACLE[key] = oracle_rounds(inst, M, K, L, SWEEPS, rounds, prec, betas(L), init_spins(M * K * L, inst.n), SEED, n_pairs_of(L),
                                     efix0=efix0)
        _ORACLE[key]["n"] = inst.n
    return _ORACLE[key]


class RunEngine(SystemsOracleEngine):
    """The helper as APT_ICM._run_device_resident drives an engine: a recorded trace, a swap log kept until it is read."""
    made = []

    def __init__(self, inst, betas, n_chains, device=0):
        super().__init__(inst, n_chains, 0, n_chains)
        self.log = []
        RunEngine.made.append(self)

    def pt_log_begin(self, round0, n_rounds, n_pairs):
        self.log = []

    def pt_log_read(self):
        return (np.stack([p for p, _ in self.log]), np.stack([a for _, a in self.log]))

    def pt_swap_philox(self, rnd, seed, n_pairs, want_log=True):
        out = super().pt_swap_philox(rnd, seed, n_pairs)
        self.log.append(out)
        return out

    def sweep_philox(self, n_sweeps, seed, sweep0=0, beta=None, precision="f32", record_stride=0):
        rec = []
        for t in range(n_sweeps):
            super().sweep_philox(1, seed, sweep0=sweep0 + t, precision=precision)
            rec.append(self.spins.copy())
        self.recorded = np.stack(rec, axis=1) if rec else np.zeros((self.n_chains, 0, self.n), np.int8)
        return {"spins": self.recorded} if record_stride else {}

    def energy_of_recorded(self, n_rec):
        return np.array([[oracle.energy(self.csr, self.h, s) for s in row] for row in self.recorded])

    def energy(self):
        return np.array([oracle.energy(self.csr, self.h, s) for s in self.spins])
