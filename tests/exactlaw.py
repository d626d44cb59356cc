"""Exact Boltzmann laws of instances made of small disjoint blocks, and the statistics that compare a sample with them.

On an instance that is a disjoint union of 6-spin blocks the Boltzmann law factorises: each block's law is known by enumeration
(64 states), exact equilibrium starts can be drawn on the host, and every correct transition -- a heat-bath sweep in any order, a
replica swap, a Houdayer exchange -- leaves that law invariant.  So the block states after any number of rounds are exact,
independent samples of a known finite distribution, and a driver-level mistake (a counter used twice, a round index that does not
advance, a wrong sign in the swap test) shows as a departure from it.  CPU only; no product import.

Energy convention (oracle/nlo.c: nlo_energy): E(s) = -(1/2 s^T J s + h . s).  Dyadic species have couplings in multiples of 1/4 and
fields in multiples of 1/8, so their energies are exact integers in units of 1/8.

Decision rule: family-wise ALPHA = 1e-4 per test; with m statistics in a test each p-value must be >= ALPHA / m (Bonferroni)."""
import numpy as np
import scipy.signal
import scipy.sparse as sp
import scipy.stats as st
from mpmath import mp, mpf, exp as mpexp

ALPHA = 1e-4
NB = 6                      # spins of a block
UNIT = 8                    # dyadic energies are integers in units of 1 / UNIT
mp.dps = 60

STATES = np.array([[1 if (k >> i) & 1 else -1 for i in range(NB)] for k in range(1 << NB)], dtype=np.int8)      # [64, 6]


class Species:
    """One kind of block: dense symmetric J [6, 6] with a zero diagonal, fields h [6]."""

    def __init__(self, name, J, h, dyadic):
        self.name, self.J, self.h, self.dyadic = name, np.asarray(J, float), np.asarray(h, float), dyadic
        assert np.array_equal(self.J, self.J.T) and not np.any(np.diag(self.J))
        s = STATES.astype(np.float64)
        self.energy = -(0.5 * np.einsum("ki,ij,kj->k", s, self.J, s) + s @ self.h)                 # [64] (exact for dyadic species)
        if dyadic:
            assert np.array_equal(self.J * 4, np.rint(self.J * 4)) and np.max(np.abs(self.J)) <= 1
            assert np.array_equal(self.h * 8, np.rint(self.h * 8))
            e8 = self.energy * UNIT
            assert np.array_equal(e8, np.rint(e8))
            self.e8 = e8.astype(np.int64)


def _sym(n, entries):
    J = np.zeros((n, n))
    for (i, j), v in entries.items():
        J[i, j] = J[j, i] = v
    return J


def _k6():
    q = [4, -3, 2, -4, 1, -2, 3, 4, -1, -4, 2, -3, 1, 4, -2]                        # upper triangle by rows, units of 1/4
    iu = np.triu_indices(NB, 1)
    return Species("k6", _sym(NB, {(int(i), int(j)): v / 4 for i, j, v in zip(*iu, q)}), np.array([1, -2, 3, 0, -1, 2]) / 8, True)


def _ring2():
    e = {(0, 1): 4, (1, 2): -4, (2, 3): 3, (3, 4): 4, (4, 5): -2, (0, 5): 4, (0, 3): -3, (1, 4): 2}
    return Species("ring2", _sym(NB, {k: v / 4 for k, v in e.items()}), np.array([-1, 2, 0, 1, -3, 2]) / 8, True)


def _gauss():
    r = np.random.default_rng(660066)
    iu = np.triu_indices(NB, 1)
    return Species("gauss", _sym(NB, {(int(i), int(j)): float(v) for i, j, v in zip(*iu, 0.6 * r.standard_normal(15))}),
                   0.3 * r.standard_normal(NB), False)


K6, RING2, GAUSS = _k6(), _ring2(), _gauss()


def is_frustrated(sp_):
    """Some triangle or 4-cycle of the block has a negative product of couplings."""
    J = sp_.J
    for a in range(NB):
        for b in range(a + 1, NB):
            for c in range(b + 1, NB):
                if J[a, b] * J[b, c] * J[a, c] < 0:
                    return True
                for d in range(NB):
                    if d not in (a, b, c) and J[a, b] * J[b, c] * J[c, d] * J[d, a] < 0:
                        return True
    return False


# ---- instances --------------------------------------------------------------------------------------------------------------------
class BlockInstance:
    """`copies` blocks, block b of species[b % len(species)].  idx[b, i]: spin index of member i of block b."""

    def __init__(self, species, copies, layout):
        self.species = list(species) if isinstance(species, (list, tuple)) else [species]
        self.copies, self.layout, self.n = int(copies), layout, NB * int(copies)
        b, i = np.meshgrid(np.arange(copies), np.arange(NB), indexing="ij")
        self.idx = {"contiguous": NB * b + i, "strided": b + copies * i}[layout].astype(np.int64)
        self.kind = np.arange(copies) % len(self.species)                     # species index of block b
        rows, cols, vals, h = [], [], [], np.zeros(self.n)
        for k, spc in enumerate(self.species):
            blocks = np.nonzero(self.kind == k)[0]
            ii, jj = np.nonzero(spc.J)
            rows.append(self.idx[blocks][:, ii].ravel())
            cols.append(self.idx[blocks][:, jj].ravel())
            vals.append(np.tile(spc.J[ii, jj], len(blocks)))
            h[self.idx[blocks]] = spc.h
        self.J = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(self.n, self.n)).tocsr()
        self.J.sort_indices()
        self.h = h

    def blocks_of(self, k):
        return np.nonzero(self.kind == k)[0]

    def state_index(self, spins):
        """spins [..., n] -> block state indices [..., copies] (bit i set: member i is +1)."""
        s = np.asarray(spins)[..., self.idx] > 0
        return (s * (1 << np.arange(NB))).sum(axis=-1).astype(np.int64)

    def spins_of(self, state):
        """block state indices [..., copies] -> spins [..., n] int8."""
        state = np.asarray(state)
        out = np.empty(state.shape[:-1] + (self.n,), np.int8)
        out[..., self.idx] = STATES[state]
        return out

    def block_energy(self, state):
        """Energies [..., copies] of block states [..., copies]."""
        E = np.stack([spc.energy for spc in self.species])                     # [species, 64]
        return E[self.kind, np.asarray(state)]


def block_instance(species, copies, layout):
    """-> (CSR J, h, idx [copies, 6]: the spin index of (block, member)); BlockInstance holds the same with the maps by block."""
    bi = BlockInstance(species, copies, layout)
    return bi.J, bi.h, bi.idx


# ---- the exact law ----------------------------------------------------------------------------------------------------------------
class Law:
    """Boltzmann law of one block species at beta: p [64] (mpmath at 60 digits, rounded to double), exact mean and variance of E."""

    def __init__(self, spc, beta):
        self.species, self.beta = spc, float(beta)
        b = mpf(float(beta))
        en = [mpf(int(e)) / UNIT for e in spc.e8] if spc.dyadic else [mpf(float(e)) for e in spc.energy]
        w = [mpexp(-b * e) for e in en]
        Z = sum(w)
        p = [x / Z for x in w]
        m1 = sum(pi * e for pi, e in zip(p, en))
        m2 = sum(pi * e * e for pi, e in zip(p, en))
        self.p = np.array([float(x) for x in p])
        self.mean, self.var = float(m1), float(m2 - m1 * m1)

    def overlap_law(self, other=None):
        """Law of q = sum_i s_i s'_i in {-6, -4, .., 6} for two independent samples (of this law and `other`) -> [7]."""
        other = self if other is None else other
        q = (STATES.astype(np.int64) @ STATES.astype(np.int64).T + NB) // 2                # [64, 64] in 0..6
        out = np.zeros(NB + 1)
        np.add.at(out, q.ravel(), np.outer(self.p, other.p).ravel())
        return out

    def energy_pmf(self):
        """(offset, pmf): P(e8 = offset + k) of a dyadic species."""
        e8 = self.species.e8
        lo = int(e8.min())
        out = np.zeros(int(e8.max()) - lo + 1)
        np.add.at(out, e8 - lo, self.p)
        return lo, out


def chain_energy_pmf(bi, beta):
    """Exact distribution of a chain's total energy in units of 1/8: integer convolution of the block distributions -> (offset, pmf)."""
    lo, pmf = 0, np.ones(1)
    for k, spc in enumerate(bi.species):
        o, f = Law(spc, beta).energy_pmf()
        for _ in range(len(bi.blocks_of(k))):
            pmf = np.convolve(pmf, f)
            lo += o
    return lo, pmf


def acceptance(pmf_a, pmf_b, beta_a, beta_b, sign=1.0):
    """E[min(1, exp(sign (beta_b - beta_a)(E_b - E_a)))] for independent chain energies with the given (offset, pmf)."""
    (la, fa), (lb, fb) = pmf_a, pmf_b
    d = scipy.signal.fftconvolve(fb, fa[::-1])                                            # P(e_b - e_a = lb - la - (len(fa) - 1) + k)
    d = np.clip(d, 0.0, None)
    dE = (lb - la - (len(fa) - 1) + np.arange(len(d))) / UNIT
    return float(np.sum(d * np.minimum(1.0, np.exp(np.minimum(0.0, sign * (beta_b - beta_a) * dE)))) / np.sum(d))


def equilibrium_start(rng, bi, beta_of_chain):
    """Independent exact block samples for every chain -> spins [R, n] int8."""
    beta_of_chain = np.asarray(beta_of_chain, float)
    state = np.empty((len(beta_of_chain), bi.copies), np.int64)
    for beta in np.unique(beta_of_chain):
        rows = np.nonzero(beta_of_chain == beta)[0]
        for k, spc in enumerate(bi.species):
            blocks = bi.blocks_of(k)
            cdf = np.cumsum(Law(spc, beta).p)
            cdf[-1] = 1.0
            state[np.ix_(rows, blocks)] = np.searchsorted(cdf, rng.random((len(rows), len(blocks))), side="right")
    return bi.spins_of(state)


# ---- statistics: each returns a p-value (and what it was made of) -------------------------------------------------------------------
def chi2_counts(counts, p, min_expected=5.0):
    """Pearson chi-square of counts against p; cells with expectation < min_expected are pooled into one.
    -> dict(chi2, dof, p, pooled_mass)."""
    counts, p = np.asarray(counts, float), np.asarray(p, float)
    n = counts.sum()
    e = n * p
    small = e < min_expected
    obs, ex = counts[~small], e[~small]
    if small.any():
        obs, ex = np.append(obs, counts[small].sum()), np.append(ex, e[small].sum())
    keep = ex > 0
    obs, ex = obs[keep], ex[keep]
    chi2 = float(np.sum((obs - ex) ** 2 / ex))
    dof = len(ex) - 1
    return {"chi2": chi2, "dof": dof, "p": float(st.chi2.sf(chi2, dof)), "pooled_mass": float(p[small].sum()), "n": int(n)}


def chi2_states(state, law):
    """(i) block states [...] against the law's 64 probabilities."""
    return chi2_counts(np.bincount(np.asarray(state).ravel(), minlength=1 << NB), law.p)


def z_two_sided(z):
    return float(2.0 * st.norm.sf(abs(z)))


def z_mean_energy(sum_e, n_by_law):
    """(ii) total of block energies against the exact mean and variance; n_by_law: [(n, law)].  -> dict(z, p, n, var_sum)."""
    mu = sum(n * law.mean for n, law in n_by_law)
    var = sum(n * law.var for n, law in n_by_law)
    z = (float(sum_e) - mu) / np.sqrt(var)
    return {"z": float(z), "p": z_two_sided(z), "n": int(sum(n for n, _ in n_by_law)), "var_sum": float(var)}


def z_adjacent_correlation(x):
    """(iii) x [chains, blocks]: block energies standardised with their exact mean and deviation, in block index order.  Under
    independence the products x_b x_{b+1} have mean 0, variance 1 and are uncorrelated."""
    prod = x[:, :-1] * x[:, 1:]
    z = float(prod.sum() / np.sqrt(prod.size))
    return {"z": z, "p": z_two_sided(z), "n": int(prod.size)}


def chi2_overlap(spins_a, spins_b, bi, k, law_a, law_b=None):
    """(iv) block overlaps of species k between two sets of configurations that should be independent."""
    blocks = bi.blocks_of(k)
    q = (np.asarray(spins_a)[..., bi.idx[blocks]].astype(np.int64) * np.asarray(spins_b)[..., bi.idx[blocks]]).sum(axis=-1)
    return chi2_counts(np.bincount(((q + NB) // 2).ravel(), minlength=NB + 1), law_a.overlap_law(law_b))


def z_acceptance(attempts, accepted, expect):
    """(v) attempts, accepted [ladders]: per independent ladder, how often one adjacent pair was tried and accepted over the rounds.
    D_l = accepted_l - attempts_l * expect has mean 0 whatever the correlation between a ladder's rounds; ladders are independent,
    so z = sum D / sqrt(sum D^2) is standard normal."""
    D = np.asarray(accepted, float) - np.asarray(attempts, float) * expect
    den = np.sqrt(np.sum(D * D))
    z = float(D.sum() / den) if den > 0 else 0.0
    return {"z": z, "p": z_two_sided(z), "n": int(np.sum(attempts)), "rate": float(np.sum(accepted) / max(1, np.sum(attempts)))}


def z_threshold(m):
    """|z| at which a two-sided test at ALPHA / m rejects."""
    return float(st.norm.isf(ALPHA / m / 2.0))


def delta_star(beta, var_sum, m):
    """Smallest relative temperature error statistic (ii) rejects: d<E>/d(ln beta) = -beta Var E, so a sum of n block energies
    moves by z_thr deviations at delta* = z_thr / (beta sqrt(n Var E)).  var_sum = sum of the exact block variances."""
    return z_threshold(m) / (float(beta) * np.sqrt(var_sum))


def blocks_needed(species, betas, copies, max_delta, m):
    """Chains per slot so that delta* <= max_delta at every beta, from the exact variances alone."""
    need = 0
    for beta in betas:
        var_chain = sum(Law(spc, beta).var * np.sum(np.arange(copies) % len(species) == k) for k, spc in enumerate(species))
        need = max(need, int(np.ceil((z_threshold(m) / (beta * max_delta)) ** 2 / var_chain)))
    return need


# ---- one slot's evaluation ---------------------------------------------------------------------------------------------------------
def slot_statistics(bi, spins, beta, correlation=True, blocks=None):
    """Statistics (i)-(iii) of configurations [chains, n] against the exact law at beta -> {name: result dict}.
    blocks: the block indices to look at (default: all); the correlation is between neighbours in that list."""
    blocks = np.arange(bi.copies) if blocks is None else np.asarray(blocks)
    state = bi.state_index(spins)[:, blocks]
    kind = bi.kind[blocks]
    laws = [Law(spc, beta) for spc in bi.species]
    out = {}
    for k, law in enumerate(laws):
        if np.any(kind == k):
            out[f"chi2 {law.species.name}"] = chi2_states(state[:, kind == k], law)
    E = np.stack([spc.energy for spc in bi.species])[kind, state]
    out["mean E"] = z_mean_energy(E.sum(), [(state.shape[0] * int(np.sum(kind == k)), law) for k, law in enumerate(laws)])
    if correlation:
        mu = np.array([laws[k].mean for k in kind])
        sd = np.sqrt(np.array([laws[k].var for k in kind]))
        out["adjacent corr"] = z_adjacent_correlation((E - mu) / sd)
    return out


def by_slot(spins, slots, L):
    """spins [G, n], slots [G] -> [L, ladders, n]: the configuration each ladder (chains g L .. g L + L - 1) holds at each slot."""
    G = spins.shape[0]
    out = np.empty((L, G // L) + spins.shape[1:], spins.dtype)
    out[np.asarray(slots), np.arange(G) // L] = spins
    return out


def swap_counts(pairs, acc, L):
    """Swap log pairs [rounds, ladders, P, 2], acc [rounds, ladders, P] -> attempts, accepted [L - 1, ladders]."""
    nl = pairs.shape[1]
    att, got = np.zeros((L - 1, nl)), np.zeros((L - 1, nl))
    lad = np.broadcast_to(np.arange(nl)[None, :, None], acc.shape)
    np.add.at(att, (pairs[..., 0].ravel(), lad.ravel()), 1)
    np.add.at(got, (pairs[..., 0].ravel(), lad.ravel()), np.asarray(acc).ravel())
    return att, got


class Verdict:
    """The statistics of one test: name -> p under the true law, and p under each wrong hypothesis (smallest of its statistics)."""

    def __init__(self, route):
        self.route, self.true, self.wrong, self.delta, self.pooled, self._acc, self._slots = route, {}, {}, [], [], [], []

    def add(self, name, res):
        self.true[name] = res
        if "pooled_mass" in res:
            self.pooled.append(res["pooled_mass"])

    def add_slot(self, tag, bi, spins, beta, correlation=True, blocks=None):
        """(i)-(iii) at the true beta; finish() evaluates the same sample against beta (1 + 2 delta*) as a wrong hypothesis."""
        res = slot_statistics(bi, spins, beta, correlation, blocks)
        for k, v in res.items():
            self.add(f"{tag} {k}", v)
        self._slots.append((tag, bi, spins, beta, res["mean E"]["var_sum"], blocks))

    def add_acceptance(self, bi, betas, pairs, acc):
        """(v) per adjacent ladder pair against the exact expectation; finish() evaluates the same counts against the expectation
        with the sign of dBeta dE flipped as a wrong hypothesis."""
        L = len(betas)
        pm = [chain_energy_pmf(bi, b) for b in betas]
        att, got = swap_counts(pairs, acc, L)
        for i in range(L - 1):
            self.add(f"pair{i} acceptance", z_acceptance(att[i], got[i], acceptance(pm[i], pm[i + 1], betas[i], betas[i + 1])))
            self._acc.append((i, att[i], got[i], acceptance(pm[i], pm[i + 1], betas[i], betas[i + 1], sign=-1.0)))

    def add_wrong(self, name, p):
        self.wrong[name] = min(self.wrong.get(name, 1.0), p)

    @property
    def m(self):
        return len(self.true)

    def finish(self):
        """Once every true statistic is in: delta* per slot with the final m, and the wrong temperature beta (1 + 2 delta*)."""
        for tag, bi, spins, beta, var_sum, blocks in self._slots:
            d = delta_star(beta, var_sum, self.m)
            self.delta.append(d)
            res = slot_statistics(bi, spins, beta * (1 + 2 * d), correlation=False, blocks=blocks)
            self.add_wrong(f"{tag} beta(1+2delta*)", min(v["p"] for v in res.values()))
        for i, att, got, flipped in self._acc:
            self.add_wrong(f"pair{i} flipped sign", z_acceptance(att, got, flipped)["p"])
        return self

    def threshold(self):
        return ALPHA / max(1, self.m)

    def ok(self):
        return all(v["p"] >= self.threshold() for v in self.true.values())

    def wrong_rejected(self):
        return all(p < self.threshold() for p in self.wrong.values())

    def worst(self):
        return min(self.true.items(), key=lambda kv: kv[1]["p"])

    def summary(self):
        name, w = self.worst()
        chis = [v for v in self.true.values() if "chi2" in v]
        big = max(chis, key=lambda v: v["chi2"] / max(1, v["dof"])) if chis else {"n": 0, "dof": 0, "chi2": 0.0}
        ds = f"{max(self.delta):.4f}" if self.delta else "-"
        pw = f"{max(self.wrong.values()):.1e}" if self.wrong else "-"
        return (f"STAT {self.route}: m={self.m} n={big['n']} dof={big['dof']} chi2={big['chi2']:.1f} min p={w['p']:.2e} ({name}) "
                f"threshold={self.threshold():.1e} delta*={ds} pooled<={max(self.pooled) if self.pooled else 0:.1e} weakest wrong p={pw}")

