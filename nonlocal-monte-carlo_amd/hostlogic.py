"""Host-side (Python) logic that stays on the CPU in the reference too: temperature schedules, phase flags,
stream drawing in the reference's program order.  No spin is updated here."""
import numpy as np

from . import _abi


def beta_schedule(num_sweeps, beta, anneal=False, sweeps_per_beta=1, initial_beta=0):
    """Per-sweep inverse temperature of MCMC() (NMC/nmc.py:56-69).  The index is incremented BEFORE use, so
    linspace's first value is never applied; num_betas = num_sweeps // sweeps_per_beta."""
    run = np.full(int(num_sweeps), float(beta), dtype=np.float64)
    if anneal:
        nb = int(num_sweeps) // int(sweeps_per_beta)
        vals = np.linspace(initial_beta, beta, nb)
        idx = 0
        for jj in range(int(num_sweeps)):
            if jj % sweeps_per_beta == 0 and idx < nb - 1:
                idx += 1
            run[jj] = vals[idx]
    return run


def draw_legacy_stream(n_sweeps, n):
    """One chain's draws in the reference's order: per sweep np.random.permutation(N) then N x np.random.rand()
    (NMC/nmc.py:71,87).  Consumes the global legacy NumPy stream exactly like the reference does."""
    perm = np.empty((n_sweeps, n), dtype=np.int32)
    u = np.empty((n_sweeps, n), dtype=np.float64)
    for t in range(n_sweeps):
        perm[t] = np.random.permutation(n)
        u[t] = np.random.rand(n)
    return perm, u


def check_wave_rounds(wave_rounds, waves, needs="waves='auto' or 'force'"):
    """wave_rounds without wave sweeps: ValueError.  `needs`: how the caller's keyword is spelled in the message."""
    if wave_rounds and waves == "off":
        raise ValueError(f"wave_rounds needs {needs} (the rounds run inside the wave kernels' launches)")


def check_wave_long(wave_long, waves, needs="waves='auto' or 'force'"):
    """wave_long without wave sweeps: ValueError.  `needs`: how the caller's keyword is spelled in the message."""
    if wave_long and waves == "off":
        raise ValueError(f"wave_long needs {needs} (it widens the wave route to chains of up to 1024 spins)")


def check_wave_nmc(wave_nmc, waves, needs="waves='auto' or 'force'"):
    """wave_nmc given (True or False) without wave sweeps: ValueError.  `needs`: how the caller's keyword is spelled in the message."""
    if wave_nmc is not None and waves == "off":
        raise ValueError(f"wave_nmc needs {needs} (it says how the NMC phases run on the wave route)")


def check_wave_long_nmc(wave_long_nmc, wave_long):
    """wave_long_nmc given (True or False) without wave_long: ValueError."""
    if wave_long_nmc is not None and not wave_long:
        raise ValueError("wave_long_nmc needs wave_long=True (it says how the NMC phases of chains of 257 to 1024 spins run on the wave route)")


def check_wave_long_rounds(wave_long_rounds, wave_rounds, wave_long):
    """wave_long_rounds without wave_rounds or without wave_long: ValueError."""
    if wave_long_rounds and not (wave_rounds and wave_long):
        raise ValueError("wave_long_rounds needs wave_rounds=True and wave_long=True (the rounds of chains of 257..1024 spins run "
                         "inside the long wave kernel's launches)")


def check_route_keywords(lanes="off", waves="off", wave_rounds=False, rng=None, precision="f32", wave_long=False, wave_long_rounds=False):
    """The `lanes` / `waves` / `wave_rounds` / `wave_long` / `wave_long_rounds` keywords of NPT, APT_ICM and APT_preprocessor.  rng None (a constructor that
    does not know its backend yet): the mode values only; otherwise also what they need of `rng` and `precision`."""
    for name, mode in (("lanes", lanes), ("waves", waves)):
        if mode not in ("off", "auto", "force"):
            raise ValueError(f"{name} must be 'off', 'auto' or 'force'")
    if rng is None:
        return
    for name, mode in (("lanes", lanes), ("waves", waves)):
        if mode != "off" and rng != "philox":
            raise ValueError(f"{name} applies to rng='philox' (rng='numpy' runs the reference's own stream order)")
    if waves != "off" and precision == "f64":
        raise ValueError("waves applies to precision='f32' (the wave-per-chain sweeps have no fp64 arithmetic)")
    check_wave_rounds(wave_rounds, waves)
    if wave_rounds and precision == "f64":
        raise ValueError("wave_rounds applies to precision='f32' (the wave-per-chain kernels have no fp64 arithmetic)")
    check_wave_long(wave_long, waves)
    if wave_long and rng != "philox":
        raise ValueError("wave_long applies to rng='philox' (rng='numpy' runs the reference's own stream order)")
    if wave_long and precision == "f64":
        raise ValueError("wave_long applies to precision='f32' (the wave-per-chain kernels have no fp64 arithmetic)")
    check_wave_long_rounds(wave_long_rounds, wave_rounds, wave_long)


def set_route_modes(eng, lanes="off", waves="off", wave_rounds=False, wave_long=False, wave_long_rounds=False):
    """Engine.set_lane_sweeps / set_wave_sweeps / set_wave_rounds / set_wave_long / set_wave_long_rounds of a fresh engine, for the
    modes that are not the default.  wave_long_rounds without wave_rounds and wave_long: ValueError."""
    check_wave_long_rounds(wave_long_rounds, wave_rounds, wave_long)
    if lanes != "off":
        eng.set_lane_sweeps(lanes)
    if waves != "off":
        eng.set_wave_sweeps(waves)
    if wave_rounds:
        eng.set_wave_rounds(True)
    if wave_long:
        eng.set_wave_long(True)
    if wave_long_rounds:
        eng.set_wave_long_rounds(True)


def phase_flags(n, m_init, clusters, phase):
    """Flags realising the three NMC phases (NMC/nmc.py:377-381, 398-401, 419-421):
       'C'  : cluster rows of (J,h) / temp_x, every other spin frozen by h = 10000 * m_init
       'NC' : cluster spins frozen by h = 10000 * m_init
       'ALL': plain (J,h)."""
    fl = np.zeros(n, dtype=np.uint8)
    if phase == "ALL":
        return fl
    m_init = np.asarray(m_init)
    cl = np.asarray(clusters, dtype=np.int64)
    frozen_code = np.where(m_init > 0, _abi.SPIN_FROZEN_UP, _abi.SPIN_FROZEN_DOWN).astype(np.uint8)
    if phase == "C":
        fl[:] = frozen_code
        fl[cl] = _abi.SPIN_SCALED
    elif phase == "NC":
        fl[cl] = frozen_code[cl]
    else:
        raise ValueError(phase)
    return fl


# ---- what a per-round energy log says about a ladder (Engine.elog_read; no device code) --------------------------------------
def log_by_slot(energies, slots, ladder_len):
    """A log by chain -> by temperature slot.  energies, slots [n_rounds, G], chains g L .. g L + L - 1 forming ladder g ->
    (energy [n_rounds, G // L, L], chain [n_rounds, G // L, L]): the energy on every slot and the chain (its index in the log's
    columns) that held it; NaN / -1 in rows no observation reached."""
    e, s = np.asarray(energies, dtype=np.float64), np.asarray(slots)
    L = int(ladder_len)
    R, G = e.shape
    if L < 1 or G % L != 0 or s.shape != e.shape:
        raise ValueError("log_by_slot: energies and slots must be [n_rounds, n_ladders * ladder_len]")
    nl = G // L
    by_e, by_c = np.full((R, nl, L), np.nan), np.full((R, nl, L), -1, dtype=np.int32)
    seen = s >= 0
    rr, cc = np.nonzero(seen)
    by_e[rr, cc // L, s[rr, cc]] = e[rr, cc]
    by_c[rr, cc // L, s[rr, cc]] = cc
    return by_e, by_c


def ladder_report(energies, slots, beta_list):
    """Mixing statistics of every ladder of a per-round energy log.  energies, slots [n_rounds, G] by chain as elog_read returns
    them (rows no observation reached, NaN / -1, are left out), beta_list [L], chains g L .. g L + L - 1 forming ladder g.  A list
    with one dict per ladder:
      beta [L]; mean_energy [L], sigma_energy [L]  by temperature slot, over the observed rounds; sigma is the population standard
                                                   deviation (np.std), what APT_preprocessor calls sigma_E (NPT/apt_preprocessor.py:179)
      swap_attempts [L - 1]   transitions between two consecutive observed rounds: every adjacent pair of slots had that many chances
      swap_accepts [L - 1]    transitions in which the chains on slots i and i + 1 exchanged their slots
      acceptance [L - 1]      accepts / attempts: the rate of exchange per ROUND (a round selects n_pairs of the L - 1 pairs, so this
                              is the chance of being selected times the acceptance of a selected pair -- what the ladder mixes with);
                              NaN without a transition.  Derived from the slots alone: the swap log is not needed.
      round_trips [L]         per chain of the ladder: completed journeys slot 0 -> slot L - 1 -> slot 0
      tau_round_trip          observed rounds x chains / all round trips: rounds a chain needs per trip, inf if there was none
      n_rounds                observed rounds"""
    beta = np.asarray(beta_list, dtype=np.float64).reshape(-1)
    L = beta.size
    by_e, by_c = log_by_slot(energies, slots, L)
    s_all = np.asarray(slots)
    out = []
    for g in range(by_e.shape[1]):
        ok = (by_c[:, g, :] >= 0).all(axis=1)
        e, c = by_e[ok, g, :], by_c[ok, g, :]
        n_obs = int(e.shape[0])
        with np.errstate(invalid="ignore"):
            mean = e.mean(axis=0) if n_obs else np.full(L, np.nan)
            sigma = e.std(axis=0) if n_obs else np.full(L, np.nan)
        # transitions between CONSECUTIVE rounds that were both observed
        idx = np.nonzero(ok)[0]
        cons = np.nonzero(np.diff(idx) == 1)[0]
        attempts = np.full(max(L - 1, 0), cons.size, dtype=np.int64)
        accepts = np.zeros(max(L - 1, 0), dtype=np.int64)
        if L > 1 and cons.size:
            a, b = c[cons], c[cons + 1]
            accepts = ((a[:, :-1] == b[:, 1:]) & (a[:, 1:] == b[:, :-1])).sum(axis=0).astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            acceptance = np.where(attempts > 0, accepts / np.maximum(attempts, 1), np.nan)
        trips = np.zeros(L, dtype=np.int64)
        sl = s_all[ok][:, g * L:(g + 1) * L]
        for j in range(L):
            leg = 0                                   # 0: not at the bottom yet, 1: left slot 0 for the top, 2: reached the top
            for v in sl[:, j]:
                if v == 0:
                    if leg == 2:
                        trips[j] += 1
                    leg = 1
                elif v == L - 1 and leg == 1:
                    leg = 2
        total = int(trips.sum())
        out.append(dict(beta=beta.copy(), mean_energy=mean, sigma_energy=sigma, swap_attempts=attempts, swap_accepts=accepts,
                        acceptance=acceptance, round_trips=trips, tau_round_trip=(n_obs * L / total) if total else float("inf"),
                        n_rounds=n_obs))
    return out


def pool_reports(reports):
    """One report for several ladders at the same temperatures (the sub-replicas of an APT system): means of mean_energy and
    sigma_energy over the ladders (APT_preprocessor averages the replicas' standard deviations), attempts and accepts summed,
    round_trips concatenated."""
    reports = list(reports)
    att = np.sum([r["swap_attempts"] for r in reports], axis=0)
    acc = np.sum([r["swap_accepts"] for r in reports], axis=0)
    trips = np.concatenate([r["round_trips"] for r in reports])
    n_obs = max(r["n_rounds"] for r in reports)
    total = int(trips.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        acceptance = np.where(att > 0, acc / np.maximum(att, 1), np.nan)
    return dict(beta=reports[0]["beta"].copy(), mean_energy=np.mean([r["mean_energy"] for r in reports], axis=0),
                sigma_energy=np.mean([r["sigma_energy"] for r in reports], axis=0), swap_attempts=att, swap_accepts=acc,
                acceptance=acceptance, round_trips=trips, tau_round_trip=(n_obs * trips.size / total) if total else float("inf"),
                n_rounds=n_obs)


def suggest_ladder(report, beta_list, alpha=1.25, beta_max=None, sigma_min=0.0, max_len=4096):
    """A new ladder from the measured energy spread, by APT_preprocessor's recurrence beta_{i+1} = beta_i + alpha / sigma_E(beta_i)
    (NPT/apt_preprocessor.py:151-186), starting at the smallest measured beta.  sigma_E(beta) is report["sigma_energy"] interpolated
    linearly in beta between the measured slots and held constant outside them.  It stops as the preprocessor stops: when sigma_E at
    the last beta is not above `sigma_min` (the caller passes 0.5 min|J_ij|, the preprocessor's freeze-out), or when the last beta
    exceeds `beta_max` (default: the largest measured beta) -- like the preprocessor's list, the result may END with the one value
    above beta_max.  `report`: one dict of ladder_report / pool_reports.  Returns a strictly increasing float64 array."""
    b = np.asarray(beta_list, dtype=np.float64).reshape(-1)
    sig = np.asarray(report["sigma_energy"], dtype=np.float64).reshape(-1)
    if b.size != sig.size or b.size == 0:
        raise ValueError("suggest_ladder: the report and beta_list differ in length")
    if not (alpha > 0):
        raise ValueError("suggest_ladder: alpha must be positive")
    order = np.argsort(b, kind="stable")
    b, sig = b[order], sig[order]
    bmax = float(b[-1]) if beta_max is None else float(beta_max)
    out = [float(b[0])]
    while len(out) < int(max_len):
        s = float(np.interp(out[-1], b, sig))
        if not (s > sigma_min) or not np.isfinite(s) or out[-1] > bmax:
            break
        out.append(out[-1] + alpha / s)
    return np.asarray(out, dtype=np.float64)
