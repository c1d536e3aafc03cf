"""Newton seeds: one crafted wave whose lanes fall into different classes of getT's iteration in the same layer.

getT_chain (samsim_amd/csrc/samsim_thermo.h) runs getT's guarded Newton iteration for the 64 columns of a wave together and keeps
each lane's part in it -- does it want another evaluation, has it left the fast loop for the general routine -- as one bit of two
64-bit lane masks.  A wave of real columns hardly exercises that: in winter every lane is a mushy layer that converges in three or
four evaluations.  Here the lanes of ONE wave disagree in every way the loop knows, in the same layer:

  iso     isothermal at the bottom temperature: the first evaluation already has |f| <= 1, the lane never wants more
  jump    10-25 K between neighbouring layers: the guess (the temperature of the layer below) is far off, many evaluations
  odd     a fresh layer (S_bu < 0.001) and a pure-brine layer among mushy ones: not mushy, odd from the start
  leave   a layer just below 0 C whose guess comes from a cold layer: the iterate overshoots and leaves (-200, 0)
  tiny    a layer whose guess (a layer of all but fresh water a hair below 0 C) has a liquidus salinity under 1e-4

with N_active spread over 2..80, so that lanes sit layers out (partial exec).  The special layers stand at fixed layer numbers
(FEATURE_LAYERS), so that the classes meet in one layer of the wave.

The grid, the snow cover, the surface state, the clock and the forcing are those of tests/test_gpu_up_sweep_trips.py::spread_columns:
the regular grid at Nlayer 80 = 20+40+20, SHEBA winter scalars of the first member of the day-200 ensemble fixture.

`sweep` restates the iteration of one bottom-to-top getT sweep (mo_thermo_functions.f90:62-143, the guess of layer k is the
temperature found for layer k+1, the bottom layer's is T_bottom) in numpy and reports, per layer and lane, the class it falls into
and the number of evaluations: tests/test_newton_seeds_host.py holds the crafted wave against it, on the CPU.
"""
import numpy as np

from samsim_amd import testcases as tcs
from samsim_amd.capi import State
from tests.helpers import golden

WAVE = 64
NLAYER, N_TOP, N_BOTTOM = 80, 20, 20
NSTEPS = 50
CLASSES = ("iso", "jump", "odd", "leave", "tiny")
FEATURE_LAYERS = (5, 25, 45, 65)        # 1-based; a feature uses layers k .. k+3 and needs N_active >= k+4
FRESH_S_BU = 0.0
ODD_FROM = 40
# What the first choice of lanes found (every fifth lane odd, from lane 2 on): in the odd columns of 29 and 42 layers (lanes 22 and
# 32: fresh layer 25 of 29 resp. 42, frozen solid by then, under 0.13 m of snow) the HIP library returns NaN in layer 1 from step 8
# on, with status 0, where the oracle stays finite -- with the library of the parent commit as with this one, the same report line
# for line, so it is no matter of the Newton loop's masks.  Its cause is not found; the odd columns were moved to the lanes in which
# the same layers ran clean.
FINDING = "odd columns of 29 and 42 layers: NaN in layer 1 from step 8 on the device, parent and new alike; oracle finite"
SEED = 20260          # of the jumps' sizes; chosen on the CPU (tests/test_newton_seeds_host.py), see SEEDS_TRIED
# seeds the CPU oracle was asked about: (seed, verdict)
SEEDS_TRIED = ((20260, "status 0 in all 64 columns after 50 steps; every class in layer 5; evaluations 1..>=6"),)

LATENT_HEAT, C_S, C_S_BETA, C_L = tcs.LATENT_HEAT, 2020.0, 7.6973, tcs.C_L
SALT = (-18.7, -0.519, -0.00535)        # sea-salt liquidus (salt_flag 1), mo_thermo_functions.f90:324-326


def S_br(T):
    return SALT[0] * T + SALT[1] * T ** 2 + SALT[2] * T ** 3


def ddT_S_br(T):
    Tc = np.maximum(T, -20.0)           # derivative-only clamp below -20 C, mo_thermo_functions.f90:408-412
    return SALT[0] + 2.0 * SALT[1] * Tc + 3.0 * SALT[2] * Tc ** 2


def H_mushy(T, S_bu):
    """specific enthalpy of a mushy layer at temperature T (the relation getT inverts)"""
    return -LATENT_HEAT + LATENT_HEAT * S_bu / S_br(T) + C_S * T + C_S_BETA * T * T / 2.0


def lane_class(i):
    """the odd columns are among the long ones (ODD_FROM: N_active >= 52, enough ice to carry the snow cover with the freeboard above
    the water line): see FINDING"""
    if i < ODD_FROM:
        return ("iso", "jump", "leave", "tiny")[i % 4]
    return CLASSES[i % len(CLASSES)]


def n_active():
    na = np.rint(np.linspace(2, NLAYER, WAVE)).astype(np.int32)
    assert na[0] == 2 and na[-1] == NLAYER and len(np.unique(na)) == WAVE
    return na


def column_profile(i, n, rng):
    """(T[n], S_bu[n], kind[n]) of lane i with n active layers, top to bottom; kind: 'm' mushy (H from T), 'f' fresh ice at 0 C,
    'b' pure brine at T, 'w' all but fresh water a hair below 0 C"""
    cls = lane_class(i)
    k = (np.arange(n) + 0.5) / n
    T = -15.0 + (15.0 - 1.9) * k                     # spread_columns' linear profile
    S = np.full(n, 5.0)
    kind = np.array(["m"] * n)
    if cls == "iso":
        T[:] = -1.0                                  # cfg.T_bottom: the bottom layer's guess, and then every layer's
    elif cls == "jump":
        d = 10.0 + 15.0 * rng.random(n)
        T = np.where(np.arange(n) % 2 == 0, -3.0, -3.0 - d)
    else:
        for k0 in FEATURE_LAYERS:
            if n < k0 + 4:
                continue
            j = k0 - 1                               # 0-based index of layer k0
            if cls == "odd":
                f, b = (j, j + 2) if (i // len(CLASSES)) % 2 == 0 else (j + 2, j)   # (both kinds meet in layer k0 of the wave)
                kind[f], S[f] = "f", FRESH_S_BU      # fresh ice, 90 % solid
                kind[b], S[b], T[b] = "b", 34.0, -1.0     # sea water at -1 C: S_br(-1) = 18.2 < S_bu, pure brine
            elif cls == "leave":
                T[j], S[j] = -0.05, 0.5              # S_br(-0.05) = 0.93: mushy, 46 % solid; the guess is T[j+1], about -14 C
                T[j + 1] = -14.0
            elif cls == "tiny":
                kind[j + 1], S[j + 1], T[j + 1] = "w", 0.002, -2.0e-6   # S_br(-2e-6) = 3.7e-5 < S_bu: pure brine, and < 1e-4
                T[j], S[j] = -0.5, 2.0
    return T, S, kind


def crafted_wave(seed=SEED):
    """(cfg, State of 64 columns, clock)"""
    z = golden("sheba_ensemble_80.npz")
    cfg, _ = tcs.testcase4(1, nlayer=NLAYER, n_top=N_TOP, n_bottom=N_BOTTOM)
    rng = np.random.default_rng(seed)
    na = n_active()
    lay = np.zeros((4, NLAYER, WAVE))
    for i, n in enumerate(na):
        T, S_bu, kind = column_profile(i, int(n), rng)
        H, phi = np.zeros(n), np.zeros(n)
        for j in range(n):
            if kind[j] == "m":
                phi[j] = 1.0 - S_bu[j] / S_br(T[j])
                H[j] = H_mushy(T[j], S_bu[j])
                assert 0.0 < phi[j] < 1.0
            elif kind[j] == "f":
                phi[j], H[j] = 0.9, -0.9 * LATENT_HEAT
            else:
                phi[j], H[j] = 0.0, C_L * T[j]
        m = cfg.thick_0 / (phi / 920.0 + (1.0 - phi) / tcs.RHO_L)
        lay[0, :n, i], lay[1, :n, i], lay[2, :n, i], lay[3, :n, i] = H * m, S_bu * m, m, cfg.thick_0
    scal = np.ascontiguousarray(np.repeat(z["scal"][:, :1], WAVE, axis=1))
    clock = dict(time=float(z["time"]), step=int(z["step"]), n_time_out=int(z["n_time_out"]),
                 time_counter=int(z["time_counter"]), n_outputs=int(z["n_outputs"]))
    return cfg, State(np.ascontiguousarray(lay), scal, na), clock


def warm_wave():
    """(cfg, State, clock, dT2m, precip_scale): the first 64 members of the day-360 SHEBA ensemble (melt season), not crafted"""
    z = golden("sheba_ensemble_80_day360.npz")
    cfg, _ = tcs.testcase4(1, nlayer=int(z["nlayer"]), n_top=int(z["n_top"]), n_bottom=int(z["n_bottom"]))
    st = State(np.ascontiguousarray(z["lay"][:, :, :WAVE]), np.ascontiguousarray(z["scal"][:, :WAVE]),
               np.ascontiguousarray(z["n_active"][:WAVE]))
    clock = dict(time=float(z["time"]), step=int(z["step"]), n_time_out=int(z["n_time_out"]),
                 time_counter=int(z["time_counter"]), n_outputs=int(z["n_outputs"]))
    return cfg, st, clock, np.ascontiguousarray(z["dT2m"][:WAVE]), np.ascontiguousarray(z["precip_scale"][:WAVE])


def columns(st, idx):
    return State(np.ascontiguousarray(st.lay[:, :, idx]), np.ascontiguousarray(st.scal[:, idx]), np.ascontiguousarray(st.n_active[idx]))


def repeated(st, times):
    """column b of st, `times` times in a row, for every b"""
    return State(np.ascontiguousarray(np.repeat(st.lay, times, axis=2)), np.ascontiguousarray(np.repeat(st.scal, times, axis=1)),
                 np.ascontiguousarray(np.repeat(st.n_active, times)))


def with_first_columns_again(st, extra):
    """st and its first `extra` columns once more behind it"""
    idx = np.concatenate([np.arange(st.ncol), np.arange(extra)])
    return columns(st, idx), idx


# ------------------------------------------------------------------ the iteration, restated
def _T_freeze_of(S_bu):
    T = -1.0
    while abs(S_br(T) / S_bu - 1.0) > float(np.float32(0.0001)):
        T = T - (S_br(T) - S_bu) / ddT_S_br(T)
    return T


def _eval(H, S_bu, T_0, floor):
    sb = S_br(T_0)
    f = -LATENT_HEAT - H + LATENT_HEAT * S_bu / max(sb, floor) + C_S * T_0 + C_S_BETA * T_0 * T_0 / 2.0
    df = C_S + C_S_BETA * T_0 - LATENT_HEAT * S_bu * ddT_S_br(T_0) / max(sb * sb, 1.0e-10)
    return f, T_0 - f / df, sb


def getT(H, S_bu, T_in):
    """(T, evaluations, flags) of one layer; flags: the ways in which the layer is not the fast loop's"""
    flags = set()
    Tl = H / C_L
    if max(S_br(Tl), S_bu) > S_bu and S_bu > 0.001:
        f, T, sb = _eval(H, S_bu, T_in, 1.0e-9)
        if not sb > 1.0e-4:
            flags.add("tiny")
        n = 1
        while abs(f) > 1.0:
            T_0 = T
            if T_0 > 0.0 or T_0 < -200.0:
                flags.add("leave")
                T_0 = _T_freeze_of(S_bu)
            f, T, sb = _eval(H, S_bu, T_0, 1.0e-10)
            if not sb > 1.0e-4:
                flags.add("tiny")
            n += 1
            if n > 260:
                flags.add("stop99")
                break
        return T, n, flags
    if S_bu < 0.001:
        flags.add("fresh")
        if H > 0.0:
            return Tl, 0, flags
        if H <= -LATENT_HEAT:
            return (H + LATENT_HEAT) / C_S, 0, flags
        return 0.0, 0, flags
    flags.add("brine")
    return Tl, 0, flags


def sweep(cfg, st):
    """one getT sweep, bottom to top, over every column of st: (evals[nlayer, ncol] (-1: the lane sits the layer out), flags[nlayer][ncol])"""
    nl, nc = st.nlayer, st.ncol
    evals = np.full((nl, nc), -1, dtype=np.int64)
    flags = [[set() for _ in range(nc)] for _ in range(nl)]
    H_abs, S_abs, m = st.arr("H_abs"), st.arr("S_abs"), st.arr("m")
    for c in range(nc):
        T_test = cfg.T_bottom
        for k in range(int(st.n_active[c]) - 1, -1, -1):
            T_test, evals[k, c], flags[k][c] = getT(H_abs[k, c] / m[k, c], S_abs[k, c] / m[k, c], T_test)
    return evals, flags
