"""The two wave-level votes of the fused up sweep, restated in numpy.

  bound     s1_layer (samsim_amd/csrc/samsim_sweeps_fused.h) stores a sparse row of the Rayleigh-number array only when some lane of
            the wave exceeds ray_crit.  It decides most rows without the number: with P = c * d_S_br * height * (st + bot) and
            Q = ray_crit * (1 - 2**-20) * (stp + botterm), a lane with P < Q, or with minp < 1e-14 (hp = 0), is below (the last
            constant of c, 1 / (kappa_l * mu), is carried on Q's side as kappa_l * mu).
  shortcut  getT_chain (samsim_thermo.h) takes `above` (the liquidus salinity at H/c_l exceeds S_bu) as true for the whole wave
            where every lane has H/c_l < -3 and S_bu < 40.

`first_sweep` walks the columns of a State bottom to top as the first sweep does (mo_grotz.f90:297-307, mo_grav_drain.f90:103-136)
and returns, per layer and column, the Rayleigh number, the operands of the bound and of the shortcut.  Rows are the device's: layer k
of 64 consecutive columns.
"""
import numpy as np

from samsim_amd import testcases as tcs

WAVE = 64
RAY_CRIT = 4.89
MARGIN = 2.0 ** -20
SALTS = {1: (-18.7, -0.519, -0.00535), 2: (-17.6, -0.389, -0.00362)}   # func_S_br, mo_thermo_functions.f90:324-326 / :343-345
GRAV_F = float(np.float32(9.8061))
RHO_S, RHO_L, C_L, K_L = 920.0, tcs.RHO_L, tcs.C_L, 0.523
BBETA = 0.8 * float(np.float32(1e-3))
MU = 2.55 * float(np.float32(1e-3))
KAPPA_L = K_L / RHO_L / C_L
PSI_S_MIN = 0.05
P17, P14 = 10.0 ** -17.0, 10.0 ** -14.0
C_PRODUCT = GRAV_F * RHO_L * BBETA          # the constants of the product, folded as the compiler folds them
C_RAY = C_PRODUCT * (1.0 / (KAPPA_L * MU))  # all constants of the Rayleigh number
Q_RAY = RAY_CRIT * (1.0 - MARGIN)
T_SHORT, S_SHORT = -3.0, 40.0


def S_br_poly(T, salt=1):
    c2, c3, c4 = SALTS[salt]
    return T * (c2 + T * (c3 + T * c4))


def ray_of(d_S_br, height, h_sum, h_den, minp):
    """the Rayleigh number as s1_layer forms it (harmonic_flag 2)"""
    with np.errstate(all="ignore"):
        hp = np.where(minp < P14, 0.0, h_sum / h_den)
        ray = C_PRODUCT * d_S_br * height * hp
        ray = ray * (1.0 / (KAPPA_L * MU))
    return np.where(ray > 0.0, ray, 0.0)


def bound_below(d_S_br, height, h_sum, h_den, minp, margin=MARGIN, minp_case=True):
    """the lane is below ray_crit by the division-free bound (a NaN operand fails the compare)"""
    with np.errstate(all="ignore"):
        P = C_PRODUCT * d_S_br * height * h_sum                       # (begins with the two products ray_of begins with)
        Q = RAY_CRIT * (1.0 - margin) * (KAPPA_L * MU) * h_den
        below = P < Q
    return below | (minp < P14) if minp_case else below


def shortcut_lane(Tl, S_bu, s_limit=S_SHORT):
    with np.errstate(all="ignore"):
        return (Tl < T_SHORT) & (S_bu < s_limit)


def first_sweep(st, salt=1):
    """dict of [nlayer, ncol] arrays over a State with T and phi (what get_state returns): `inner` = the lane has the layer and it is
    not its bottom layer (where the Rayleigh number exists), `active` = the lane has the layer; ray, the bound's operands d_S_br,
    height, h_sum, h_den, minp; Tl = H / c_l and S_bu"""
    nl, nc = st.nlayer, st.ncol
    na = st.n_active.astype(np.int64)
    H_abs, S_abs, m, thick, T, phi = (st.arr(n) for n in ("H_abs", "S_abs", "m", "thick", "T", "phi"))
    out = {n: np.zeros((nl, nc)) for n in ("ray", "d_S_br", "height", "h_sum", "h_den", "minp", "Tl", "S_bu")}
    out["inner"] = np.zeros((nl, nc), dtype=bool)
    out["active"] = np.arange(nl)[:, None] < na[None, :]
    minp = np.full(nc, 1.0e300)
    stp, s_t, bot, botterm, S_br_bot = (np.zeros(nc) for _ in range(5))
    with np.errstate(all="ignore"):
        for k in range(nl - 1, -1, -1):       # 0-based layer
            act = k < na
            mk = np.where(act, m[k], 1.0)
            th = np.where(act, thick[k], 1.0)
            S_bu = S_abs[k] / mk
            out["S_bu"][k] = S_bu
            out["Tl"][k] = (H_abs[k] / mk) * (1.0 / C_L)
            S_br = np.maximum(S_br_poly(T[k], salt), S_bu)
            V_s, V_l = mk * phi[k] * (1.0 / RHO_S), mk * (1.0 - phi[k]) * (1.0 / RHO_L)
            V_ex = np.maximum(V_l + V_s - th, 0.0)
            psi_s, psi_l = V_s / th, np.maximum((V_l - V_ex) / th, 0.0)
            perm = P17 * np.power(1000.0 * np.abs(psi_l), 3.1)
            is_bot = act & (k == na - 1)
            inner = act & ~is_bot
            b = th * psi_s / PSI_S_MIN
            S_br_bot = np.where(is_bot, S_br, S_br_bot)
            bot = np.where(is_bot, b, bot)
            botterm = np.where(is_bot, b / perm, botterm)
            height = s_t + bot
            minp = np.where(inner, np.minimum(minp, perm), minp)
            stp = np.where(inner, stp + th / perm, stp)
            s_t = np.where(inner, s_t + th, s_t)
            d = S_br - S_br_bot
            h_sum, h_den = s_t + bot, stp + botterm
            out["inner"][k] = inner
            for n, v in (("d_S_br", d), ("height", height), ("h_sum", h_sum), ("h_den", h_den), ("minp", minp)):
                out[n][k] = np.where(inner, v, 0.0)
            out["ray"][k] = np.where(inner, ray_of(d, height, h_sum, h_den, minp), 0.0)
    return out


def rows(mask_lane, lanes):
    """[nlayer, nwave]: the predicate holds in every lane of `lanes` of the row (a row without such a lane is not counted: None-like
    rows are returned False in `any_lane`); returns (all_of, any_lane)"""
    nl, nc = mask_lane.shape
    pad = (-nc) % WAVE
    a = np.pad(mask_lane | ~lanes, ((0, 0), (0, pad)), constant_values=True).reshape(nl, -1, WAVE).all(axis=2)
    e = np.pad(lanes, ((0, 0), (0, pad)), constant_values=False).reshape(nl, -1, WAVE).any(axis=2)
    return a & e, e


def row_any(mask_lane):
    nl, nc = mask_lane.shape
    pad = (-nc) % WAVE
    return np.pad(mask_lane, ((0, 0), (0, pad)), constant_values=False).reshape(nl, -1, WAVE).any(axis=2)
