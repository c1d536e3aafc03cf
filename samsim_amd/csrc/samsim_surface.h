// samsim_surface.h -- what happens above the ice and at its surface: the snow cover (snow_coupling*, snow_fall, snow_block), the
// radiation header and the surface energy balance (radiation_header, radiative_T_top, surface_flux), the melt film (sub_melt_thick).
// Part of the translation unit samsim_kernels.hip: expects samsim_step_types.h (`c`, `x`, `g`; CL, GS, LAY, CFG, STOPC) and samsim_thermo.h.
#ifndef SAMSIM_SURFACE_H
#define SAMSIM_SURFACE_H

namespace {

// ---------------------------------------------------------------- snow, mo_snow.f90
// snow_coupling, mo_snow.f90:61-104.  The reference passes T_snow / T as both the guess and the result of getT;
// by-reference argument passing makes the guess H/c_l (getT's first statement overwrites it).
// (core: the top layer's enthalpy, temperature and solid fraction in registers -- the fused down sweep calls it between the
// brine expulsion and the drainage of layer 1; the wrapper below works on the arrays, as the unfused order and the up sweep do)
template <class K>
__device__ RARE int snow_coupling_core(Col &c, const Ctx &x, double &H_abs, const double m, const double S_bu, double &T, double &phi) {
  const Salt &s = x.salt;
  double H;
  const double m_snow = CL(m_snow), S_abs_snow = GS(S_ABS_SNOW);
  double phi_sn = GS(PHI_S);
  int rc = 0;
  H_abs = H_abs + m_snow * latent_heat + CL(H_abs_snow);
  CL(H_abs_snow) = -m_snow * latent_heat;
  H = H_abs / m;
#define COUPLE_GETT()                                                                                      \
  do {                                                                                                     \
    double hs = CL(H_abs_snow) / m_snow;                                                                     \
    double T_sn = CL(T_snow);                                                                              \
    rc |= getT(s, hs, S_abs_snow / m_snow, hs / c_l, T_sn, phi_sn);                                        \
    CL(T_snow) = T_sn;                                                                                     \
    rc |= getT(s, H, S_bu, H / c_l, T, phi);                                                               \
  } while (0)
  COUPLE_GETT();
  if (T > 0.0 && H_abs <= -CL(H_abs_snow)) {
    CL(H_abs_snow) = CL(H_abs_snow) + H_abs;
    H_abs = 0.0;
    COUPLE_GETT();
  } else if (T > 0.0 && H_abs > -CL(H_abs_snow)) {
    H_abs = (H_abs + CL(H_abs_snow)) * m / m_snow / (1.0 + m / m_snow);
    CL(H_abs_snow) = H_abs * m_snow / m;
    COUPLE_GETT();
  } else {
    int jj = 0;
    while (fabs(T - CL(T_snow)) > (double)0.1f && jj < 201) {
      double d = CL(T_snow) - (CL(T_snow) + T) / 2.0;
      double sg = dmax(fabs(d), 0.1);
      if (signbit(d)) sg = -sg;
      CL(H_abs_snow) = CL(H_abs_snow) - sg * c_s * m_snow;
      H_abs = H_abs + sg * c_s * m_snow;
      jj = jj + 1;
      H = H_abs / m;
      COUPLE_GETT();
    }
    if (jj > 200 && fabs(T - CL(T_snow)) > 1.0) rc = 16;
  }
#undef COUPLE_GETT
  GS(PHI_S) = phi_sn;
  return rc ? (rc == 16 ? 16 : 99) : 0;
}
template <class K>
__device__ RARE void snow_coupling(Col &c, const Ctx &x) {
  double H_abs = LAY(SAMSIM_A_H_ABS, 1), T = LAY(SAMSIM_A_T, 1), phi = LAY(SAMSIM_A_PHI, 1);
  const int rc = snow_coupling_core<K>(c, x, H_abs, LAY(SAMSIM_A_M, 1), LAY(SAMSIM_A_S_BU, 1), T, phi);
  LAY(SAMSIM_A_H_ABS, 1) = H_abs;
  LAY(SAMSIM_A_T, 1) = T;
  LAY(SAMSIM_A_PHI, 1) = phi;
  if (rc) STOPC(rc, 1);
}

// snow_precip (mo_snow.f90:123-150) and snow_precip_0 (:167-192), called from mo_grotz.f90:251-265
template <class K>
__device__ __forceinline__ void snow_fall(Col &c, const Ctx &x) {
  const samsim_config &g = x.p->cfg;
  if (!(dmax(CL(liquid_precip), CL(solid_precip)) > 0.0)) return;
  const double dt = g.dt, T2m = CL(T2m);
  double solid, liquid;
  if (CFG(precip_flag) == 0) { solid = CL(solid_precip); liquid = CL(liquid_precip); }
  else if (T2m > 0.0) { solid = 0.0; liquid = CL(liquid_precip); }
  else { solid = CL(liquid_precip); liquid = 0.0; }
  if (c.Na > 1) {
    double d_thick = dt * solid * rho_l / rho_snow;
    CL(m_snow) = CL(m_snow) + dt * rho_l * (liquid + solid);
    CL(thick_snow) = CL(thick_snow) + d_thick;
    CL(H_abs_snow) = CL(H_abs_snow) + dt * T2m * liquid * rho_l * c_l;
    CL(H_abs_snow) = CL(H_abs_snow) + dt * dmin(T2m, -1.0) * solid * rho_l * c_s;
    CL(H_abs_snow) = CL(H_abs_snow) - dt * solid * rho_l * latent_heat;
  } else {
    double H_abs = LAY(SAMSIM_A_H_ABS, 1), S_abs = LAY(SAMSIM_A_S_ABS, 1);
    const double m = LAY(SAMSIM_A_M, 1), T = LAY(SAMSIM_A_T, 1);
    H_abs = H_abs + (liquid + solid) * (T2m - T) * dt;
    H_abs = H_abs - solid * latent_heat * dt;
    S_abs = S_abs - (liquid + solid) * S_abs / m * dt;
    LAY(SAMSIM_A_H_ABS, 1) = H_abs;
    LAY(SAMSIM_A_S_ABS, 1) = S_abs;
  }
}

// snow_thermo (mo_snow.f90:212-320) / snow_thermo_meltwater (:331-454) wrapped in the block of
// mo_grotz.f90:273-292 and :604-624
template <class K>
__device__ RARE void snow_block(Col &c, const Ctx &x) {
  const samsim_config &g = x.p->cfg;
  // (psi_l_snow, psi_g_snow and S_abs_snow are only read by this routine and by rare events -- flooding, the melting of a thin
  // cover, melt water from the snow: they live in the scalar block, which is written where a value changes)
  if (!(CL(thick_snow) > 0.0)) {
    if ((c.flags & COLF_RESTART) || CL(m_snow) != 0.0 || CL(thick_snow) != 0.0 || CL(psi_s_snow) != 0.0 || CL(H_abs_snow) != 0.0) {   // the cover has just gone (or the state is new)
      GS(PSI_L_SNOW) = 0.0; GS(PSI_G_SNOW) = 0.0; GS(S_ABS_SNOW) = 0.0;
    }
    CL(thick_snow) = 0.0; CL(m_snow) = 0.0; CL(psi_s_snow) = 0.0;
    CL(H_abs_snow) = 0.0; CL(melt_thick_snow) = 0.0;
    return;
  }
  double psi_l_sn, psi_g_sn;
  const double S_abs_sn = GS(S_ABS_SNOW);
  CL(melt_thick_snow) = 0.0;
  const bool meltwater = (CFG(snow_flush_flag) == 1);
  double m = LAY(SAMSIM_A_M, 1), thick = LAY(SAMSIM_A_THICK, 1), H_abs = LAY(SAMSIM_A_H_ABS, 1);
  bool touched = false;
  double phi_snow = 0.0, max_lwc, max_lwc_v, sat_snow;
  const double H_snow = quot(CL(H_abs_snow), CL(m_snow)), S_bu_snow = quot(S_abs_sn, CL(m_snow)), psi_s_old = CL(psi_s_snow);
  const double T_in = CL(T_snow);
  double T_sn = T_in;
  int rc = getT(x.salt, H_snow, S_bu_snow, T_in, T_sn, phi_snow);
  CL(T_snow) = T_sn;
  if (rc) STOPC(99, 0);
  CL(psi_s_snow) = quot(quot(CL(m_snow) * phi_snow, rho_s), CL(thick_snow));
  psi_l_sn = quot(quot(CL(m_snow) * (1.0 - phi_snow), rho_l), CL(thick_snow));
  if (CL(psi_s_snow) + psi_l_sn > 1.0) {
    CL(thick_snow) = CL(m_snow) * (phi_snow / rho_s + (1.0 - phi_snow) / rho_l);
    CL(psi_s_snow) = CL(m_snow) * phi_snow / rho_s / CL(thick_snow);
    psi_l_sn = CL(m_snow) * (1.0 - phi_snow) / rho_l / CL(thick_snow);
    if (fabs(CL(psi_s_snow) + psi_l_sn - 1.0) > 0.0000001) { GS(PSI_L_SNOW) = psi_l_sn; STOPC(345, 0); }
  }
  psi_g_sn = 1.0 - CL(psi_s_snow) - psi_l_sn;
  if (CL(psi_s_snow) > 0.0) max_lwc = quot(0.057 * (1.0 - CL(psi_s_snow)), CL(psi_s_snow)) + 0.017;
  else max_lwc = 0.0;

  if (psi_s_old > CL(psi_s_snow) && CL(psi_s_snow) > 0.0) {
    if ((1.0 - phi_snow) > max_lwc) CL(thick_snow) = CL(thick_snow) * (1.0 - (psi_s_old - CL(psi_s_snow)) / psi_s_old);
    double tmin = (phi_snow * CL(m_snow) / rho_s + (1.0 - phi_snow) * CL(m_snow) / rho_l);
    if (CL(thick_snow) < tmin) CL(thick_snow) = tmin;
    CL(psi_s_snow) = CL(m_snow) * phi_snow / rho_s / CL(thick_snow);
    psi_l_sn = CL(m_snow) * (1.0 - phi_snow) / rho_l / CL(thick_snow);
    psi_g_sn = 1.0 - CL(psi_s_snow) - psi_l_sn;
    psi_g_sn = fabs(psi_g_sn);
  } else if (CL(psi_s_snow) < 0.000001) {
    CL(thick_snow) = CL(m_snow) / rho_l;
    CL(psi_s_snow) = 0.0; psi_g_sn = 0.0; psi_l_sn = 1.0;
  }

  const bool wet = (1.0 - phi_snow) > max_lwc && psi_g_sn > 0.0 && (!meltwater || psi_l_sn > 0.0);
  if (wet) {
    touched = true;
    const double T_snow = CL(T_snow), pss = CL(psi_s_snow);
    max_lwc_v = max_lwc * CL(m_snow) / (rho_l * CL(thick_snow));
    if (!meltwater) {
      sat_snow = CL(thick_snow) * (psi_l_sn - max_lwc_v);
      sat_snow = sat_snow / (1.0 - pss - max_lwc_v - dmin(gas_snow_ice2, psi_g_sn));
      CL(thick_snow) = CL(thick_snow) - sat_snow;
      thick = thick + sat_snow;
      CL(m_snow) = CL(m_snow) - sat_snow * (pss * rho_s + (1.0 - pss - gas_snow_ice2) * rho_l);
      m = m + sat_snow * (pss * rho_s + (1.0 - pss - gas_snow_ice2) * rho_l);
      CL(H_abs_snow) = CL(H_abs_snow) - sat_snow * pss * rho_s * c_s * T_snow;
      H_abs = H_abs + sat_snow * pss * rho_s * c_s * T_snow;
      CL(H_abs_snow) = CL(H_abs_snow) + sat_snow * pss * rho_s * latent_heat;
      H_abs = H_abs - sat_snow * pss * rho_s * latent_heat;
      CL(H_abs_snow) = CL(H_abs_snow) - sat_snow * (1.0 - pss) * rho_l * c_l * T_snow;
      H_abs = H_abs + sat_snow * (1.0 - pss) * rho_l * c_l * T_snow;
    } else {
      const double ksf = g.k_snow_flush;
      double slush = (psi_l_sn - max_lwc_v) * (1.0 - ksf);
      double flush = (psi_l_sn - max_lwc_v) * ksf;
      CL(melt_thick_snow) = CL(thick_snow) * flush;
      sat_snow = CL(thick_snow) * (slush);
      sat_snow = sat_snow / (1.0 - pss - max_lwc_v - dmin(gas_snow_ice2, psi_g_sn));
      const double gmin = dmin(gas_snow_ice2, psi_g_sn);
      CL(thick_snow) = CL(thick_snow) - sat_snow - CL(melt_thick_snow);
      thick = thick + sat_snow;
      CL(m_snow) = CL(m_snow) - sat_snow * (pss * rho_s + (1.0 - pss - gmin) * rho_l) - CL(melt_thick_snow) * rho_l;
      m = m + sat_snow * (pss * rho_s + (1.0 - pss - gmin) * rho_l);
      CL(H_abs_snow) = CL(H_abs_snow) - sat_snow * pss * rho_s * c_s * T_snow;
      H_abs = H_abs + sat_snow * pss * rho_s * c_s * T_snow;
      CL(H_abs_snow) = CL(H_abs_snow) + sat_snow * pss * rho_s * latent_heat;
      H_abs = H_abs - sat_snow * pss * rho_s * latent_heat;
      CL(H_abs_snow) = CL(H_abs_snow) - sat_snow * (1.0 - pss - gmin) * rho_l * c_l * T_snow - CL(melt_thick_snow) * rho_l * c_l * T_snow;
      H_abs = H_abs + sat_snow * (1.0 - pss - gmin) * rho_l * c_l * T_snow;
    }
  } else if (psi_g_sn <= 0.0) {
    touched = true;
    H_abs = H_abs + CL(H_abs_snow); m = m + CL(m_snow); thick = thick + CL(thick_snow);
    CL(H_abs_snow) = 0.0; CL(m_snow) = 0.0; CL(thick_snow) = 0.0;
    psi_g_sn = 0.0; CL(psi_s_snow) = 0.0; psi_l_sn = 0.0;
  }
  if (touched) {
    LAY(SAMSIM_A_M, 1) = m;
    LAY(SAMSIM_A_THICK, 1) = thick;
    LAY(SAMSIM_A_H_ABS, 1) = H_abs;
  }
  GS(PSI_L_SNOW) = psi_l_sn;
  GS(PSI_G_SNOW) = psi_g_sn;
  if (psi_g_sn < 0.0) STOPC(9876, 0);
}

// ---------------------------------------------------------------- surface energy balance, mo_heat_fluxes.f90:77-195
// sets fl_Q(1), T_top, fl_Q_snow, albedo, fl_sw, fl_lw, T_freeze; returns the Beer-law surface value temp2
// K::general = false: the instantiation for the primary configurations (forcing tables or cooling plate, grav_flag 1/2, flush_flag
// 1/5, flood_flag 1/2, testcases without layer-array specifics); the secondary parametrisations compile away there.
template <class K>
__device__ __forceinline__ double radiation_header(Col &c, const Ctx &x, double time, int tc) {
  const samsim_config &g = x.p->cfg;
  if (CFG(boundflux_flag) != 2) return 0.0;
  CL(albedo) = func_albedo(CL(thick_snow), CL(T_snow), c.psi_l_top, g.thick_min, CFG(albedo_flag));
  if (!K::general || CFG(atmoflux_flag) == 2) {
    if (time == time_input(tc)) {
      CL(fl_sw) = x.f_sw[x.soff + tc - 1];
      CL(fl_lw) = x.f_lw[x.soff + tc - 1];
    } else {
      const double temp = (time - time_input(tc - 1)) / (time_input(tc) - time_input(tc - 1));
      CL(fl_sw) = (1.0 - temp) * x.f_sw[x.soff + tc - 2] + temp * x.f_sw[x.soff + tc - 1];
      CL(fl_lw) = (1.0 - temp) * x.f_lw[x.soff + tc - 2] + temp * x.f_lw[x.soff + tc - 1];
    }
  } else if (CFG(atmoflux_flag) == 1) {
    // sub_notzflux(time + 180 days), mo_functions.f90:270-289 (47.9, 53.1 are default-REAL literals); fl_rest lives in
    // the scalar block (atmoflux_flag 3 leaves fl_sw and fl_rest as the caller set them)
    double day = (time + 86400.0 * 180.0) / 86400.0;
    while (day > 360.0) day = day - 360.0;
    const double a = (day - 164.0) / (double)47.9f, b = (day - 206.0) / (double)53.1f;
    CL(fl_sw) = 314.0 * exp(-0.5 * (a * a));
    if (day < 60.0 || day > 300.0) CL(fl_sw) = 0.0;
    GSI(SAMSIM_S_FL_REST) = 118.0 * exp(-0.5 * (b * b)) + 179.0;
  }
  const double pen = (CL(thick_snow) < g.thick_min) ? penetr : 0.0;
  return pen * (1.0 - CL(albedo)) * CL(fl_sw);
}

// twice-iterated linearised radiative balance for the surface temperature, mo_heat_fluxes.f90:115-148: a function of the
// forcing, the albedo, and the temperature of the snow (or of the top layer under thin / no snow)
__device__ __forceinline__ double radiative_T_top(const Col &c, double fl_rest, double T1, double thick_min) {
  double T_old = (CL(thick_snow) < thick_min) ? T1 : CL(T_snow);
  const double emi = (CL(thick_snow) < thick_min) ? emissivity_ice : emissivity_snow;
  const double pen = (CL(thick_snow) < thick_min) ? penetr : 0.0;
  T_old = T_old + zeroK;
  double temp1 = (1.0 - CL(albedo)) * (1.0 - pen) * CL(fl_sw) + fl_rest;
  temp1 = temp1 + emi * 3.0 * sigma * pow_4(T_old);
  temp1 = quot(temp1, emi * 4.0 * sigma * (T_old * T_old * T_old));
  temp1 = temp1 - zeroK;
  T_old = temp1 + zeroK;
  temp1 = (1.0 - CL(albedo)) * (1.0 - pen) * CL(fl_sw) + fl_rest;
  temp1 = temp1 + emi * 3.0 * sigma * pow_4(T_old);
  temp1 = quot(temp1, emi * 4.0 * sigma * (T_old * T_old * T_old));
  temp1 = temp1 - zeroK;
  return temp1;
}

template <class K>
__device__ __forceinline__ void surface_flux(Col &c, const Ctx &x) {
  const samsim_config &g = x.p->cfg;
  const int Na = c.Na;
  const double psi_s1 = LAY(SAMSIM_A_PSI_S, 1), psi_l1 = LAY(SAMSIM_A_PSI_L, 1), psi_g1 = LAY(SAMSIM_A_PSI_G, 1);
  const double thick1 = LAY(SAMSIM_A_THICK, 1), T1 = LAY(SAMSIM_A_T, 1);
  const double k1 = psi_s1 * k_s + psi_l1 * k_l + psi_g1 * 0.0;
  if (CFG(boundflux_flag) == 1) {  // cooling plate, mo_heat_fluxes.f90:77-87
    double fl = (T1 - CL(T_top)) / (thick1 / (2.0 * k1));
    if (fabs(fl) > g.max_flux_plate) fl = fl / fabs(fl) * g.max_flux_plate;
    CL(fl_Q1) = fl;
    return;
  }
  if (K::general && CFG(boundflux_flag) == 3) {  // lab air temperature, mo_heat_fluxes.f90:202-219 (lab_snow_flag 0)
    GS(T_FREEZE) = dmin(func_T_freeze(LAY(SAMSIM_A_S_ABS, Na) / LAY(SAMSIM_A_M, Na), CFG(salt_flag), x.tf_c3), 0.0);
    CL(T_top) = T1;
    CL(fl_Q1) = g.alpha_flux_instable * (CL(T_top) - CL(T2m));
    if (CL(fl_Q1) < 0.0) {
      CL(T_top) = dmax(GS(T_FREEZE), T1);
      CL(fl_Q1) = g.alpha_flux_stable * (CL(T_top) - CL(T2m));
    }
    return;
  }
  // boundflux_flag 2, mo_heat_fluxes.f90:91-195
  const double thick_min = g.thick_min;
  const double fl_rest = (!K::general || CFG(atmoflux_flag) == 2) ? CL(fl_lw) + 0.0 + 0.0 : GSI(SAMSIM_S_FL_REST);
  const double emi = (CL(thick_snow) < thick_min) ? emissivity_ice : emissivity_snow;
  const double pen = (CL(thick_snow) < thick_min) ? penetr : 0.0;
  double temp1;
  CL(T_top) = radiative_T_top(c, fl_rest, T1, thick_min);

  double Tf;
  if (CL(thick_snow) >= thick_min / 100.0) Tf = 0.0;
  else Tf = func_T_freeze(quot(LAY(SAMSIM_A_S_ABS, 1), LAY(SAMSIM_A_M, 1)), CFG(salt_flag), x.tf_c3);

  GS(T_FREEZE) = Tf;

  const double k_snow = (CL(thick_snow) >= thick_min / 100.0) ? func_k_snow(CL(m_snow), CL(thick_snow)) : 0.0;
  // sub_fl_Q_snow, mo_snow.f90:498-518
  const double flq_snow_ice = quot(T1 - CL(T_snow), quot(CL(thick_snow), 2.0 * k_snow) + quot(thick1, 2.0 * (psi_s1 * k_s + psi_l1 * k_l)));
  if (CL(T_top) > Tf && Na > 1) {
    temp1 = emi * sigma * pow_4(Tf + zeroK) - (1.0 - CL(albedo)) * (1.0 - pen) * CL(fl_sw) - fl_rest;
    if (CL(thick_snow) >= thick_min) { CL(fl_Q_snow) = temp1; CL(fl_Q1) = flq_snow_ice; }
    else if (CL(thick_snow) >= thick_min / 100.0) { CL(fl_Q_snow) = temp1; CL(fl_Q1) = 0.0; }
    else CL(fl_Q1) = temp1;
    CL(T_top) = Tf;
  } else {
    if (CL(thick_snow) >= thick_min) {
      CL(fl_Q1) = flq_snow_ice;
      CL(fl_Q_snow) = quot(CL(T_snow) - CL(T_top), quot(CL(thick_snow), 2.0 * k_snow));  // sub_fl_Q_0_snow, mo_snow.f90:528-546
    } else if (CL(thick_snow) > thick_min / 100.0 && CL(thick_snow) < thick_min) {
      CL(fl_Q1) = 0.0;
      // sub_fl_Q_0_snow_thin, mo_snow.f90:466-487
      double k = CL(thick_snow) / (CL(thick_snow) + thick1) * k_snow + thick1 / (CL(thick_snow) + thick1) * k1;
      CL(fl_Q_snow) = (CL(T_snow) - CL(T_top)) / ((CL(thick_snow) + thick1) / (2.0 * k));
    } else {
      CL(fl_Q1) = (T1 - CL(T_top)) / (thick1 / (2.0 * k1));
    }
  }
}

// ---------------------------------------------------------------- melt film, mo_functions.f90:386-474
__device__ __forceinline__ void sub_melt_thick(double psi_l, double psi_s, double psi_g, double T, double T_freeze, double T_top, double fl_Q,
                               double thick_snow, double dt, double &melt_thick, double &thick, double thick_min) {
  melt_thick = 0.0;
  if (thick_snow < thick_min && T_top >= T_freeze) {
    melt_thick = -fl_Q - 2.0 * (psi_l * k_l + psi_s * k_s) / thick * (T_freeze - T);
    melt_thick = melt_thick * dt / dmax(latent_heat * rho_s * psi_s, 0.000000000000001);
    melt_thick = dmin(psi_l * thick, melt_thick);
  }
  if (psi_s < psi_s_top_min) melt_thick = thick * (1.0 - psi_s / psi_s_top_min);
  if (melt_thick > 0.0 && psi_g > gas_snow_ice2) {
    if (melt_thick > (psi_g - gas_snow_ice2) * thick) {
      melt_thick = melt_thick - (psi_g - gas_snow_ice2) * thick;
      thick = thick * (1.0 - (psi_g - gas_snow_ice2));
    } else {
      thick = thick - melt_thick;
      melt_thick = 0.0;
    }
  }
}

}  // namespace

#endif
