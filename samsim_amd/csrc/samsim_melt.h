// samsim_melt.h -- the passes of the melt season: func_freeboard, flooding (flood_core / flood / flood_simple, refresh_ray_top), flushing
// (flush3, flush4) and the prescribed salinity profile.  Part of the translation unit samsim_kernels.hip: expects samsim_step_types.h
// (`c`, `x`, `g`; CL, GS, LAY, SPEC, CFG, STOPC, THICK_AT, RARE_CHUNK) and samsim_thermo.h.
#ifndef SAMSIM_MELT_H
#define SAMSIM_MELT_H

namespace {

// ---------------------------------------------------------------- func_freeboard, mo_functions.f90:79-130
// O(N): one pass for the column totals, one pass for the waterline search with prefix sums (the reference
// recomputes the suffix sums for every candidate layer).
template <class K>
__device__ RARE double func_freeboard(Col &c, const Ctx &x) {
  const int Na = c.Na;
  double snowmass = ((K::fixed ? K::freeboard_snow_flag : x.p->cfg.freeboard_snow_flag) == 0) ? CL(m_snow) : 0.0;
  THICK_RULE_INIT(tr);
  // The column totals SUM(psi_s*thick) and SUM(psi_g*thick): the sweep that stored the volume-fraction rows (sweep_down_fused,
  // sweep_expulsion_transfer, refill_psi_rows) summed them over layers 2..N_active as it went, top -> bottom like the reference's
  // SUM, and left the two sums in the hand-over block; layer 1 -- whose thickness snow slush, the melt film and melt water may have
  // changed since -- is added here with what it holds now.  (Round 2 walked the whole column for them: two rows per layer-cell in
  // every step of a melt season.)
  const double th1 = LAY(SAMSIM_A_THICK, 1);
  const double A = LAY(SAMSIM_A_PSI_S, 1) * th1 + ((Na >= 2) ? SPEC(SP_FB_A2) : 0.0);
  const double G = LAY(SAMSIM_A_PSI_G, 1) * th1 + ((Na >= 2) ? SPEC(SP_FB_G2) : 0.0);
  double buoy = A * (rho_l - rho_s) + G * rho_l;
  double freeboard;
  if (snowmass > buoy) {
    freeboard = (buoy - snowmass) / rho_l;
  } else {
    double Ap = 0.0, Gp = 0.0, Mp = 0.0, Tp = 0.0;  // prefix sums over 1..k-1
    double test2 = 0.0, mk = 0.0, thk = 1.0;
    bool done = false;
    for (int k0 = 1; !done; k0 += RARE_CHUNK) {
      double m_[RARE_CHUNK], th_[RARE_CHUNK], ps_[RARE_CHUNK], pg_[RARE_CHUNK];
#pragma unroll
      for (int i = 0; i < RARE_CHUNK; ++i) {
        const int kk = (k0 + i <= c.N) ? k0 + i : c.N;
        m_[i] = LAY(SAMSIM_A_M, kk); th_[i] = THICK_AT(tr, kk);
        ps_[i] = LAY(SAMSIM_A_PSI_S, kk); pg_[i] = LAY(SAMSIM_A_PSI_G, kk);
      }
#pragma unroll
      for (int i = 0; i < RARE_CHUNK; ++i) {
        if (!done) {
          const int k = k0 + i;
          mk = m_[i];
          thk = th_[i];
          double a = ps_[i] * thk, g = pg_[i] * thk;
          // buoyancy of the layers below k, mass of layers 1..k
          test2 = (k == Na) ? 0.0 : ((A - (Ap + a)) * (rho_l - rho_s) + (G - (Gp + g)) * rho_l);
          double test1 = (Mp + mk) + snowmass;
          if (!(test1 < test2) || k >= Na) done = true;
          else { Ap += a; Gp += g; Mp += mk; Tp += thk; }
        }
      }
    }
    double test1 = Mp + snowmass;
    freeboard = test2 - test1 + (rho_l - mk / thk) * thk;
    freeboard = freeboard / rho_l;
    freeboard = freeboard + Tp;
  }
  return freeboard;
}

// ---------------------------------------------------------------- flood, mo_flood.f90:55-151
// The arithmetic of flood on the two layers it touches, held in registers: layer 1 (S1, H1, m1, th1) and layer N_active (SN, HN, mN,
// TN: read; its increments incS, incH are returned, applied where `deep` -- the instant flooding below neg_free), and the snow
// (in LDS).  flood() below runs it on the arrays (the unfused order); the fused order on what its dry run of the expulsion returned.
struct FloodEnds { double S1, H1, m1, th1, SN, HN, mN, TN, incS, incH; bool deep; };
template <class K>
__device__ __forceinline__ double flood_core(Col &c, const Ctx &x, double hp, double sall, FloodEnds &e) {
  const samsim_config &g = x.p->cfg;
  const double freeboard = GS(FREEBOARD), psi_g_snow = GS(PSI_G_SNOW);
  double flood_brine = -g.dt * grav_f * rho_l * rho_l * hp * (freeboard) / (mu * sall);
  const double shift_ice = flood_brine / (rho_l * psi_g_snow / ratio_flood);
  const double shift_snow = shift_ice * (1 + psi_g_snow / (1.0 - psi_g_snow) * (1.0 - 1.0 / ratio_flood));
  double S1 = e.S1, H1 = e.H1, m1 = e.m1, th1 = e.th1;
  const double SN = e.SN, HN = e.HN, mN = e.mN, TN = e.TN;
  const double S_buN = SN / mN;

  S1 = S1 + flood_brine * S_buN;
  H1 = H1 + flood_brine * HN / mN;
  m1 = m1 + flood_brine;
  th1 = th1 + shift_ice;
  H1 = H1 + shift_snow / CL(thick_snow) * CL(H_abs_snow);
  CL(H_abs_snow) = CL(H_abs_snow) - shift_snow / CL(thick_snow) * CL(H_abs_snow);
  m1 = m1 + shift_snow / CL(thick_snow) * CL(m_snow);
  CL(m_snow) = CL(m_snow) - shift_snow / CL(thick_snow) * CL(m_snow);
  CL(thick_snow) = CL(thick_snow) - shift_snow;

  e.deep = freeboard + shift_ice < neg_free;
  e.incS = 0.0; e.incH = 0.0;
  if (e.deep) {
    const double shift = neg_free - (freeboard + shift_ice);
    flood_brine = shift * (psi_g_snow) * rho_l;
    e.incS = (x.S_bu_bottom - S_buN) * flood_brine;
    e.incH = (g.T_bottom - TN) * c_l * flood_brine;
    S1 = S1 + S_buN * flood_brine;
    H1 = H1 + TN * c_l * flood_brine;
    m1 = m1 + flood_brine;
    th1 = th1 + shift;
    H1 = H1 + shift / CL(thick_snow) * CL(H_abs_snow);
    CL(H_abs_snow) = CL(H_abs_snow) - shift / CL(thick_snow) * CL(H_abs_snow);
    m1 = m1 + shift / CL(thick_snow) * CL(m_snow);
    CL(m_snow) = CL(m_snow) - shift / CL(thick_snow) * CL(m_snow);
    CL(thick_snow) = CL(thick_snow) - shift;
  }
  e.S1 = S1; e.H1 = H1; e.m1 = m1; e.th1 = th1;
  return flood_brine;
}

template <class K>
__device__ RARE void flood(Col &c, const Ctx &x) {
  const samsim_config &g = x.p->cfg;
  const int Na = c.Na;
  // harmonic-mean permeability of the column and its total thickness: from the first sweep of this step (flood_handover); without
  // Rayleigh-number drainage (grav_flag 1: no scan) the column is walked here
  double hp, sall;
  if (CFG(grav_flag) >= 2) {
    hp = SPEC(SP_FL_HP);
    sall = SPEC(SP_FL_SALL);
  } else {
    double sth = 0.0;
    hp = 0.0;
    for (int k = 1; k <= Na - 1; ++k) {
      const double thick = LAY(SAMSIM_A_THICK, k);
      const double perm = x.p17 * pow_3p1(1000.0 * LAY(SAMSIM_A_PSI_L, k));
      hp = hp + thick / perm;
      sth += thick;
    }
    const double thN = LAY(SAMSIM_A_THICK, Na), psN = LAY(SAMSIM_A_PSI_S, Na);
    const double permN = x.p17 * pow_3p1(1000.0 * LAY(SAMSIM_A_PSI_L, Na));
    hp = hp + (thN * psN / psi_s_min) / permN;
    hp = (sth + thN * psN / psi_s_min) / hp;
    sall = sth + thN;
  }
  FloodEnds e;
  e.S1 = LAY(SAMSIM_A_S_ABS, 1); e.H1 = LAY(SAMSIM_A_H_ABS, 1); e.m1 = LAY(SAMSIM_A_M, 1); e.th1 = LAY(SAMSIM_A_THICK, 1);
  e.SN = LAY(SAMSIM_A_S_ABS, Na); e.HN = LAY(SAMSIM_A_H_ABS, Na); e.mN = LAY(SAMSIM_A_M, Na); e.TN = LAY(SAMSIM_A_T, Na);
  c.bgc_flood = flood_core<K>(c, x, hp, sall, e);
  if (e.deep) {
    LAY(SAMSIM_A_S_ABS, Na) = e.SN + e.incS;
    LAY(SAMSIM_A_H_ABS, Na) = e.HN + e.incH;
  }
  LAY(SAMSIM_A_S_ABS, 1) = e.S1;
  LAY(SAMSIM_A_H_ABS, 1) = e.H1;
  LAY(SAMSIM_A_M, 1) = e.m1;
  LAY(SAMSIM_A_THICK, 1) = e.th1;
}

// ---------------------------------------------------------------- flood_simple, mo_flood.f90:167-210 (flood_flag 3)
template <class K>
__device__ RARE void flood_simple(Col &c, const Ctx &x) {
  const samsim_config &g = x.p->cfg;
  const double shift = GS(FREEBOARD) - neg_free;
  const double flood_brine = -shift * GS(PSI_G_SNOW) * rho_l;
  double S1 = LAY(SAMSIM_A_S_ABS, 1), H1 = LAY(SAMSIM_A_H_ABS, 1), m1 = LAY(SAMSIM_A_M, 1), th1 = LAY(SAMSIM_A_THICK, 1);
  th1 = th1 - shift;
  S1 = S1 + x.S_bu_bottom * flood_brine;
  H1 = H1 - shift / CL(thick_snow) * CL(H_abs_snow);
  H1 = H1 + g.T_bottom * c_l * flood_brine;
  m1 = m1 - shift / CL(thick_snow) * CL(m_snow);
  m1 = m1 + flood_brine;
  CL(H_abs_snow) = CL(H_abs_snow) + shift / CL(thick_snow) * CL(H_abs_snow);
  CL(m_snow) = CL(m_snow) + shift / CL(thick_snow) * CL(m_snow);
  CL(thick_snow) = CL(thick_snow) + shift;
  LAY(SAMSIM_A_S_ABS, 1) = S1;
  LAY(SAMSIM_A_H_ABS, 1) = H1;
  LAY(SAMSIM_A_M, 1) = m1;
  LAY(SAMSIM_A_THICK, 1) = th1;
}

// recompute ray(1) after flood changed thick(1) (thick(1) enters only the k = 1 harmonic mean)
// (thick: the flooded thick(1); psi_l, S_br: the top layer's liquid fraction and brine salinity of this step's first sweep)
template <class K>
__device__ RARE void refresh_ray_top(Col &c, const Ctx &x, double thick, double psi_l, double S_br) {
  const samsim_config &g = x.p->cfg;
  if (CFG(harmonic_flag) != 2) return;  // MINVAL variant does not depend on thick(1)
  // the scan over layers N_active..2 as the first sweep left it (flood_handover), completed with the flooded top layer exactly as
  // s1_layer completes it
  const double perm = x.p17 * pow_3p1(1000.0 * fabs(psi_l));
  const double st2 = SPEC(SP_ST), bot = SPEC(SP_BOT);
  const double height = st2 + bot;
  const double minp = dmin(SPEC(SP_MINP), perm);
  const double stp = SPEC(SP_STP) + quot(thick, perm);
  const double st = st2 + thick;
  const double hp = (minp < x.p14) ? 0.0 : quot(st + bot, stp + SPEC(SP_BOTTERM));
  double ray = grav_f * rho_l * bbeta * (S_br - SPEC(SP_SBR_BOT)) * height * hp;
  ray = ray * (1.0 / (kappa_l * mu));
  LAY(SAMSIM_A_RAY, 1) = dmax(ray, 0.0);
}

// ---------------------------------------------------------------- flush3, mo_flush.f90:70-237
template <class K>
__device__ RARE void flush3(Col &c, const Ctx &x) {
  const samsim_config &g = x.p->cfg;
  const Salt &s = x.salt;
  const int Na = c.Na, N = c.N;
  const double dt = g.dt;
  // horizontal flow length = total thickness (mo_flush.f90:104)
  double cnst = 0.0;
  THICK_RULE_INIT(tr);
  for (int k0 = 1; k0 <= Na; k0 += 2 * RARE_CHUNK) {   // (rows requested a chunk at a time, see RARE_CHUNK)
    double th_[2 * RARE_CHUNK];
#pragma unroll
    for (int i = 0; i < 2 * RARE_CHUNK; ++i) { const int kk = (k0 + i <= N) ? k0 + i : N; th_[i] = THICK_AT(tr, kk); }
#pragma unroll
    for (int i = 0; i < 2 * RARE_CHUNK; ++i) if (k0 + i <= Na) cnst += th_[i];
  }
  cnst = cnst * para_flush_horiz;
  const double psi_l1 = LAY(SAMSIM_A_PSI_L, 1), thick1 = LAY(SAMSIM_A_THICK, 1), T1 = LAY(SAMSIM_A_T, 1);
  CL(melt_thick) = dmin(CL(melt_thick), psi_l1 * thick1);
  CL(melt_thick) = dmin(CL(melt_thick), g.thick_0 / 3.0);

  // permeability and bottom -> top equivalent resistance R(k) (stored in the V_ex scratch rows)
  const double pfill = (CFG(snow_flush_flag) == 1) ? 0.0 : 1.0;
  for (int k = Na + 1; k <= N; ++k) LAY(SAMSIM_A_PERM, k) = pfill;
  double R_below = 0.0;  // R(k+1)
  for (int k0 = Na; k0 >= 1; k0 -= RARE_CHUNK) {
    double th_[RARE_CHUNK], pl_[RARE_CHUNK], pg_[RARE_CHUNK];
#pragma unroll
    for (int i = 0; i < RARE_CHUNK; ++i) {
      const int kk = (k0 - i >= 1) ? k0 - i : 1;
      th_[i] = THICK_AT(tr, kk); pl_[i] = LAY(SAMSIM_A_PSI_L, kk);
      pg_[i] = (CFG(snow_flush_flag) == 1) ? LAY(SAMSIM_A_PSI_G, kk) : 0.0;
    }
#pragma unroll
    for (int i = 0; i < RARE_CHUNK; ++i) {
      const int k = k0 - i;
      if (k >= 1) {
        const double thick = th_[i];
        double perm;
        if (CFG(snow_flush_flag) == 1) {
          perm = x.p17 * pow_3p1(1000.0 * fabs(pl_[i] + 2.0 * pg_[i]));
          if (perm == 0.0) perm = 1.0;
        } else {
          perm = x.p17 * pow_3p1(1000.0 * fabs(pl_[i]));
        }
        LAY(SAMSIM_A_PERM, k) = perm;
        const double pm = dmax(perm, 0.00000000000000000000001);
        const double R_v = mu * thick / pm, R_h = mu * cnst / (thick * pm);
        double R;
        if (k == Na) R = 0.0;
        else if (k == Na - 1) R = R_v;
        else { R = R_below + R_v; R = ((R)*R_h) / (R + R_h); }
        LAY(D_V_EX, k) = R;
        R_below = R;
      }
    }
  }
  const double R1 = R_below;
  double flush_total = (GS(FREEBOARD) + CL(melt_thick)) / R1 * grav_f * dt * func_density(T1, S_br_poly(s, T1)) * rho_l;
  flush_total = dmin(flush_total, CL(melt_thick) * rho_l);
  GS(MELT_ERR) = GS(MELT_ERR) + CL(melt_thick) - dmin(flush_total / rho_l, CL(melt_thick));

  // top -> bottom: split into vertical / horizontal parts, vertical mass_transfer (fl_m(k+1) = -flush_v(k) <= 0),
  // horizontal loss of every layer goes to layer N_active
  double fv_up = 0.0;                                  // flush_v(k-1)
  double T_up = 0.0, S_bu_up = 0.0, S_abs_up = 0.0;    // layer k-1: T, local S_bu snapshot, S_abs after the vertical transfer
  double sum_fh = 0.0, accH = 0.0, accS = 0.0, minS = 1.0e300;
  double S_bu_N = 0.0;
  constexpr int CH2 = RARE_CHUNK / 2;   // nine operands per layer
  for (int k0 = 1; k0 <= Na; k0 += CH2) {
    double th_[CH2], pe_[CH2], T_[CH2], m_[CH2], S_[CH2], H_[CH2], Rn_[CH2], fvv_[CH2], fhh_[CH2];
#pragma unroll
    for (int i = 0; i < CH2; ++i) {
      const int kk = (k0 + i <= N) ? k0 + i : N, kn = (kk + 1 <= N) ? kk + 1 : N;
      th_[i] = THICK_AT(tr, kk); pe_[i] = LAY(SAMSIM_A_PERM, kk); T_[i] = LAY(SAMSIM_A_T, kk);
      m_[i] = LAY(SAMSIM_A_M, kk); S_[i] = LAY(SAMSIM_A_S_ABS, kk); H_[i] = LAY(SAMSIM_A_H_ABS, kk);
      Rn_[i] = LAY(D_V_EX, kn); fvv_[i] = LAY(SAMSIM_A_FLUSH_V, kk); fhh_[i] = LAY(SAMSIM_A_FLUSH_H, kk);
    }
#pragma unroll
    for (int i = 0; i < CH2; ++i) {
    const int k = k0 + i;
    if (k <= Na) {
    const double thick = th_[i], perm = pe_[i], T = T_[i];
    double m = m_[i], S_abs = S_[i], H_abs = H_[i];
    const double S_bu = S_abs / m;  // local S_bu of flush3 (mo_flush.f90:101)
    const double pm = dmax(perm, 0.00000000000000000000001);
    const double R_v = mu * thick / pm, R_h = mu * cnst / (thick * pm);
    double fh, fv;
    if (k <= Na - 1) {
      const double Rn = Rn_[i];
      const double src = (k == 1) ? flush_total : fv_up;
      fh = src * (Rn + R_v) / (Rn + R_v + R_h);
      fv = src * R_h / (Rn + R_v + R_h);
    } else {
      fv = fv_up;
      fh = 0.0;
    }
    LAY(SAMSIM_A_FLUSH_V, k) = fvv_[i] + fv;  // accumulated output, mo_grotz.f90:697-737
    LAY(SAMSIM_A_FLUSH_H, k) = fhh_[i] + fh;
    if (HAS_BGC) { BFL(BFL_V, k) = fv; BFL(BFL_H, k) = fh; }
    sum_fh += fh;
    const double flm_next = -fv, flm_k = -fv_up;
    if (flm_next < 0.0) {
      H_abs = H_abs + flm_next * T * c_l;
      S_abs = S_abs + dmax(flm_next * S_br_clamped(s, T, S_bu), -S_abs);
    }
    if (k > 1 && flm_k < 0.0) {
      H_abs = H_abs - flm_k * T_up * c_l;
      S_abs = S_abs - dmax(flm_k * S_br_clamped(s, T_up, S_bu_up), -S_abs_up);
    }
    T_up = T; S_bu_up = S_bu; S_abs_up = S_abs;
    fv_up = fv;
    if (k == Na) {
      S_bu_N = S_bu;
      if (CFG(flush_heat_flag) == 2) H_abs = H_abs - flm_next * T * c_l;
      // horizontal contributions of the layers above, then the loss of all horizontal brine
      H_abs = H_abs + accH;
      S_abs = S_abs + accS;
      const double loss_S = sum_fh * S_bu_N, loss_H = sum_fh * T * c_l;
      if (CFG(flush_heat_flag) == 2) H_abs = H_abs - loss_H;
      S_abs = S_abs - loss_S;
    } else {
      if (k == 1) {
        m = m - flush_total;
        LAY(SAMSIM_A_M, 1) = m;
        LAY(SAMSIM_A_THICK, 1) = thick - flush_total / rho_l;
      }
      const double loss_S = fh * S_br_clamped(s, T, S_abs / m);
      const double loss_H = fh * T * c_l;
      S_abs = S_abs - loss_S;
      H_abs = H_abs - loss_H;
      accH += loss_H;
      accS += loss_S;
    }
    LAY(SAMSIM_A_S_ABS, k) = S_abs;
    LAY(SAMSIM_A_H_ABS, k) = H_abs;
    minS = dmin(minS, S_abs);
    }
    }
  }
  if (minS < -0.00000000000000000000000001) {
    for (int k = 1; k <= Na; ++k) {
      const double v = LAY(SAMSIM_A_S_ABS, k);
      if (v < 0.0) LAY(SAMSIM_A_S_ABS, k) = 0.0;
    }
  }
  if (fabs(LAY(SAMSIM_A_M, 1)) < 0.000001) STOPC(9876, 1);
}

// prescribe_flag 2, mo_grotz.f90:482-497: bulk salinity linear from S_bu_bottom to 4 over the lowest 0.15 m and from 4 to 0
// above it.  The SUMs start afresh for every layer, in ascending order like the reference's; of S_bu only layer 1 is written (the up
// sweep refreshes the others from S_abs before anything reads them).  Layer 1 of ice thinner than 0.15 m keeps the S_bu of the first sweep.
template <class K>
__device__ RARE void prescribe_salinity(Col &c, const Ctx &x) {
  const int N = c.N, Na = c.Na;
  const double Sb = x.S_bu_bottom;
  auto thick_sum = [&](int a) { double t = 0.0; for (int j = a; j <= Na; ++j) t += LAY(SAMSIM_A_THICK, j); return t; };
  const double total = thick_sum(1);
  double S_bu1 = LAY(SAMSIM_A_S_BU, 1);
  int k = Na;
  while (k > 1) {
    const double t = thick_sum(k);
    if (!(t < 0.15)) break;
    LAY(SAMSIM_A_S_ABS, k) = (Sb - t / 0.15 * (Sb - 4.0)) * LAY(SAMSIM_A_M, k);
    k = k - 1;
  }
  while (k > 1) {
    const double t = thick_sum(k);
    if (!(t >= 0.15)) break;
    LAY(SAMSIM_A_S_ABS, k) = (4.0 - 4.0 * (t - 0.15) / (total - 0.15)) * LAY(SAMSIM_A_M, k);
    k = k - 1;
    S_bu1 = 0.0;
  }
  // Both loops ending above layer 1 takes SUMs that shrink as layers are added (a negative or NaN thickness).  The reference then
  // leaves S_bu(2..k) as the refresh of mo_grotz.f90:333 set them and forms S_abs = S_bu*m from that; the unfused order, which a
  // prescribed profile always takes, has that row in the array (sweep_expulsion_transfer).
  for (int j = k; j > 1; --j) LAY(SAMSIM_A_S_ABS, j) = LAY(SAMSIM_A_S_BU, j) * LAY(SAMSIM_A_M, j);
  if (Na > 1) LAY(SAMSIM_A_S_ABS, Na) = Sb * LAY(SAMSIM_A_M, Na);
  else S_bu1 = Sb;
  LAY(SAMSIM_A_S_ABS, 1) = S_bu1 * LAY(SAMSIM_A_M, 1);
  LAY(SAMSIM_A_S_BU, 1) = S_bu1;  // read by the thin-snow coupling of sub_heat_fluxes (mo_heat_fluxes.f90:293)
  for (int j = Na + 1; j <= N; ++j) LAY(SAMSIM_A_S_ABS, j) = 0.0;
}

// flush4, mo_flush.f90:253-296 (flush_flag 6): the melt water leaves the top layer with its brine salinity; every layer more
// liquid than the one above loses the fraction 1 - para_flush_gamma of its salt, down to the first one that is not
// (layers below N_active hold no salt, so the walk may end there).
template <class K>
__device__ RARE void flush4(Col &c, const Ctx &x) {
  const int Na = c.Na;
  const double T1 = LAY(SAMSIM_A_T, 1), m1 = LAY(SAMSIM_A_M, 1), melt = CL(melt_thick);
  double S1 = LAY(SAMSIM_A_S_ABS, 1);
  LAY(SAMSIM_A_H_ABS, 1) = LAY(SAMSIM_A_H_ABS, 1) - melt * rho_l * c_l * T1;
  S1 = S1 - melt * rho_l * S_br_clamped(x.salt, T1, S1 / m1);
  LAY(SAMSIM_A_THICK, 1) = LAY(SAMSIM_A_THICK, 1) - melt;
  LAY(SAMSIM_A_M, 1) = m1 - melt * rho_l;
  CL(melt_thick) = 0.0;
  double above = LAY(SAMSIM_A_PSI_L, 1);
  for (int k = 2; k <= Na; ++k) {
    const double here = LAY(SAMSIM_A_PSI_L, k);
    if (!(here > above)) break;
    LAY(SAMSIM_A_S_ABS, k) = para_flush_gamma * LAY(SAMSIM_A_S_ABS, k);
    above = here;
  }
  LAY(SAMSIM_A_S_ABS, 1) = dmax(S1, 0.0);
  double mn = 0.0;
  for (int k = 2; k <= Na; ++k) mn = dmin(mn, LAY(SAMSIM_A_S_ABS, k));
  if (mn < 0.0) STOPC(9876, 0);
}

}  // namespace

#endif
