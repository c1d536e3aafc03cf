// samsim_sweeps_unfused.h -- the reference's order of a step, sweep by sweep: the full first sweep (sweep_thermo_expulsion),
// sweep_expulsion_transfer, sweep_grav_drain(_simple), sweep_heat_down, their driver down_unfused, and refill_psi_rows.
// Part of the translation unit samsim_kernels.hip: expects samsim_step_types.h (`c`, `x`, `g`; CL, GS, LAY / LAYU, SPEC, CFG, STOPC,
// THICK_AT), samsim_thermo.h, samsim_surface.h, samsim_sweeps_fused.h (s1_layer, sweep_beer, heat_conductance) and samsim_melt.h.
#ifndef SAMSIM_SWEEPS_UNFUSED_H
#define SAMSIM_SWEEPS_UNFUSED_H

namespace {

// defined in samsim_kernels.hip (the output block sits inside the unfused order)
template <class K>
__device__ RARE void output_point(Col &c, const Ctx &x, long long col, double time);
template <class K>
__device__ __forceinline__ void testcase_scalars(Col &c, const Ctx &x, const samsim_config &g, double time);

// all_phi: the solid fractions of every layer go to their array (an output point follows); otherwise only where something reads them
// before the up sweep rewrites them (layer 1, the bottom two layers: thin-snow coupling, regrid trigger).  whole_wave: every column
// of the wave runs this sweep (the normal state of a melt season, when every column flushes in every step): then the Rayleigh rows
// are stored and flagged like the fused up sweep's -- only where some column drains -- instead of all of them.
template <class K>
__device__ RARE void sweep_thermo_expulsion(Col &c, const Ctx &x, bool all_phi, bool whole_wave) {
  const samsim_config &g = x.p->cfg;
  const Salt &s = x.salt;
  const int Na = c.Na;
  const bool do_ray = (CFG(grav_flag) >= 2 && Na > 1);
  double T_test = g.T_bottom;
  RayScan r, r_below_top;
  ray_scan_init(r);
  r_below_top = r;
  double thick_bottom = 0.0;
  int rc = 0, rc_layer = 0;
  if (do_ray && Na <= c.N - 1 && (!whole_wave || x.ray_rows_all)) LAYU(SAMSIM_A_RAY, Na) = 0.0;
  if (whole_wave) {
    for (int w = 0; w <= (c.N - 1) >> 6; ++w) x.rflag[w] = 0ull;   // every lane writes the same zeros
    __builtin_amdgcn_wave_barrier();
  }
  // operands requested two layers ahead of the arithmetic, unconditionally and from a clamped row, as in sweep_up_fused.
  // The thickness rule (COLF_REGULAR) is checked against the array after samsim_set_state and after a regrid; in between -- the
  // steps of a melt season, which take this sweep because flush3 rewrites every layer -- nothing touches the thicknesses below
  // layer 1 and a regular column's come from the rule.  Decided per wave, so that the loop's requests stay unconditional.
  struct L4 { double H, m, th, S; };
  bool regular = true;
  const double th_mid_rule = LAYU(SAMSIM_A_THICK, g.n_top + 1);
  const bool check_col = (c.flags & COLF_REGULAR) == 0 || (c.flags & (COLF_RESTART | COLF_REGRID)) != 0;
  // A state that samsim_set_state has just uploaded has no previous step: its salt is taken as it is, as the reference takes its
  // initial state (a negative S_abs then meets gravity drainage's MINVAL(S_abs) test, STOP 1337).  samsim_get_state returns the
  // clamped values, so a checkpoint holds nothing this sweep would have clamped.
  const bool uploaded = (c.flags & COLF_RESTART) != 0;
  const bool check_wave = wave_any(check_col);
  const int kmax = wave_max(Na);
  auto run = [&](auto check_tag) {
    constexpr bool CHECK = decltype(check_tag)::value;
    auto ld = [&](int j) -> L4 {
      L4 r;
      r.H = LAYU(SAMSIM_A_H_ABS, j); r.m = LAYU(SAMSIM_A_M, j); r.S = LAYU(SAMSIM_A_S_ABS, j);
      r.th = (CHECK || j < 2) ? LAYU(SAMSIM_A_THICK, j) : thick_by_rule(j, g.n_top, g.n_middle, th_mid_rule, g.thick_0);
      return r;
    };
    L4 cur = ld(Na), nxt = ld(Na >= 2 ? Na - 1 : 1), nn = nxt;
    for (int k = kmax; k >= 1; --k) {
      if (k > Na) continue;
      nn = ld(k >= 3 ? k - 2 : 1);
      const double H_abs = cur.H, m = cur.m, thick = cur.th;
      if (CHECK && k >= 2 && thick != thick_by_rule(k, g.n_top, g.n_middle, th_mid_rule, g.thick_0)) regular = false;
      double S_abs = cur.S;
      cur = nxt; nxt = nn;
      if (S_abs < 0.0 && !uploaded) {  // health check of the previous step, mo_grotz.f90:812-818 (element-wise clamp)
        S_abs = 0.0;
        LAYU(SAMSIM_A_S_ABS, k) = S_abs;
      }
      double S_bu, H;
      per_mass(S_abs, H_abs, m, S_bu, H);
      double T, phi = 0.0;
      int rr = getT_chain<true>(s, H, S_bu, T_test, T, phi);
      if (rr && !rc) { rc = rr; rc_layer = k; }
      T_test = T;
      // T and phi are the hand-over to the down sweep; S_bu / S_br are recomputed there from T, S_abs, m
      LAYU(SAMSIM_A_T, k) = T;
      if (all_phi || k == 1 || k >= Na - 1) LAYU(SAMSIM_A_PHI, k) = phi;
      if (k == 1) r_below_top = r;                                   // the scan over layers N_active..2 (flood_handover)
      if (k == Na) thick_bottom = thick;
      s1_layer<K>(c, x, k, Na, do_ray, T, phi, S_bu, m, thick, recip(thick), r, whole_wave);
    }
  };
  if (check_wave) run(std::true_type{}); else run(std::false_type{});
  if (whole_wave) { __builtin_amdgcn_wave_barrier(); c.ray_all = false; }   // the rows that hold a value are the flagged ones
  if (do_ray) flood_handover<K>(c, x, r, r_below_top, thick_bottom);
  c.neg_psi = r.min_psi_s < 0.0;
  c.buoy_s = r.buoy_s;
  c.flags = regular ? (c.flags | COLF_REGULAR) : (c.flags & ~COLF_REGULAR);
  if (rc) STOPC(rc, rc_layer);
}

// ---------------------------------------------------------------- P2: expulsion_flux + mass_transfer, top -> bottom
// expulsion_flux (mo_mass.f90:112-136): downward brine flux recurrence, m and psi_g update.  mass_transfer
// (mo_mass.f90:53-96) with these fluxes (all <= 0: brine only moves down) needs the layer above only.  Then the
// S_bu refresh of mo_grotz.f90:333-335.  mass_transfer is skipped on the first step (mo_grotz.f90:313).
// DRY: nothing is stored -- the sweep only tells what flooding needs to know before the fused down sweep runs (column_step): the
// gas-filled volume of the column after expulsion_flux (for the freeboard) and the top and bottom layers as brine expulsion and its
// mass_transfer leave them (flooding moves water between exactly these two and the snow).
struct ExpelledEnds {
  double S1, H1, m1, psi_l1, S_br1;    // layer 1 after expulsion + mass_transfer; its liquid fraction and brine salinity of the first sweep
  double SN, HN, mN, TN, psi_gN;       // layer N_active likewise (before the gas -> ocean water replacement)
  double buoy_g;                       // SUM(psi_g*thick) after expulsion_flux
};
template <class K, bool DRY = false>
__device__ RARE void sweep_expulsion_transfer(Col &c, const Ctx &x, ExpelledEnds *ends = nullptr) {
  const int Na = c.Na;
  const bool transfer = (c.step + 1 != 1);
  double flm_k = 0.0;  // fl_m(k)
  double buoy_g = 0.0;
  double fb_a2 = 0.0, fb_g2 = 0.0;   // SUM(psi_s*thick), SUM(psi_g*thick) over layers >= 2 for func_freeboard
  double T_up = 0.0, S_br_up = 0.0, S_abs_up = 0.0;  // layer k-1: snapshot T, S_br, UPDATED S_abs
  // rows are requested a chunk at a time (see RARE_CHUNK)
  constexpr int CH = RARE_CHUNK / 2;
  THICK_RULE_INIT(tr);
  for (int k0 = 1; k0 <= Na; k0 += CH) {
    double m_[CH], th_[CH], T_[CH], H_[CH], S_[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int kk = (k0 + i <= c.N) ? k0 + i : c.N;
      m_[i] = LAY(SAMSIM_A_M, kk); th_[i] = THICK_AT(tr, kk); T_[i] = LAY(SAMSIM_A_T, kk);
      H_[i] = LAY(SAMSIM_A_H_ABS, kk); S_[i] = LAY(SAMSIM_A_S_ABS, kk);
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
    const int k = k0 + i;
    if (k <= Na) {
    double m = m_[i];
    const double thick = th_[i];
    // Expulsion of the first sweep (mo_grotz.f90:306), re-evaluated from its inputs phi, thick, m
    const double T = T_[i], H_abs_in = H_[i];
    double S_abs = S_[i];
    double S_bu_in, H_in;
    per_mass(S_abs, H_abs_in, m, S_bu_in, H_in);
    // S_br(k) of the first sweep = func_S_br(T, S_abs/m) with the mass BEFORE expulsion_flux: recomputed bit for bit
    // (same inputs, same operations) instead of being stored by every S1 sweep; this unfused path keeps it for P3
    const double S_br = S_br_clamped(x.salt, T, S_bu_in);
    const Expelled ex = expulsion(phi_from_T(x.salt, H_in, S_bu_in, S_br), thick, m, recip(thick));
    const double V_ex = ex.V_ex;
    double psi_g = ex.psi_g;
    double flm_next;
    if (k == 1 || psi_g < (double)0.001f) {
      flm_next = (k == 1) ? -V_ex * rho_l : -V_ex * rho_l + flm_k;
    } else {
      flm_next = -dmax((V_ex - psi_g * thick) * rho_l, 0.0);
      psi_g = dmax((psi_g * thick - V_ex) / thick, 0.0);
    }
    if (psi_g > 0.0) buoy_g += psi_g * thick;
    if (k >= 2) { fb_a2 += ex.psi_s * thick; fb_g2 += psi_g * thick; }
    if (!DRY) {
      LAY(SAMSIM_A_PSI_S, k) = ex.psi_s;
      LAY(SAMSIM_A_PSI_L, k) = ex.psi_l;
      LAY(SAMSIM_A_PSI_G, k) = psi_g;
    }
    m = m + flm_next - flm_k;
    if (!DRY) {
      LAY(SAMSIM_A_M, k) = m;
      if (HAS_BGC) BFL(BFL_E, k) = transfer ? -flm_next : 0.0;
      LAY(SAMSIM_A_S_BR, k) = S_br;
    }
    double H_abs = H_abs_in;
    if (transfer) {
      bool ch = false;
      if (flm_next < 0.0) {
        H_abs = H_abs + flm_next * T * c_l;
        S_abs = S_abs + dmax(flm_next * S_br, -S_abs);
        ch = true;
      }
      if (flm_k < 0.0) {
        H_abs = H_abs - flm_k * T_up * c_l;
        S_abs = S_abs - dmax(flm_k * S_br_up, -S_abs_up);
        ch = true;
      }
      if (ch && !DRY) {
        LAY(SAMSIM_A_H_ABS, k) = H_abs;
        LAY(SAMSIM_A_S_ABS, k) = S_abs;
      }
    }
    if (!DRY) LAY(SAMSIM_A_S_BU, k) = S_abs / m;
    if (DRY) {
      if (k == 1) { ends->S1 = S_abs; ends->H1 = H_abs; ends->m1 = m; ends->psi_l1 = ex.psi_l; ends->S_br1 = S_br; }
      if (k == Na) { ends->SN = S_abs; ends->HN = H_abs; ends->mN = m; ends->TN = T; ends->psi_gN = psi_g; }
    }
    T_up = T; S_br_up = S_br; S_abs_up = S_abs;
    flm_k = flm_next;
    }
    }
  }
  if (DRY) { ends->buoy_g = buoy_g; return; }
  c.buoy_g = buoy_g;
  SPEC(SP_FB_A2) = fb_a2; SPEC(SP_FB_G2) = fb_g2;
}

// ---------------------------------------------------------------- P3: gravity drainage, top -> bottom
// fl_grav_drain (mo_grav_drain.f90:138-200) with ray(k) from S1: drainage flux of layer k leaves straight to the
// ocean, the compensating upward flow fl_up passes through every layer below (running sum), then mass_transfer
// (mo_mass.f90:53-96) with fl_m(k+1) = fl_up(k) >= 0.  mass_transfer reads the salt of the layer BELOW after the
// drainage loop (snapshot SS_abs), so layer k+1 is drained one iteration ahead of the transfer into layer k.
// The same pass multiplies up the Beer-law transmittance for fl_rad(N_active) (mo_heat_fluxes.f90:151-155).
template <class K>
__device__ RARE void sweep_grav_drain(Col &c, const Ctx &x, bool do_beer, double beer0) {
  const samsim_config &g = x.p->cfg;
  const Salt &s = x.salt;
  const int Na = c.Na;
  const double dt = g.dt;
  double heat_loss = 0.0, cum = 0.0, sum_before = 0.0, sum_after = 0.0, minS = 1.0e300;
  // Beer law: temp2 decays layer by layer; exp() is re-evaluated only when the thickness changes
  double temp2 = beer0, e = 0.0, th_prev = -1.0;
  int stop_layer = 0;

  struct L { double T, S_bu, S_abs, H_abs, flup, fdown; bool ch; };
  struct Ops { double T, S_bu, S_abs, H_abs, thick, S_br, S_br_below; };

  // drain(j): gravity-drainage loss of layer j (mo_grav_drain.f90:144-170) and fl_up(j)
  auto drain = [&](int j, const Ops &o) -> L {
    L r;
    r.T = o.T;
    r.S_bu = o.S_bu;
    r.S_abs = o.S_abs;
    r.H_abs = o.H_abs;
    r.ch = false;
    r.fdown = 0.0;
    const double thick = o.thick;
    if (do_beer) {
      if (thick != th_prev) { e = exp(-extinc * thick); th_prev = thick; }
      if (j == Na) c.frad = temp2 - temp2 * e;
      temp2 = temp2 * e;
    }
    sum_before += r.S_abs;
    r.flup = cum;
    if (j <= Na - 1) {
      const double S_br = o.S_br;
      const double ray = ray_row_valid(c, x, j) ? LAY(SAMSIM_A_RAY, j) : 0.0;
      if (ray > ray_crit && S_br > o.S_br_below) {
        const double psi_s = LAY(SAMSIM_A_PSI_S, j), m = LAY(SAMSIM_A_M, j);
        if (psi_s > 0.001 && r.S_abs / m > 0.1) {
          const double psi_l = LAY(SAMSIM_A_PSI_L, j);
          double flux = x_grav * (ray - ray_crit) * dt * thick;
          flux = dmin(flux, psi_l * rho_l * thick);
          r.S_abs = r.S_abs - flux * S_br;
          if (r.S_abs < 0.0 && !stop_layer) stop_layer = j;
          CL(grav_temp) = CL(grav_temp) + flux * r.T;
          r.H_abs = r.H_abs - flux * c_l * r.T;
          heat_loss = heat_loss + flux * c_l * r.T;
          cum = cum + flux;
          r.flup = dmin(cum, psi_l * rho_l * thick);
          r.fdown = flux;
          r.ch = true;
        }
      }
    }
    sum_after += r.S_abs;
    return r;
  };

  // Layer j is drained, then layer j-1 -- which now knows its neighbour below -- is finished: the reference's order.  The plain
  // operands of a chunk of layers are requested together (see RARE_CHUNK); what only a draining layer reads is loaded there.
  constexpr int CH = RARE_CHUNK / 2;
  const int N = c.N;
  THICK_RULE_INIT(tr);
  L cur = {0, 0, 0, 0, 0, 0, false};
  double flup_prev = 0.0;  // fl_up(k-1) = fl_m(k)
  for (int j0 = 1; j0 <= Na + 1; j0 += CH) {
    double T_[CH], Sbu_[CH], S_[CH], H_[CH], th_[CH], Sbr_[CH + 1];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int kk = (j0 + i <= N) ? j0 + i : N;
      T_[i] = LAY(SAMSIM_A_T, kk); Sbu_[i] = LAY(SAMSIM_A_S_BU, kk); S_[i] = LAY(SAMSIM_A_S_ABS, kk);
      H_[i] = LAY(SAMSIM_A_H_ABS, kk); th_[i] = THICK_AT(tr, kk); Sbr_[i] = LAY(SAMSIM_A_S_BR, kk);
    }
    Sbr_[CH] = LAY(SAMSIM_A_S_BR, (j0 + CH <= N) ? j0 + CH : N);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int j = j0 + i;
      if (j <= Na + 1) {
        L nxt = cur;
        if (j <= Na) nxt = drain(j, Ops{T_[i], Sbu_[i], S_[i], H_[i], th_[i], Sbr_[i], Sbr_[i + 1]});
        if (j >= 2) {
          const int k = j - 1;
          double T_below, S_bu_below, SS_abs_below;
          if (k < Na) {
            T_below = nxt.T; S_bu_below = nxt.S_bu; SS_abs_below = nxt.S_abs;
          } else {
            T_below = g.T_bottom; S_bu_below = x.S_bu_bottom; SS_abs_below = x.S_bu_bottom * 2000.0;
          }
          if (cur.flup > 0.0) {  // fl_m(k+1) > 0: inflow from below
            cur.H_abs = cur.H_abs + cur.flup * T_below * c_l;
            cur.S_abs = cur.S_abs + dmin(cur.flup * S_br_clamped(s, T_below, S_bu_below), SS_abs_below);
            cur.ch = true;
          }
          if (flup_prev > 0.0) {  // fl_m(k) > 0: outflow to the layer above
            cur.H_abs = cur.H_abs - flup_prev * cur.T * c_l;
            cur.S_abs = cur.S_abs - dmin(flup_prev * S_br_clamped(s, cur.T, cur.S_bu), cur.S_abs);
            cur.ch = true;
          }
          if (k == Na) {
            CL(grav_drain) = CL(grav_drain) + cur.flup;
            if (CFG(grav_heat_flag) == 2) { cur.H_abs = cur.H_abs + heat_loss - cur.flup * c_l * g.T_bottom; cur.ch = true; }
          }
          if (cur.ch) {
            LAY(SAMSIM_A_S_ABS, k) = cur.S_abs;
            LAY(SAMSIM_A_H_ABS, k) = cur.H_abs;
          }
          if (HAS_BGC) { BFL(BFL_D, k) = cur.fdown; BFL(BFL_U, k) = cur.flup; }
          minS = dmin(minS, cur.S_abs);
          flup_prev = cur.flup;
        }
        cur = nxt;
      }
    }
  }
  CL(grav_salt) = CL(grav_salt) + sum_before;
  CL(grav_salt) = CL(grav_salt) - sum_after;
  if (stop_layer) STOPC(21234, stop_layer);
  if (minS < 0.0) STOPC(1337, 0);
}

// fl_grav_drain_simple (mo_grav_drain.f90:218-278, grav_flag 3) with ray(k) from S1: every layer above the critical
// Rayleigh number loses 1 % of its salt (`0.99` is a default-REAL literal); fused with the Beer-law pass like P3.
template <class K>
__device__ RARE void sweep_grav_drain_simple(Col &c, const Ctx &x, bool do_beer, double beer0) {
  const int Na = c.Na;
  double temp2 = beer0, e = 0.0, th_prev = -1.0;
  for (int k = 1; k <= Na; ++k) {
    if (do_beer) {
      const double thick = LAY(SAMSIM_A_THICK, k);
      if (thick != th_prev) { e = exp(-extinc * thick); th_prev = thick; }
      if (k == Na) c.frad = temp2 - temp2 * e;
      temp2 = temp2 * e;
    }
    if (k <= Na - 1 && ray_row_valid(c, x, k) && LAY(SAMSIM_A_RAY, k) > ray_crit) LAY(SAMSIM_A_S_ABS, k) = LAY(SAMSIM_A_S_ABS, k) * (double)0.99f;
  }
  CL(grav_drain) = 0.0;
}

// Conductive update of sub_heat_fluxes (mo_heat_fluxes.f90:272-285) for layers 2..N_active on the unfused path, top -> bottom from
// the arrays (old temperatures, this step's volume fractions, the thickness flooding may just have changed): the fused down sweep
// applies it on the fly, so the up sweep never does.  Layer 1 is left to the top-layer block (fl_Q(1) comes from the surface
// balance); fl_Q(2) and the two energy sums are handed on in the column struct.
template <class K>
__device__ RARE void sweep_heat_down(Col &c, const Ctx &x) {
  const int Na = c.Na, N = c.N;
  const double dt = x.p->cfg.dt;
  const double frad_dt = c.frad * dt;
  double esum = 0.0;
  c.flq2 = 0.0;
  if (Na >= 2) {
    double T_up = LAY(SAMSIM_A_T, 1);
    double g_up = heat_conductance(LAY(SAMSIM_A_PSI_S, 1), LAY(SAMSIM_A_PSI_L, 1), recip(LAY(SAMSIM_A_THICK, 1)));
    double flq_k = 0.0;   // fl_Q(k)
    constexpr int CH = RARE_CHUNK / 2;   // five operands per layer (rows requested a chunk at a time, see RARE_CHUNK)
    THICK_RULE_INIT(tr);
    for (int k0 = 2; k0 <= Na; k0 += CH) {
      double T_[CH], th_[CH], ps_[CH], pl_[CH], Hm_[CH];
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int kk = (k0 + i <= N) ? k0 + i : N;
        T_[i] = LAY(SAMSIM_A_T, kk); th_[i] = THICK_AT(tr, kk);
        ps_[i] = LAY(SAMSIM_A_PSI_S, kk); pl_[i] = LAY(SAMSIM_A_PSI_L, kk);
        Hm_[i] = LAY(SAMSIM_A_H_ABS, kk - 1);    // layer k-1 (kk >= 2), finished when layer k's flux is known
      }
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int k = k0 + i;
        if (k <= Na) {
          const double T = T_[i];
          const double gk = heat_conductance(ps_[i], pl_[i], recip(th_[i]));
          const double flq = heat_flux_between(T - T_up, g_up, gk);
          if (k == 2) c.flq2 = flq;
          if (k >= 3) {   // layer k-1: both of its fluxes are known now
            const double H_b = Hm_[i];
            double H_abs = H_b + (flq - flq_k) * dt;
            H_abs = H_abs + frad_dt;
            esum += H_b - H_abs;
            LAY(SAMSIM_A_H_ABS, k - 1) = H_abs;
          }
          T_up = T; g_up = gk; flq_k = flq;
        }
      }
    }
    const double H_b = LAY(SAMSIM_A_H_ABS, Na);   // bottom layer: fl_Q(N_active+1) = fl_q_bottom
    double H_abs = H_b + (c.fl_q_bottom - flq_k) * dt;
    H_abs = H_abs + frad_dt;
    esum += H_b - H_abs;
    LAY(SAMSIM_A_H_ABS, Na) = H_abs;
  }
  c.esum = esum;
}

// The reference's order between expulsion and the heat fluxes, sweep by sweep: taken whenever something sits between
// expulsion and gravity drainage (the output block, thin-snow coupling, a possible flooding event) or no Rayleigh-number
// drainage runs at all; mo_grotz.f90:312-565.
template <class K>
__device__ RARE void down_unfused(Col &c, const Ctx &x, long long col, double time, int tc, bool out_step, bool coupling,
                                  bool do_grav, bool do_beer) {
  const samsim_config &g = x.p->cfg;
  const int N = c.N, Na = c.Na;
    sweep_expulsion_transfer<K>(c, x);   // mo_grotz.f90:312-335

    if (out_step) output_point<K>(c, x, col, time);  // mo_grotz.f90:340-398

    // bottom-layer gas -> ocean water, mo_grotz.f90:405-410
    {
      const double psi_gN = LAY(SAMSIM_A_PSI_G, Na);
      if (psi_gN > 0.0) {
        const double temp2 = psi_gN * LAY(SAMSIM_A_THICK, Na) * rho_l;
        LAY(SAMSIM_A_M, Na) = LAY(SAMSIM_A_M, Na) + temp2;
        LAY(SAMSIM_A_S_ABS, Na) = LAY(SAMSIM_A_S_ABS, Na) + temp2 * x.S_bu_bottom;
        LAY(SAMSIM_A_H_ABS, Na) = LAY(SAMSIM_A_H_ABS, Na) + temp2 * c_l * g.T_bottom;
      }
    }
    // thin-snow coupling, mo_grotz.f90:418-420
    if (coupling) {
      snow_coupling<K>(c, x);
      if (c.status) return;
    }
    // flooding, mo_grotz.f90:428-445
    if (Na > 1 && CFG(flood_flag) > 1 && CL(m_snow) > 0.0 && CFG(freeboard_snow_flag) == 0) {
      // func_freeboard's "snow underwater" branch (mo_functions.f90:96-101) needs only the buoyancy totals, which S1
      // and P2 have accumulated; a non-negative freeboard is not read here and every later reader re-evaluates it
      const double buoy = c.buoy_s * (rho_l - rho_s) + c.buoy_g * rho_l;
      if (CL(m_snow) > buoy) {
        GS(FREEBOARD) = (buoy - CL(m_snow)) / rho_l;
        if (GS(FREEBOARD) < 0.0 && CFG(flood_flag) == 2) {
          flood<K>(c, x);
          if (CFG(grav_flag) >= 2) refresh_ray_top<K>(c, x, LAY(SAMSIM_A_THICK, 1), LAY(SAMSIM_A_PSI_L, 1), LAY(SAMSIM_A_S_BR, 1));
        } else if (K::general && CFG(flood_flag) == 3 && GS(FREEBOARD) < neg_free) {
          flood_simple<K>(c, x);
          if (CFG(grav_flag) >= 2) refresh_ray_top<K>(c, x, LAY(SAMSIM_A_THICK, 1), LAY(SAMSIM_A_PSI_L, 1), LAY(SAMSIM_A_S_BR, 1));
        }
      }
    }
    // bottom turbulence, sub_turb_flux mo_functions.f90:347-363
    if (CFG(turb_flag) == 2) {
      const double m = LAY(SAMSIM_A_M, Na), T = LAY(SAMSIM_A_T, Na);
      double S_abs = LAY(SAMSIM_A_S_ABS, Na);
      const double turb = Turb_A * exp(Turb_B * (-ocean_density<K>(x) + func_density(T, S_abs / m))) * g.dt;
      S_abs = S_abs - turb * (S_abs / m - x.S_bu_bottom);
      LAY(SAMSIM_A_S_ABS, Na) = S_abs;
      if (HAS_BGC) {  // the tracers of the bottom layer mix with the same coefficient, :358-360
        for (int t = 0; t < x.n_bgc; ++t) { const double q = BGC(t, Na); BGC(t, Na) = q - turb * (q / m - BGC_BOT(t)); }
      }
    }

    // testcase specifics, mo_grotz.f90:503-565 (the scalar ones commute with the gravity drainage sweep below)
    testcase_scalars<K>(c, x, g, time);

    // gravity drainage (mo_grotz.f90:463-477) fused with the Beer-law pass of sub_heat_fluxes
    const double beer0 = radiation_header<K>(c, x, time, tc);
    c.frad = 0.0;
    if (do_grav) {
      sweep_grav_drain<K>(c, x, do_beer, beer0);
      c.bgc_grav = true;
      if (c.status) return;
    } else if (K::general && CFG(grav_flag) == 3 && Na > 1) {
      sweep_grav_drain_simple<K>(c, x, do_beer, beer0);
    } else if (do_beer) {
      sweep_beer<K>(c, x, beer0);
    }
    if (K::general && CFG(prescribe_flag) == 2) prescribe_salinity<K>(c, x);  // mo_grotz.f90:482-497
    if (K::general && CFG(testcase) == 5 && c.step + 1 == 2) {  // mo_grotz.f90:543-544
      for (int k = 1; k <= N; ++k) LAY(SAMSIM_A_S_ABS, k) = 5.0 * LAY(SAMSIM_A_M, k);
    }
    // conductive update of layers >= 2 (sub_heat_fluxes, mo_grotz.f90:584; the tank budget in between only reads S_abs and m)
    sweep_heat_down<K>(c, x);
}

// Safety net of the stored-row decision (sweep_down_fused): a late reader of psi_s / psi_l / psi_g -- func_freeboard, flush3 -- in a
// step whose down sweep skipped the rows of layers >= 3.  The sweep evaluates those readers' conditions exactly before it skips
// (tests/test_gpu_melt_onset.py: a wave of columns 2..17 steps before their melt onsets, and crafted leaders of single conditions,
// never get here; the stamps build counts the calls, CT_REFILL, and that test asserts the count is 0), so this is not on any
// tested trajectory; should a column ever arrive, it keeps running:
// the rows are filled by one Expulsion pass over the finished layers (temperature of the second sweep, current masses) -- the
// values the next step's first sweep will form -- instead of the column being stopped.
template <class K>
__device__ RARE void refill_psi_rows(Col &c, const Ctx &x) {
  ST_COUNT(CT_REFILL, (unsigned long long)__popcll(__ballot(1)));
  THICK_RULE_INIT(tr);
  double fb_a2 = LAY(SAMSIM_A_PSI_S, 2) * THICK_AT(tr, 2), fb_g2 = LAY(SAMSIM_A_PSI_G, 2) * THICK_AT(tr, 2);
  for (int k = 3; k <= c.Na; ++k) {
    const double m = LAY(SAMSIM_A_M, k), thick = THICK_AT(tr, k);
    double S_bu, H;
    per_mass(LAY(SAMSIM_A_S_ABS, k), LAY(SAMSIM_A_H_ABS, k), m, S_bu, H);
    const double S_br = S_br_clamped(x.salt, LAY(SAMSIM_A_T, k), S_bu);
    const Expelled e = expulsion(phi_from_T(x.salt, H, S_bu, S_br), thick, m, recip(thick));
    LAY(SAMSIM_A_PSI_S, k) = e.psi_s;
    LAY(SAMSIM_A_PSI_L, k) = e.psi_l;
    LAY(SAMSIM_A_PSI_G, k) = e.psi_g;
    fb_a2 += e.psi_s * thick; fb_g2 += e.psi_g * thick;
  }
  SPEC(SP_FB_A2) = fb_a2; SPEC(SP_FB_G2) = fb_g2;
  c.psi_full = true;
}

}  // namespace

#endif
