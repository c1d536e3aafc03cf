// samsim_sweeps_fused.h -- the two sweeps of the common (winter) step and what they share with the other order: the Rayleigh scan and
// the per-layer body of the first sweep (RayScan, expulsion, s1_layer, flood_handover, prologue_top_layer), the Beer-law pass, the
// conductive flux between two layers, sweep_down_fused and sweep_up_fused.  Part of the translation unit samsim_kernels.hip: expects
// samsim_step_types.h (`c`, `x`, `g`; CL, GS, LAY / LAYU / LAYU_LD, SPEC, CFG, STOPC), samsim_thermo.h and samsim_surface.h.
#ifndef SAMSIM_SWEEPS_FUSED_H
#define SAMSIM_SWEEPS_FUSED_H

namespace {

// Arithmetic choices of the fused sweeps (each an ulp-level deviation from the reference's operation order; the parity bar is 1e-6
// relative, observed against the reference's own records <= 1e-11 on one-day windows, tests/test_gpu_reference_windows.py):
//  * quotients that share a divisor go through one reciprocal (Expulsion: /thick three times and the two density constants; getT:
//    /S_br and /S_br**2; S_abs/m and H_abs/m; H/c_l; the constant kappa_l*mu); recip() / quot() of samsim_div.h are the compiler's
//    own Newton sequence without the operand scaling and special-case fix-up around it (the divisors are normal-range numbers);
//  * the liquidus polynomial in Horner form (5 operations instead of 9 per evaluation);
//  * the thicknesses of a regular column from the grid rule: the semi-adaptive grid (mo_layer_dynamics.f90) keeps every layer but
//    the first at thick_0, except the N_middle elastic layers, which all share one value (they receive the same increments in the
//    same order).  Where a column follows that rule (COLF_REGULAR, checked by the full first sweep after samsim_set_state and after
//    every regrid) the sweeps form thick(k) from thick(1), thick(N_top+1) and thick_0 instead of streaming the array; a column that
//    does not follow it (a hand-made state) loads the array and takes the unfused order.

// ---------------------------------------------------------------- S1: first thermodynamic sweep, bottom -> top
// mo_grotz.f90:297-307 (S_bu, H, getT chain, S_br, Expulsion mo_thermo_functions.f90:157-187) fused with the
// permeability / Rayleigh-number part of fl_grav_drain (mo_grav_drain.f90:103-136): ray(k) needs only suffix
// quantities over k..N_active, which an upward sweep meets in the right order.
//
// RayScan carries those suffix quantities; s1_layer is the per-layer body shared by
//   - sweep_thermo_expulsion  the full sweep (first step, and after flushing / regridding changed the column),
//   - sweep_up_fused          which runs it for layers N_active..2 of the NEXT step right after the second getT of
//                             this step (same enthalpy, same guess chain => the same T and phi, computed once),
//   - prologue_top_layer      layer 1 of the current step (everything that changes between two steps touches layer 1).
struct RayScan {
  double minp, stp, st;                      // suffix min(perm), sum(thick/perm), sum(thick) over k..Na-1
  double bot, botterm, perm_bot, S_br_bot;   // bottom layer (enters linearly, mo_grav_drain.f90:119-120,128)
  double buoy_s, min_psi_s;                  // SUM(psi_s*thick), MIN(psi_s)
};
__device__ __forceinline__ void ray_scan_init(RayScan &r) {
  r.minp = 1.0e300; r.stp = 0.0; r.st = 0.0; r.bot = 0.0; r.botterm = 0.0; r.perm_bot = 0.0; r.S_br_bot = 0.0;
  r.buoy_s = 0.0; r.min_psi_s = 1.0e300;
}

// Expulsion, mo_thermo_functions.f90:157-187: volume fractions and expelled brine volume of one layer
struct Expelled { double psi_s, psi_l, psi_g, V_ex; };
// (rth = recip(thick): the fused up sweep forms it once per sweep for the two thicknesses of the grid rule; recip() is a function of
// its argument alone, so the bits are the same wherever it is formed)
__device__ __forceinline__ Expelled expulsion(double phi, double thick, double m, double rth) {
  Expelled e;
  const double V_s = m * phi * (1.0 / rho_s), V_l = m * (1.0 - phi) * (1.0 / rho_l);
  e.V_ex = dmax(V_l + V_s - thick, 0.0);   // (a sum above thick leaves a positive difference, one at or below it none)
  e.psi_s = V_s * rth;
  e.psi_l = (V_l - e.V_ex) * rth;
  e.psi_g = (thick - V_l - V_s + e.V_ex) * rth;
  e.psi_l = dmax(e.psi_l, 0.0);
  e.psi_g = dmax(e.psi_g, 0.0);
  return e;
}

// Permeability + Rayleigh number of layer k from its T, phi (Expulsion evaluated in registers).  Only PHI (by the caller)
// and ray are stored: the down sweep re-evaluates Expulsion from PHI, m and thick (same inputs, same operations) and
// writes the psi arrays itself, which is cheaper than handing psi_s, psi_l, psi_g and V_ex over through HBM.
// (S_br_T: S_br_clamped(T, S_bu) where the caller has it already -- getT_chain's S_br_out)
template <class K>
__device__ __forceinline__ void s1_layer(Col &c, const Ctx &x, int k, int Na, bool do_ray, double T, double phi, double S_bu,
                                         double m, double thick, double rth, RayScan &r, bool sparse_rows = false, const double *S_br_T = nullptr) {
  const samsim_config &g = x.p->cfg;
  const double S_br = S_br_T ? *S_br_T : S_br_clamped(x.salt, T, S_bu);
  const Expelled e = expulsion(phi, thick, m, rth);
  r.min_psi_s = dmin(r.min_psi_s, e.psi_s);
  r.buoy_s += e.psi_s * thick;
  if (k == 1) c.psi_l_top = e.psi_l;
  if (do_ray) {
    const double perm = x.p17 * pow_3p1(1000.0 * fabs(e.psi_l));  // mo_grav_drain.f90:105
    if (k == Na) {
      r.S_br_bot = S_br;
      r.bot = thick * e.psi_s / psi_s_min;
      r.perm_bot = perm;
      r.botterm = r.bot / perm;
    } else {
      const double height = r.st + r.bot;  // thick(k+1..Na-1) + bottom part
      r.minp = dmin(r.minp, perm);
      r.stp = r.stp + quot(thick, perm);
      r.st = r.st + thick;
      double ray;
      const double d_S_br = S_br - r.S_br_bot;
      const bool harmonic = CFG(harmonic_flag) == 2;
      // numerator and divisor of the harmonic-mean permeability (formed once for the vote below and for the quotient)
      const double h_sum = harmonic ? r.st + r.bot : 0.0, h_den = harmonic ? r.stp + r.botterm : 0.0;
      // A sparse row is stored only when some lane's Rayleigh number exceeds ray_crit, and three rows in four hold none: the vote does
      // not need the number.  ray = c * d_S_br * height * (st+bot) / (stp+botterm) up to a few ulp (c: the constants of the product
      // below), so c * d_S_br * height * (st+bot) < ray_crit * (1 - 2**-20) * (stp+botterm) puts it below ray_crit with a margin
      // that is 2**30 times the rounding error of either side; minp < p14 makes hp, and with it ray, 0.  Where that holds in every lane
      // the quotient, the product, the store and the row flag are skipped -- what the vote on the number itself would have decided.
      // Any other lane (a NaN operand fails P < Q like a large one) sends the whole wave through the code below, unchanged.
      if (sparse_rows && harmonic && k != 1 && !x.ray_rows_all) {
        // (the product's last constant 1 / (kappa_l * mu) stands on Q's side, so that P begins with the two products the number
        // itself begins with: a row that is not decided has paid two multiplications and a compare for the attempt)
        constexpr double q_ray = ray_crit * (1.0 - 0x1p-20) * (kappa_l * mu);
        const double P = grav_f * rho_l * bbeta * d_S_br * height * h_sum, Q = q_ray * h_den;
        ST_COUNT(CT_RAY_ROWS, 1);
        // (the ballot of each compare, AND-ed on the scalar side: a lane is undecided when neither test puts it below)
        if ((__builtin_amdgcn_ballot_w64(!(P < Q)) & __builtin_amdgcn_ballot_w64(!(r.minp < x.p14))) == 0ull) {
          ST_COUNT(CT_RAY_ROWS_BOUND, 1);
          return;
        }
      }
      if (harmonic) {
        const double hp = (r.minp < x.p14) ? 0.0 : quot(h_sum, h_den);
        ray = grav_f * rho_l * bbeta * d_S_br * height * hp;
      } else {
        ray = grav_f * rho_l * bbeta * d_S_br * height * dmin(r.minp, r.perm_bot);
      }
      ray = ray * (1.0 / (kappa_l * mu));
      ray = dmax(ray, 0.0);
      if (!sparse_rows) {
        LAYU(SAMSIM_A_RAY, k) = ray;
      } else if (k == 1 || x.ray_rows_all || wave_any(ray > ray_crit)) {  // wave-uniform k, see Ctx::rflag (row 1 always: ray_row_valid)
        LAYU(SAMSIM_A_RAY, k) = ray;
        // (every executing lane reads the word, sets the same bit and writes the same value back -- two LDS instructions in
        // lock-step, no leader to elect: the lane number a leader test compares with was one more value carried through the loop)
        x.rflag[(k - 1) >> 6] = x.rflag[(k - 1) >> 6] | (1ull << ((k - 1) & 63));
      }
    }
  }
}

// What flooding needs of the whole column (mo_flood.f90:66-80: the harmonic-mean permeability SUM(thick) / SUM(thick/perm) with the
// bottom layer's solid part, and the total thickness) is what the first sweep's scan holds once layer 1 is in: instead of walking
// the column twice more (flood, then refresh_ray_top after flooding has changed thick(1); a power per layer each), the sweep leaves
// the two numbers in the hand-over block where the snow load makes flooding possible -- and the scan WITHOUT layer 1, which
// refresh_ray_top completes with the flooded top layer.  (sums bottom -> top where the reference's run top -> bottom: round-off)
template <class K>
__device__ __forceinline__ void flood_handover(Col &c, const Ctx &x, const RayScan &all, const RayScan &below_top, double thick_bottom) {
  const samsim_config &g = x.p->cfg;
  if (!(CFG(flood_flag) > 1 && c.Na > 1 && CL(m_snow) > all.buoy_s * (rho_l - rho_s))) return;   // (= flood_possible of column_step)
  SPEC(SP_FL_HP) = quot(all.st + all.bot, all.stp + all.botterm);
  SPEC(SP_FL_SALL) = all.st + thick_bottom;
  SPEC(SP_MINP) = below_top.minp; SPEC(SP_STP) = below_top.stp; SPEC(SP_ST) = below_top.st;
  SPEC(SP_BOT) = below_top.bot; SPEC(SP_BOTTERM) = below_top.botterm; SPEC(SP_SBR_BOT) = below_top.S_br_bot;
}

// Layer 1 of the first sweep when layers N_active..2 were already done by the previous step's up sweep
// (their prognostic values have not changed since).  The scan state comes from the hand-over block.
template <class K>
__device__ __forceinline__ void prologue_top_layer(Col &c, const Ctx &x) {
  const samsim_config &g = x.p->cfg;
  const int Na = c.Na;
  const bool do_ray = (CFG(grav_flag) >= 2 && Na > 1);
  RayScan r;
  r.minp = SPEC(SP_MINP); r.stp = SPEC(SP_STP); r.st = SPEC(SP_ST);
  r.bot = SPEC(SP_BOT); r.botterm = SPEC(SP_BOTTERM); r.perm_bot = SPEC(SP_PERM_BOT);
  r.S_br_bot = SPEC(SP_SBR_BOT); r.buoy_s = SPEC(SP_BUOY_S); r.min_psi_s = SPEC(SP_MIN_PSI_S);
  const RayScan r_below_top = r;
  const double H_abs = LAY(SAMSIM_A_H_ABS, 1), m = LAY(SAMSIM_A_M, 1), thick = LAY(SAMSIM_A_THICK, 1);
  double S_abs = LAY(SAMSIM_A_S_ABS, 1);
  if (S_abs < 0.0) { S_abs = 0.0; LAY(SAMSIM_A_S_ABS, 1) = S_abs; }
  double S_bu, H;
  per_mass(S_abs, H_abs, m, S_bu, H);
  if (K::general && CFG(prescribe_flag) == 2) LAY(SAMSIM_A_S_BU, 1) = S_abs / m;  // read back by prescribe_salinity
  const double T_test = (Na > 1) ? LAY(SAMSIM_A_T, 2) : g.T_bottom;
  double T, phi = 0.0;
  const int rc = getT_chain(x.salt, H, S_bu, T_test, T, phi);   // (the wave's columns together, as in the sweeps)
  LAY(SAMSIM_A_T, 1) = T;
  LAY(SAMSIM_A_PHI, 1) = phi;
  s1_layer<K>(c, x, 1, Na, do_ray, T, phi, S_bu, m, thick, recip(thick), r);
  if (do_ray && CFG(flood_flag) > 1 && CL(m_snow) > r.buoy_s * (rho_l - rho_s)) {   // (flood_handover's own test: the thickness of the bottom layer is only formed where it is used)
    THICK_RULE_INIT(tr);
    flood_handover<K>(c, x, r, r_below_top, THICK_AT(tr, Na));
  }
  c.neg_psi = r.min_psi_s < 0.0;
  c.buoy_s = r.buoy_s;
  if (rc) STOPC(rc, 1);
}

// Beer-law absorption alone (no gravity drainage this step): fl_rad(N_active), mo_heat_fluxes.f90:151-155
// temp2(k) = temp2(k-1) * exp(-extinc * thick(k)) from temp2(0) = beer0, and fl_rad(N_active) = temp2(Na-1) - temp2(Na): a chain of Na
// sequentially rounded products, so the order is the reference's and nothing is re-associated or raised to a power.  What varies is
// how the factor is found.  A column that follows the grid rule is walked as the fused sweeps walk it -- layer 1, top block, elastic
// block, bottom block -- with the factor formed where a stretch begins (exp is a function of its operand alone: the bits are those of
// a loop that forms it per layer, whichever layer that is) and the multiply alone inside: per layer one instruction where the
// per-layer form spends a thickness select, a `thick != th_prev` test with its exec-mask region around the inlined exp, a
// `k == Na` test with its region and the multiply.  A hand-made column keeps the per-layer form.
template <class K>
__device__ RARE void sweep_beer(Col &c, const Ctx &x, double beer0) {
  const samsim_config &g = x.p->cfg;
  const int Na = c.Na;   // (>= 1: samsim_set_state, and no regrid removes the last layer)
  // Polar night: no lane of the wave has short-wave radiation to absorb.  With temp2 = beer0 = +-0 and a factor e in [0, 1] (thick is
  // a positive number) every product temp2 * e is a zero of temp2's sign, and fl_rad = temp2 - temp2 * e is x - x of two equal zeros,
  // which rounds to +0.0 whatever their sign: the value set here.  (A NaN beer0 compares unequal and takes the walk.)  This assumes
  // finite positive thicknesses, as every valid state has: a NaN thick, or one below -355 m whose factor overflows, made the loop's
  // fl_rad a NaN (0 * NaN, 0 * inf) where this gives +0.0 -- in a column that is already lost.
  if (!wave_any(beer0 != 0.0)) { c.frad = 0.0; return; }
  if ((c.flags & COLF_REGULAR) != 0) {
    // the layer count as a scalar where the lanes (those of the wave that are here) agree on it, else the wave's maximum with each
    // lane's value kept at its own N_active; a lane's products past its bottom layer are not read
    const int n0 = __builtin_amdgcn_readfirstlane(Na);
    const bool same = !wave_any(Na != n0);
    const int kend = same ? n0 : wave_max(Na);
    const int b0 = g.n_top, b1 = g.n_top + g.n_middle;
    double temp2 = beer0, frad = 0.0;
    // (one copy of the stretch in the listing, and so of the inlined exp, walked four times: the pass is inlined at three places of
    // every step kernel, and the top and bottom blocks forming the same factor twice costs a column some forty instructions)
#pragma unroll 1
    for (int st = 0; st < 4; ++st) {
      const int klo = st == 0 ? 1 : (st == 1 ? 2 : (st == 2 ? b0 + 1 : b1 + 1));
      const int khi_s = st == 0 ? 1 : (st == 1 ? b0 : (st == 2 ? b1 : kend));
      if (klo > kend) break;
      if (klo > khi_s) continue;
      const int khi = khi_s < kend ? khi_s : kend;
      const double thick = st == 0 ? LAYU(SAMSIM_A_THICK, 1) : (st == 2 ? LAYU(SAMSIM_A_THICK, g.n_top + 1) : g.thick_0);
      const double e = exp(-extinc * thick);
      if (same) {
        const int kmul = khi < kend ? khi : kend - 1;    // (the product of layer N_active itself is only fl_rad's subtrahend)
        for (int k = klo; k <= kmul; ++k) temp2 = temp2 * e;
        if (khi == kend) frad = temp2 - temp2 * e;
      } else {
        for (int k = klo; k <= khi; ++k) {
          const double t = temp2 * e;
          if (k == Na) frad = temp2 - t;
          temp2 = t;
        }
      }
    }
    c.frad = frad;
  } else {
    double temp2 = beer0, e = 0.0, th_prev = -1.0;
    for (int k = 1; k <= Na; ++k) {
      const double thick = LAYU(SAMSIM_A_THICK, k);
      if (thick != th_prev) { e = exp(-extinc * thick); th_prev = thick; }
      if (k == Na) c.frad = temp2 - temp2 * e;
      temp2 = temp2 * e;
    }
  }
}

// sub_fl_Q, mo_thermo_functions.f90:201-223, between two layers: dT / (thick_a/(2 k_a) + thick_b/(2 k_b)).  With the half-layer
// conductance g = 2k/thick = 2k * (1/thick) -- 1/thick is at hand in the sweeps, one value per stretch of the grid -- the flux is
// dT * g_a*g_b / (g_a + g_b): one division per layer where the resistance form has two (a division is a quarter-rate reciprocal
// plus five instructions).  An ulp-level re-association like the shared reciprocals; both orders of the step use it.
__device__ __forceinline__ double heat_conductance(double psi_s, double psi_l, double rth) {
  return (2.0 * (psi_s * k_s + psi_l * k_l)) * rth;
}
__device__ __forceinline__ double heat_flux_between(double dT, double g_a, double g_b) {
  return quot(dT * (g_a * g_b), g_a + g_b);
}

// A copy of v in registers of its own, which the optimiser cannot fold back into v (to the compiler the move is an opaque
// instruction with one result): ends the life of the registers v sits in.  See the trip loop of sweep_down_fused.
__device__ __forceinline__ double out_of_row(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r;
  asm volatile("v_mov_b64 %0, %1" : "=v"(r) : "v"(v));
  return r;
#else
  return v;
#endif
}

// ---------------------------------------------------------------- D: fused down sweep (P2 + P3), top -> bottom
// One pass instead of two for the common step (not the first, not an output step, no thin-snow coupling, no flooding):
// per layer j   A(j) expulsion_flux + mass_transfer + S_bu refresh          (mo_mass.f90:112-136, 53-96; mo_grotz.f90:333)
//               [j = N_active: gas -> ocean water, bottom turbulence]        (mo_grotz.f90:405-410, 450-457)
//               B(j) gravity-drainage loss of layer j, fl_up(j)              (mo_grav_drain.f90:144-170)
//               C(j-1) return-flow mass_transfer into layer j-1, final store (mo_grav_drain.f90:174-193)
// A(j) of the reference runs for all layers before B starts, but A(j) only reads layers <= j and B/C(j-1) only layers
// j-1, j, so the interleaving computes the same values.  S_br(j) and S_br(j+1) of the first sweep are recomputed from
// T and the pre-expulsion S_abs/m (bit-identical), which needs the raw loads of layer j+1 one iteration early.
template <class K>
// store_default: whether the volume fractions of layers >= 3 are stored when the sweep does not decide itself; decide_psi: it
// decides after layer 2 (see there), storing them anyway under store_default; surface_done: the sweep evaluated the surface balance
// couple: this column has a thin snow cover (snow_coupling, mo_grotz.f90:418-420, between the brine expulsion and the drainage);
// late_rad: some column of the wave has, so the radiation header and the Beer-law pass -- which read the snow temperature the
// coupling sets -- run inside the sweep, after the top two layers (time, tc, do_beer are theirs)
// COLF_FLOODED: this column was flooded before the sweep (column_step, from a dry run of the expulsion): layer 1 takes the flooded
// salt, enthalpy, mass and thickness (hand-over block) where the unfused order's flood() would have changed the arrays -- after its
// expulsion and mass_transfer, before its drainage -- and the bottom layer the increments of an instant flooding (COLF_FLOOD_DEEP)
__device__ __forceinline__ void sweep_down_fused(Col &c, const Ctx &x, bool store_default, bool decide_psi, bool &surface_done,
                                                 bool couple, bool late_rad, double time, int tc, bool do_beer) {
  const samsim_config &g = x.p->cfg;
  const Salt &s = x.salt;
  const int Na = c.Na;
  const double dt = g.dt;
  double heat_loss = 0.0, cum = 0.0, sum_before = 0.0, sum_after = 0.0, minS = 1.0e300;
  double fb_a2 = 0.0, fb_g2 = 0.0;       // SUM(psi_s*thick), SUM(psi_g*thick) over layers >= 2 for func_freeboard (see there)
  int stop_layer = 0;
  bool store_psi = true;                 // layers 1 and 2 always; the others as decided after layer 2 (below)
  // conductive heat fluxes (sub_heat_fluxes, mo_heat_fluxes.f90:272-285): see C(j-1) below
  double g_up = 0.0, flq_up = 0.0;       // half-layer conductance 2k/thick of layer j-1, fl_Q(j-1)
  double esum = 0.0;                     // SUM(H_abs before - after) of the conductive update, for the energy assert

  // The sweeps are latency bound (a wave waits on memory for most of its life), so the loads run ahead of the arithmetic:
  // the six values of layer j+2 are requested at the top of iteration j and first touched in iteration j+1 (S_br of the
  // layer below is needed one layer early), which puts a full iteration of work between request and use.  Measured on the
  // default bench: loads at use 82.3 ms per launch, one layer ahead 76.0, two ahead at 3 waves/SIMD 73.8 (two ahead at
  // 4 waves/SIMD spills inside the loop: 93).
  // Operands run two iterations ahead of the arithmetic with two request buffers and ONE finished layer: the operands of layer
  // j+2 are requested at the top of iteration j and turned into `raw` at the END of iteration j+1.  (Round 1 and the first half of
  // round 2 finished layer j+1 at the top of iteration j, because the drainage test of B(j) compares S_br(j) with S_br(j+1): one
  // iteration of lead, a second finished layer -- 18 registers -- held for the sake of a test that is reached in a fifth of the
  // layers.  That test now forms S_br(j+1) from the request buffer on demand.)
  struct Ld { double T, S_abs, m, H_abs, ray; };
  struct Raw { double T, S_abs, m, S_bu, S_br, H_abs, ray, H; };
  // This sweep only runs on columns that follow the grid rule: the interior layers are walked in three stretches (top block,
  // elastic block, bottom block), inside each of which thick and 1/thick are one value -- the loop body neither loads nor selects
  // them (round 2 formed them per layer from the configuration, which the compiler re-read from memory inside the loop).  The
  // two values are formed where a stretch begins (the elastic block's thickness is one load per sweep), so that nothing but the
  // current pair is carried through the loop.
  auto load_ld = [&](int j) -> Ld {
    Ld r;
    r.T = LAYU_LD(SAMSIM_A_T, j);
    r.S_abs = LAYU_LD(SAMSIM_A_S_ABS, j);
    r.m = LAYU_LD(SAMSIM_A_M, j);
    r.H_abs = LAYU_LD(SAMSIM_A_H_ABS, j);
    // (the row flags are read from LDS at every layer: a word kept across iterations is one more value the allocator spills,
    // and a scratch reload drains every outstanding request of the sweep)
    r.ray = (j <= Na - 1 && ray_row_valid(c, x, j)) ? LAYU(SAMSIM_A_RAY, j) : 0.0;
    return r;
  };
  auto finish = [&](const Ld &l, int j) -> Raw {
    Raw r;
    r.T = l.T; r.S_abs = l.S_abs; r.m = l.m; r.H_abs = l.H_abs; r.ray = l.ray;
    per_mass(r.S_abs, r.H_abs, r.m, r.S_bu, r.H);   // as the first sweep formed them
    r.S_br = S_br_clamped(s, r.T, r.S_bu);
    return r;
  };
  auto S_br_below = [&](const Ld &l) -> double {    // S_br of the layer in a request buffer, exactly as finish() will form it
    double S_bu, H;
    per_mass(l.S_abs, l.H_abs, l.m, S_bu, H);
    return S_br_clamped(s, l.T, S_bu);
  };
  // (SA, mA: salt and mass right after A(j).  Their quotient, the refreshed bulk salinity of mo_grotz.f90:333-335, is only
  // read where brine actually moves -- the drainage test of B(j) and the return-flow transfers of C -- so it is formed there:
  // same operands, same quotient, one division less in the nine layers out of ten that do not drain)
  // (ch: brine moved in or out of the layer -- expulsion, drainage, return flow -- so its mass or salt changed.  In winter that
  // holds in a quarter of the layer rows of a wave; elsewhere m and S_abs would be stored with the bits they were loaded with,
  // and the stores are skipped: 16 of the 88 bytes a layer-cell moves per step.)
  struct Lay { double T, SA, mA, S_abs, H_abs, m, flup; bool ch; };

  double flm_j = 0.0;                                  // fl_m(j) of expulsion_flux
  double T_up = 0.0, S_br_up = 0.0, S_abs_up = 0.0;    // layer j-1 as mass_transfer #1 sees it
  // (requests are issued unconditionally, from a clamped row where the layer does not exist -- see sweep_up_fused)
  const int N = c.N;
  Raw raw = finish(load_ld(1), 1);
  Ld ahead = load_ld(2), ahead2 = ahead;               // layers j+1 and j+2 (nlayer >= 3, samsim_create)
  Lay prev = {0, 0, 1, 0, 0, 0, 0, true};              // layer j-1 after A and B, waiting for C
  double flup_pp = 0.0;                                // fl_up(j-2)
  // One layer of the sweep: A(j), B(j), C(j-1).  LAST = the column's bottom layer N_active, which differs from lane to lane: it
  // runs after the loop (once per wave, every lane with its own j), so that the loop body -- the interior layers -- carries
  // neither the bottom-layer work (gas -> ocean water, the bottom turbulence with its exp and two pow) nor its registers.
  auto layer = [&](const int j, const Ld &below, const double thick, const double rth, auto last_tag, auto first_tag) {   // below: the request buffer that holds layer j+1
    constexpr bool LAST = decltype(last_tag)::value, FIRST = decltype(first_tag)::value;
    if (!LAST && !FIRST) { ISA_MARK("D_LAYER_A"); }
    // ---- A(j)
    // Expulsion of the first sweep (mo_grotz.f90:306), re-evaluated from its inputs phi, thick, m
    double H_abs = raw.H_abs;
    const Expelled ex = expulsion(phi_from_T(s, raw.H, raw.S_bu, raw.S_br), thick, raw.m, rth);
    const double V_ex = ex.V_ex;
    double psi_g = ex.psi_g, m = raw.m, S_abs = raw.S_abs;
    const double T = raw.T, S_br = raw.S_br;
    double flm_next;
    if (j == 1 || psi_g < (double)0.001f) {
      flm_next = (j == 1) ? -V_ex * rho_l : -V_ex * rho_l + flm_j;
    } else {
      flm_next = -dmax((V_ex - psi_g * thick) * rho_l, 0.0);
      psi_g = dmax(quot(psi_g * thick - V_ex, thick), 0.0);
    }
    if (!FIRST) { fb_a2 += ex.psi_s * thick; fb_g2 += psi_g * thick; }
    // The up sweep only needs the layer's half resistance thick/(2k) (sub_fl_Q, mo_thermo_functions.f90:201-223); the three
    // volume fractions are stored when something reads them this step (see column_step), and always for layer 1
    if (store_psi || j == 1) {
      LAYU(SAMSIM_A_PSI_S, j) = ex.psi_s;
      LAYU(SAMSIM_A_PSI_L, j) = ex.psi_l;
      LAYU(SAMSIM_A_PSI_G, j) = psi_g;
    }
    // sub_fl_Q (mo_thermo_functions.f90:201-223): fl_Q(j) = (T(j) - T(j-1)) / (thick(j-1)/(2k(j-1)) + thick(j)/(2k(j))) with the
    // temperatures and volume fractions of the first sweep, k = psi_s*k_s + psi_l*k_l (the reference adds psi_g*0._wp: a no-op),
    // evaluated through the half-layer conductances (heat_flux_between);
    // th_l: the thickness the conduction and the drainage see (flooding changes layer 1's after the expulsion)
    const bool flooded_here = FIRST && (c.flags & COLF_FLOODED) != 0;
    const double th_l = flooded_here ? LAYU(SAMSIM_A_THICK, 1) : thick;
    const double gj = heat_conductance(ex.psi_s, ex.psi_l, flooded_here ? recip(th_l) : rth);
    const double flq = (j >= 2) ? heat_flux_between(T - prev.T, g_up, gj) : 0.0;
    if (j == 2) c.flq2 = flq;
    m = m + flm_next - flm_j;
    if (flm_next < 0.0) {
      H_abs = H_abs + flm_next * T * c_l;
      S_abs = S_abs + dmax(flm_next * S_br, -S_abs);
    }
    if (flm_j < 0.0) {
      H_abs = H_abs - flm_j * T_up * c_l;
      S_abs = S_abs - dmax(flm_j * S_br_up, -S_abs_up);
    }
    bool ch = LAST || (flm_next < 0.0) || (flm_j < 0.0);
#if SAMSIM_STAMPS == 2
    if (!LAST && !FIRST) {   // rows of the interior in which the expulsion moves no brine in any column of the wave (m and S_abs keep their bits)
      ST_COUNT(CT_ROWS, 1);
      if (__ballot(flm_next < 0.0 || flm_j < 0.0) == 0ull) ST_COUNT(CT_ROWS_STILL, 1);
    }
#endif
    const double SA = S_abs, mA = m;     // S_bu = SA / mA: refreshed bulk salinity, mo_grotz.f90:333-335 (formed where it is read)
    S_br_up = S_br;                      // (T_up and S_abs_up, the other two values mass_transfer #1 of the next layer sees: at the end of the layer)
    flm_j = flm_next;
    // Thin-snow coupling (mo_grotz.f90:418-420) sits between expulsion / mass_transfer and everything below in the reference.  It
    // reads and writes layer 1 only, and layer 1 is through with the expulsion here (its own flux and the one into layer 2 are
    // applied), so it runs now, on the registers: the transfers above moved brine at the temperature of the first sweep, the
    // drainage, the return flow and the conductive flux below see the coupled one -- the unfused order, operation for operation.
    double Tl = T;
    if (FIRST && couple) {
      double phi1 = LAYU(SAMSIM_A_PHI, 1);
      const double S_bu1 = S_abs / m;   // as sweep_expulsion_transfer stores it (mo_grotz.f90:333), and in the array: the second
      LAYU(SAMSIM_A_S_BU, 1) = S_bu1;   // coupling of the step (sub_heat_fluxes, in the up sweep's top-layer block) reads it there
      const int rcc = snow_coupling_core<K>(c, x, H_abs, m, S_bu1, Tl, phi1);
      LAYU(SAMSIM_A_T, 1) = Tl;
      LAYU(SAMSIM_A_PHI, 1) = phi1;
      if (rcc && !c.status) { c.status = rcc; x.err_step[c.col] = c.step + 1; x.err_layer[c.col] = 1; }
    }
    if (flooded_here) {   // flooding (mo_grotz.f90:428-445) sits here in the reference's order: flood() on the finished expulsion
      S_abs = SPEC(SP_FLD_S1); H_abs = SPEC(SP_FLD_H1); m = SPEC(SP_FLD_M1);
      ch = true;
      c.flags &= ~COLF_FLOODED;
    }
    if (LAST) {
      if (psi_g > 0.0) {  // bottom-layer gas -> ocean water
        const double t2 = psi_g * thick * rho_l;
        m = m + t2;
        S_abs = S_abs + t2 * x.S_bu_bottom;
        H_abs = H_abs + t2 * c_l * g.T_bottom;
      }
      if (c.flags & COLF_FLOOD_DEEP) {   // instant flooding below neg_free: ocean water into the bottom layer (mo_flood.f90:118-121)
        S_abs = S_abs + SPEC(SP_FL_HP);
        H_abs = H_abs + SPEC(SP_FL_SALL);
        c.flags &= ~COLF_FLOOD_DEEP;
      }
      if (CFG(turb_flag) == 2) {  // sub_turb_flux
        const double turb = Turb_A * exp(Turb_B * (-ocean_density<K>(x) + func_density(T, quot(S_abs, m)))) * dt;
        S_abs = S_abs - turb * (S_abs / m - x.S_bu_bottom);
      }
    }
    // ---- B(j)
    if (!LAST && !FIRST) { ISA_MARK("D_LAYER_B"); }
    ST_MARK(ST_D_A);
    sum_before += S_abs;
    double flup = cum;
    if (!LAST) {
      const double ray = raw.ray;
      // S_br(j+1) of the first sweep, from the request buffer of layer j+1 (same operands and operations as finish())
      if (ray > ray_crit && S_br > S_br_below(below)) {
        const double psi_s = ex.psi_s;
        if (psi_s > 0.001 && (flooded_here ? quot(S_abs, m) : quot(SA, mA)) > 0.1) {  // S_bu of this layer (j < N_active: nothing but a flooding changed it since A)
          ST_COUNT(CT_DRAIN_WAVE, 1);
          ST_COUNT(CT_DRAIN_LANE, (unsigned long long)__popcll(__ballot(1)));
          const double psi_l = ex.psi_l;
          double flux = x_grav * (ray - ray_crit) * dt * th_l;
          flux = dmin(flux, psi_l * rho_l * th_l);
          S_abs = S_abs - flux * S_br;
          if (S_abs < 0.0 && !stop_layer) stop_layer = j;
          CL(grav_temp) = CL(grav_temp) + flux * Tl;
          H_abs = H_abs - flux * c_l * Tl;
          heat_loss = heat_loss + flux * c_l * Tl;
          cum = cum + flux;
          flup = dmin(cum, psi_l * rho_l * th_l);
          ch = true;
        }
      }
    }
    sum_after += S_abs;
#if defined(__HIP_DEVICE_COMPILE__)
    // (the two sums are formed here, not wherever the scheduler finds room for them in the following layers: a deferred addition
    // keeps S_abs of this layer alive in the registers of its request buffer, past the point where the buffer is requested into again)
    asm volatile("" : "+v"(sum_before), "+v"(sum_after));
#endif
    if (!LAST && !FIRST) { ISA_MARK("D_LAYER_C"); }
    // ---- C(j-1): layer j-1 receives from layer j (fl_m(j) = fl_up(j-1)) and gives to j-2 (fl_m(j-1) = fl_up(j-2))
    if (j > 1) {
      if (prev.flup > 0.0) {
        prev.H_abs = prev.H_abs + prev.flup * T * c_l;
        prev.S_abs = prev.S_abs + dmin(prev.flup * S_br_clamped(s, T, quot(SA, mA)), S_abs);
        prev.ch = true;
      }
      if (flup_pp > 0.0) {
        prev.H_abs = prev.H_abs - flup_pp * prev.T * c_l;
        prev.S_abs = prev.S_abs - dmin(flup_pp * S_br_clamped(s, prev.T, quot(prev.SA, prev.mA)), prev.S_abs);
        prev.ch = true;
      }
      // The brine transports of layer j-1 are complete: what the reference does next to its enthalpy is the explicit conductive
      // update of sub_heat_fluxes, H_abs(k) += (fl_Q(k+1) - fl_Q(k))*dt, then += fl_rad(N_active)*dt (mo_heat_fluxes.f90:277-285:
      // sic, the bottom layer's absorption in every layer).  Both fluxes are at hand here -- old temperatures, this step's volume
      // fractions -- so the down sweep applies it and the up sweep neither reads T and the half resistances nor writes H_abs.
      // Layer 1 takes fl_Q(1) from the surface balance, which needs the finished layer 1: the top-layer block does it.
      if (j - 1 >= 2) {
        const double H_b = prev.H_abs;
        prev.H_abs = prev.H_abs + (flq - flq_up) * dt;
        prev.H_abs = prev.H_abs + c.frad * dt;
        esum += H_b - prev.H_abs;
      }
      if (wave_any(prev.ch)) {   // (wave-uniform: a row is stored for all its columns or for none)
        LAYU(SAMSIM_A_M, j - 1) = prev.m;
        LAYU(SAMSIM_A_S_ABS, j - 1) = prev.S_abs;
      }
      LAYU(SAMSIM_A_H_ABS, j - 1) = prev.H_abs;
      minS = dmin(minS, prev.S_abs);
      flup_pp = prev.flup;
    }
    g_up = gj; flq_up = flq;
    // T, and H_abs, SA and S_abs wherever no brine moved, are still the values the row was loaded with, in the registers of its
    // request buffer: out_of_row() takes them out, so that the buffer is free for the next request (see the trip loop below)
    T_up = out_of_row(T); S_abs_up = out_of_row(SA);
    prev.T = FIRST ? out_of_row(Tl) : T_up; prev.SA = S_abs_up; prev.mA = mA; prev.S_abs = out_of_row(S_abs); prev.H_abs = out_of_row(H_abs);
    prev.m = m; prev.flup = flup; prev.ch = ch;
    if (!LAST && !FIRST) { ISA_MARK("D_LAYER_END"); }
    ST_MARK(ST_D_B);
  };
  const int jmax = wave_max(Na);
  auto request = [&](const int j) { ahead2 = load_ld(j + 2 <= N ? j + 2 : N); };      // top of iteration j: layer j+2
  auto advance = [&](const int j) { raw = finish(ahead, j + 1); ahead = ahead2; };      // end of iteration j: layer j+1 becomes current
  // ---- layers 1 and 2 (where they are interior layers), volume fractions always stored
  const double thick1 = (c.flags & COLF_FLOODED) ? SPEC(SP_FLD_TH1_BEFORE) : LAYU(SAMSIM_A_THICK, 1);   // (the expulsion of layer 1 saw the unflooded thickness)
  if (1 < Na) { request(1); layer(1, ahead, thick1, recip(thick1), std::false_type{}, std::true_type{}); advance(1); }
  if (2 < Na) { request(2); layer(2, ahead, g.thick_0, recip(g.thick_0), std::false_type{}, std::false_type{}); advance(2); }   // (N_top >= 3: samsim_create)
  if (late_rad) {   // (see the head of the routine; nothing above reads fl_rad, the albedo or the short-wave flux)
    const double beer0 = radiation_header<K>(c, x, time, tc);
    c.frad = 0.0;
    if (do_beer) sweep_beer<K>(c, x, beer0);
  }
  // ---- Who reads the psi_s / psi_l / psi_g rows of the layers below?  The vital signs at the next output point and a get_state
  // after the launch (force_psi), and -- when the surface melts or the snow releases melt water -- func_freeboard and flush3
  // (mo_grotz.f90:636,670,717-725).  With N_active >= 3 layer 1 is complete by now (its return-flow transfer C(1) ran with
  // layer 2), and everything those late readers' conditions depend on can be evaluated exactly: the surface balance
  // (sub_heat_fluxes' first part reads layer 1, the snow and the forcing, none of which the rest of this sweep touches), hence
  // T_top, fl_Q(1) and fl_Q_snow; the freezing point of layer 1 (S_abs(1), m(1) stay as they are unless wet snow adds slush);
  // the snow's enthalpy after the heat fluxes, hence whether the second snow_thermo of the step can find it wet.  The rows are
  // skipped only when none of the conditions can hold, so a late reader never meets a column without them (refill_psi_rows is
  // the safety net; tests/test_gpu_melt_onset.py runs a wave of columns through their melt onsets, and with the counter build
  // asserts that no lane calls it).
  if (decide_psi && Na >= 3) {
    surface_flux<K>(c, x);
    surface_done = true;
    const double thick_min = g.thick_min;
    const double Tf = func_T_freeze(quot(LAYU(SAMSIM_A_S_ABS, 1), LAYU(SAMSIM_A_M, 1)), CFG(salt_flag), x.tf_c3);   // as mo_grotz.f90:634 will
    bool snow_wet = false;
    if (CL(thick_snow) > 0.0) {
      // snow_thermo finds liquid water iff H_abs_snow / m_snow > -latent_heat (getT's fresh branch); the up sweep adds
      // (fl_Q(1) - fl_Q_snow)*dt to a snow cover thicker than thick_min.  A thinner one does come here (its coupling runs inside
      // this sweep) and exchanges heat with layer 1 as well: it counts as wet whatever its enthalpy
      const double H_new = CL(H_abs_snow) + (CL(fl_Q1) - CL(fl_Q_snow)) * dt;
      snow_wet = !(CL(thick_snow) >= thick_min) || !(H_new / CL(m_snow) <= -latent_heat);
    }
    store_psi = store_default || LAYU(SAMSIM_A_PSI_S, 1) < psi_s_top_min || CL(T_top) >= Tf || snow_wet || CL(melt_thick_snow) > 0.0;
  } else {
    store_psi = store_default || decide_psi;   // (a deciding sweep over fewer than three layers has nothing left to skip)
  }
  c.psi_full = store_psi;
  // The interior layers 3 <= j < N_active, three per trip.  Three rows are alive at any layer -- the layer's own (`raw`, which
  // finish() forms in the registers of the buffer it was requested into), the next one and the one being requested -- so the
  // roles go round the three buffers once in three layers: with three layers in one loop body no buffer is copied into another
  // and the hand-over of layer j to C(j) of the next layer is a renaming.  (One layer per trip spent 35 of its 265 vector
  // instructions on those copies; two per trip still ended every trip by copying the row it had requested one layer before into
  // the registers the next trip expects it in, behind `s_waitcnt vmcnt(3..0)`: a full drain, the second layer's own stores
  // included, every other layer.)  A column whose interior layers end inside a trip, and the 0-2 layers a stretch has left
  // over, take single-layer steps that do copy their buffer (at most two per column and six per wave and sweep).
  // A row's VALUES live for four layer bodies, though, not three: requested two layers ahead, `raw` for a layer -- and then T,
  // and H_abs / S_abs where no brine moved, go on as `prev`, T_up and S_abs_up until C and A of the next layer, in the registers
  // they were loaded into.  A buffer that is busy for four layers does not go round in three: the third request of the trip
  // went into registers of its own and was copied into the buffer on the back edge, while still outstanding, behind
  // `s_waitcnt vmcnt(0)` -- the last full drain of the trip.  So the layer ends by moving what lives on out of the row
  // (out_of_row: at most four 64-bit moves, behind a wait the layer has had anyway) and by forming its two salt sums where the
  // source has them: the buffer is then dead when it is requested into again, and the back edge carries no copy and no wait.
  {
    const int b0 = g.n_top, b1 = g.n_top + g.n_middle;
    Ld ahead3 = ahead;
    auto single = [&](const int j, const double th_s, const double rth_s) {
      ahead2 = load_ld(j + 2 <= N ? j + 2 : N);
      layer(j, ahead, th_s, rth_s, std::false_type{}, std::false_type{});
      raw = finish(ahead, j + 1);
      ahead = ahead2;
    };
    int j = 3;
    for (int stretch = 0; stretch < 3; ++stretch) {
      const int hi_s = stretch == 0 ? b0 : (stretch == 1 ? b1 : N);
      const int hi = hi_s < jmax - 1 ? hi_s : jmax - 1;           // last interior layer of the stretch in the longest column of the wave
      const double th_s = stretch == 1 ? LAYU(SAMSIM_A_THICK, g.n_top + 1) : g.thick_0, rth_s = recip(th_s);
      for (; j + 2 <= hi; j += 3) {
        ISA_MARK("D_ITER_BEGIN");
        ST_MARK(ST_DFUSED);
        if (j + 2 < Na) {                                  // all three are interior layers of this column: one straight-line body
          ST_COUNT(CT_DOWN_TRIPS, 3);
          ahead2 = load_ld(j + 2 <= N ? j + 2 : N);        // layer j+2 -> second buffer
          layer(j, ahead, th_s, rth_s, std::false_type{}, std::false_type{});
          raw = finish(ahead, j + 1);
          ahead3 = load_ld(j + 3 <= N ? j + 3 : N);        // layer j+3 -> third buffer
          layer(j + 1, ahead2, th_s, rth_s, std::false_type{}, std::false_type{});
          raw = finish(ahead2, j + 2);
          ahead = load_ld(j + 4 <= N ? j + 4 : N);         // layer j+4 -> first buffer
          layer(j + 2, ahead3, th_s, rth_s, std::false_type{}, std::false_type{});
          raw = finish(ahead3, j + 3);
        } else if (j < Na) {                               // the column's interior layers end with layer j or j+1
          ISA_MARK("D_RARE_BEGIN");
          ST_COUNT(CT_DOWN_TRIPS, 1);
          single(j, th_s, rth_s);
          if (j + 1 < Na) { ST_COUNT(CT_DOWN_TRIPS, 1); single(j + 1, th_s, rth_s); }
        }
        ISA_MARK("D_ITER_END");
      }
      for (; j <= hi; ++j) {                               // the layers the stretch has left over
        if (j < Na) single(j, th_s, rth_s);
      }
    }
  }
  const double thick_Na = (Na > g.n_top && Na <= g.n_top + g.n_middle) ? LAYU(SAMSIM_A_THICK, g.n_top + 1) : g.thick_0;
  layer(Na, ahead, thick_Na, recip(thick_Na), std::true_type{}, std::false_type{});   // the bottom layer (this sweep only runs with N_active >= 2)
  // ---- C(Na): the ocean below (ghost cell of mass_transfer, mo_mass.f90:70-72)
  if (prev.flup > 0.0) {
    prev.H_abs = prev.H_abs + prev.flup * g.T_bottom * c_l;
    prev.S_abs = prev.S_abs + dmin(prev.flup * S_br_clamped(s, g.T_bottom, x.S_bu_bottom), x.S_bu_bottom * 2000.0);
  }
  if (flup_pp > 0.0) {
    prev.H_abs = prev.H_abs - flup_pp * prev.T * c_l;
    prev.S_abs = prev.S_abs - dmin(flup_pp * S_br_clamped(s, prev.T, quot(prev.SA, prev.mA)), prev.S_abs);
  }
  CL(grav_drain) = CL(grav_drain) + prev.flup;
  if (CFG(grav_heat_flag) == 2) prev.H_abs = prev.H_abs + heat_loss - prev.flup * c_l * g.T_bottom;
  // conductive update of the bottom layer: fl_Q(N_active+1) = fl_q_bottom (this sweep only runs with N_active >= 2)
  {
    const double H_b = prev.H_abs;
    prev.H_abs = prev.H_abs + (c.fl_q_bottom - flq_up) * dt;
    prev.H_abs = prev.H_abs + c.frad * dt;
    c.esum = esum + (H_b - prev.H_abs);
  }
  LAYU(SAMSIM_A_M, Na) = prev.m;
  LAYU(SAMSIM_A_S_ABS, Na) = prev.S_abs;
  LAYU(SAMSIM_A_H_ABS, Na) = prev.H_abs;
  minS = dmin(minS, prev.S_abs);
  if (store_psi) { SPEC(SP_FB_A2) = fb_a2; SPEC(SP_FB_G2) = fb_g2; }   // (read by func_freeboard, which only runs where the rows were stored)
  CL(grav_salt) = CL(grav_salt) + sum_before;
  CL(grav_salt) = CL(grav_salt) - sum_after;
  if (stop_layer) STOPC(21234, stop_layer);
  if (minS < 0.0) STOPC(1337, 0);
}

// ---------------------------------------------------------------- U: fused up sweep (P4 + next step's S1), bottom -> top
// sweep_heat_thermo plus, for layers N_active..2, the first sweep of the NEXT time step: that sweep would divide the
// same H_abs by the same m and start Newton from the same guesses (T_bottom, then the layer below), so its T and phi
// are exactly the ones just computed.  What it adds -- S_br, Expulsion, permeability, Rayleigh number -- is done here
// from registers and written to the NEXT psi buffers (nps/npl/npg), because this step's remaining readers (melt film,
// freeboard, flush3) still need the current ones.  Layer 1 is left to prologue_top_layer: snow, melt water and the
// regrid trigger all act on it between the two steps.  If flushing or a regrid changes deeper layers afterwards, the
// column is flagged COLF_DIRTY and the next step runs the full first sweep instead.
template <class K>
__device__ __forceinline__ void sweep_up_fused(Col &c, const Ctx &x, long long col, bool next_is_output, bool store_phi) {
  const samsim_config &g = x.p->cfg;
  const Salt &s = x.salt;
  const int Na = c.Na;
  const double dt = g.dt, thick_min = g.thick_min;
  const bool thin_snow = (CL(thick_snow) >= thick_min / 100.0 && CL(thick_snow) < thick_min);
  const bool do_ray = (CFG(grav_flag) >= 2 && Na > 1);
  const bool keep_ray = next_is_output && col >= x.out_col0 && col < x.out_col0 + x.out_ncols;
  const double H_abs_snow_before = CL(H_abs_snow);
  double esum = c.esum;   // SUM(H_abs before - after the conductive update) over the layers >= 2, from the down sweep
  double T_test = g.T_bottom;
  int rc = 0, rc_layer = 0;
  RayScan r;
  ray_scan_init(r);
  if (keep_ray) {  // `output` prints the Rayleigh numbers of THIS step's fl_grav_drain at the next step's output point
    const size_t oc = (size_t)(col - x.out_col0), on = (size_t)x.out_ncols;
    for (int k = 1; k <= c.N - 1; ++k) x.out_lay[((size_t)SAMSIM_A_RAY * c.N + (k - 1)) * on + oc] = LAYU(SAMSIM_A_RAY, k);
  }
  for (int w = 0; w <= (c.N - 1) >> 6; ++w) x.rflag[w] = 0ull;   // every lane writes the same zeros
  __builtin_amdgcn_wave_barrier();
  if (do_ray && Na <= c.N - 1 && x.ray_rows_all) LAYU(SAMSIM_A_RAY, Na) = 0.0;   // (read by `output` only)
  // The conductive update of layers >= 2 has been applied by the down sweep (sweep_down_fused / sweep_heat_down), which also
  // hands over fl_Q(2) and the energy sums: this sweep reads the finished enthalpy and runs the second getT chain -- and, for
  // layers N_active..2, the first sweep of the next step.  Its operands (H_abs, m, S_abs, thick of a layer) are requested TWO
  // iterations ahead, unconditionally and from a clamped row where the layer does not exist: the hardware counts outstanding
  // memory operations in order, and the compiler can only wait for "all but the N youngest" when every path through the loop
  // body issues the same operations -- one conditional request and it falls back to draining them all.
  // The thicknesses: a wave whose columns all follow the grid rule (COLF_REGULAR: every layer but the first is thick_0, except the
  // N_middle elastic layers, which share thick(N_top+1)) walks the column in three stretches -- bottom block, elastic block, top
  // block -- inside each of which thick and 1/thick are the same for every layer: the loop body neither loads nor selects them.  A
  // wave with a hand-made column loads the array with the other operands and forms 1/thick per layer.
  struct UL { double th, H, m, S; };
  const bool regular_wave = !wave_any((c.flags & COLF_REGULAR) == 0);
  UL cur, nxt, nn;
  bool alive = true, neg_salt = false;
  // One layer of the sweep.  TOP = layer 1, which alone meets the snow (mo_heat_fluxes.f90:291-303) and takes fl_Q(1) from the
  // surface balance: it runs after the loop, so that the loop body -- the same for every other layer -- carries neither the
  // thin-snow coupling (up to 200 getT pairs) nor its registers.
  // LITE: a wave with a column that flushed in the previous step will flush again in this one, after this sweep: flush3 rewrites
  // every layer of that column, so the wave runs the full first sweep in the next step whatever this sweep prepares (the sweep costs
  // a wave the same for one column as for 64) -- it then only runs the second getT chain, and says so for all its columns
  // (COLF_DIRTY: the full first sweep gives a column the same bits as the fused one).  A wave that does not flush after all has lost
  // nothing but the fused first sweep of one step.
  // (NewtonConsts: three constants of getT's evaluation as vector values, formed where a stretch of layers begins -- six v_mov_b32
  // per sweep and stretch instead of per layer -- and carried through the trip loop)
  NewtonConsts nc_s = newton_consts(s);   // (a wave with a hand-made column keeps this one for the whole sweep)
  auto body = [&](const int k, const UL &row, const double th_k, const double rth_k, auto top_tag, auto lite_tag) {
    constexpr bool TOP = decltype(top_tag)::value;
    constexpr bool LITE = decltype(lite_tag)::value;
    const double H_k = row.H, m_k = row.m, S_k = row.S;
    double H_abs = H_k;
    const double m = m_k;
    if (TOP) {
      // conductive update of layer 1: fl_Q(2) from the down sweep (fl_q_bottom under a single layer), fl_Q(1) from the surface balance
      const double flq_below = (Na >= 2) ? c.flq2 : c.fl_q_bottom;
      const double H_b = H_abs;
      H_abs = H_abs + (flq_below - CL(fl_Q1)) * dt;
      H_abs = H_abs + c.frad * dt;
      // snow treatment, mo_heat_fluxes.f90:291-303
      if (thin_snow) {
        CL(H_abs_snow) = CL(H_abs_snow) - CL(fl_Q_snow) * dt;
        LAYU(SAMSIM_A_H_ABS, 1) = H_abs;
        snow_coupling<K>(c, x);
        if (c.status) { alive = false; return; }
        H_abs = LAYU(SAMSIM_A_H_ABS, 1);
      } else if (CL(thick_snow) >= thick_min) {
        CL(H_abs_snow) = CL(H_abs_snow) + (CL(fl_Q1) - CL(fl_Q_snow)) * dt;
      }
      esum += H_b - H_abs;   // (after the thin-snow coupling, which moves enthalpy between the snow and layer 1)
      LAYU(SAMSIM_A_H_ABS, 1) = H_abs;
    }
    double S_abs = S_k;
    double S_bu, H;
    per_mass(S_abs, H_abs, m, S_bu, H);
    double T, phi = 0.0, S_br_T = 0.0;   // S_br_T: the liquidus salinity at T, formed once for phi and for the first sweep of the next step
    if (!TOP) { ISA_MARK("U_GETT_BEGIN"); }
    ST_MARK(ST_U_HEAD);
#if SAMSIM_STAMPS == 2
    int evals = 1;
    int rr = TOP ? getT(s, H, S_bu, T_test, T, phi, &evals) : getT_chain<LITE>(s, H, S_bu, T_test, T, phi, &evals, LITE ? nullptr : &S_br_T, &nc_s);
    {
      if (!TOP) { ST_COUNT(CT_ABOVE_ROWS, 1); if (__ballot(evals < 0)) ST_COUNT(CT_ABOVE_FAST, 1); }   // (bit 31: the wave-level shortcut of getT_chain decided `above`)
      evals &= 0x7fffffff;
      const bool was_odd = (evals >> 30) & 1;
      const int redo = (evals >> 16) & 0x3fff;
      evals &= 0xffff;
      const unsigned long long om = __ballot(was_odd);
      if (om) { ST_COUNT(CT_ODD_LANES, (unsigned long long)__popcll(om)); ST_COUNT(CT_ODD_WAVES, 1); ST_COUNT(CT_ODD_EVALS_WAVE, (unsigned long long)wave_max(redo)); }
    }
    ST_COUNT(CT_UP_TRIPS, 1);
    ST_COUNT(CT_NEWTON_WAVE, (unsigned long long)wave_max(evals));
    { int tot = 0; unsigned long long mk = __ballot(1); while (mk) { const int ln = __ffsll((long long)mk) - 1; tot += __builtin_amdgcn_readlane(evals, ln); mk &= mk - 1; }
      ST_COUNT(CT_NEWTON_LANE, (unsigned long long)tot); }
#else
    int rr = TOP ? getT(s, H, S_bu, T_test, T, phi) : getT_chain<LITE>(s, H, S_bu, T_test, T, phi, nullptr, LITE ? nullptr : &S_br_T, &nc_s);
#endif
    if (!TOP) { ISA_MARK("U_GETT_END"); }
    ST_MARK(ST_U_GETT);
    if (rr && !rc) { rc = rr; rc_layer = k; }
    T_test = T;
    LAYU(SAMSIM_A_T, k) = T;
    // the down sweeps recompute phi from T; the array is kept for its readers: the regrid trigger and layer_dynamics (bottom
    // two active layers), layer 1, the output snapshot and get_state
    if (store_phi || TOP || k >= Na - 1) LAYU(SAMSIM_A_PHI, k) = phi;
    if (!TOP && !LITE) {
      // first sweep of the next step for this layer (its own S_abs < 0 clamp first, mo_grotz.f90:812-818)
      // (a clamped salt mass changes S_bu and therefore T: such a column is left to the full sweep, flagged after the loop -- a
      // read-modify-write of the column's flag word inside the loop is one more value for the allocator to spill there)
      neg_salt = neg_salt || (S_abs < 0.0);
      s1_layer<K>(c, x, k, Na, do_ray, T, phi, S_bu, m, th_k, rth_k, r, true, &S_br_T);
    }
    ST_MARK(ST_U_TAIL);
  };
  const int kmax = wave_max(Na);
  auto load3 = [&](int j) -> UL { UL u; u.th = 0.0; u.H = LAYU_LD(SAMSIM_A_H_ABS, j); u.m = LAYU_LD(SAMSIM_A_M, j); u.S = LAYU_LD(SAMSIM_A_S_ABS, j); return u; };
  auto load4 = [&](int j) -> UL { UL u = load3(j); u.th = LAYU(SAMSIM_A_THICK, j); return u; };
  auto layers = [&](auto lite_tag) {
  if (regular_wave) {
    // Three layers per trip.  The three request buffers take the roles "this layer", "the next", "the one being requested" in
    // turn; with three textual copies of the layer in one trip the roles rotate by NAME and no buffer is ever copied into another.
    // (One layer per trip rotated them with `cur = nxt; nxt = nn;`, and those copies -- of rows requested at the top of the same
    // trip -- each waited for its row: the request lead was one layer body, with the wait at the end of it.)  The rows are the
    // wave's, not the lane's: every lane requests row k-2 at layer k whether or not the layer exists in its column (k > Na: it
    // only sits the layer out), so a shorter column finds its bottom layer in `a` when the wave arrives there, in whichever copy
    // that is.  The 0-2 layers a stretch has left over run one per trip and do copy their buffers (at most six per sweep).
    const int kc = kmax >= 2 ? kmax - 1 : 1;
    UL a = load3(kmax), b = load3(kc), d = b;       // layers k, k-1, k-2
    auto one = [&](const int k, const UL &row, UL &req, const double th_s, const double rth_s) {
      req = load3(k >= 3 ? k - 2 : 1);
      if (k <= Na) body(k, row, th_s, rth_s, std::false_type{}, lite_tag);
    };
    const int b0 = g.n_top, b1 = g.n_top + g.n_middle;
    int k = kmax;
    for (int stretch = 0; stretch < 3; ++stretch) {
      const int klo = stretch == 0 ? b1 + 1 : (stretch == 1 ? b0 + 1 : 2);
      // (formed where the stretch begins -- the elastic block's thickness is one load per sweep -- so that only this pair is carried)
      const double th_s = stretch == 1 ? LAYU(SAMSIM_A_THICK, g.n_top + 1) : g.thick_0, rth_s = recip(th_s);
      nc_s = newton_consts(s);
      for (; k - 2 >= klo; k -= 3) {
        ISA_MARK("U_ITER_BEGIN");
        ST_MARK(ST_UP);
        one(k, a, d, th_s, rth_s);
        ISA_MARK("U_LAYER_2");
        one(k - 1, b, a, th_s, rth_s);
        ISA_MARK("U_LAYER_3");
        one(k - 2, d, b, th_s, rth_s);
        ISA_MARK("U_ITER_END");
      }
      for (; k >= klo; --k) {
        ISA_MARK("U_REST_BEGIN");
        ST_MARK(ST_UP);
        one(k, a, d, th_s, rth_s);
        a = b; b = d;
        ISA_MARK("U_REST_END");
      }
    }
    cur = a;
  } else {
    cur = load4(Na); nxt = load4(Na >= 2 ? Na - 1 : 1); nn = nxt;
    for (int k = kmax; k >= 2; --k) {
      if (k > Na) continue;
      nn = load4(k >= 3 ? k - 2 : 1);
      body(k, cur, cur.th, recip(cur.th), std::false_type{}, lite_tag);
      cur = nxt; nxt = nn;
    }
  }
  };
  const bool lite = K::fixed && CFG(flush_flag) == 5 && wave_any((c.flags & COLF_FLUSHED) != 0);
  if (lite) { ST_COUNT(CT_LITE, 1); layers(std::true_type{}); } else layers(std::false_type{});
  __builtin_amdgcn_wave_barrier();   // the row flags are complete: the next readers are the down sweeps of the next step
  if (neg_salt || lite) c.flags |= COLF_DIRTY;
  body(1, cur, LAYU(SAMSIM_A_THICK, 1), 0.0, std::true_type{}, std::false_type{});
  if (!alive) return;
  // hand-over block for prologue_top_layer of the next step
  if (!lite) {
  SPEC(SP_MINP) = r.minp; SPEC(SP_STP) = r.stp; SPEC(SP_ST) = r.st;
  SPEC(SP_BOT) = r.bot; SPEC(SP_BOTTERM) = r.botterm; SPEC(SP_PERM_BOT) = r.perm_bot;
  SPEC(SP_SBR_BOT) = r.S_br_bot; SPEC(SP_BUOY_S) = r.buoy_s; SPEC(SP_MIN_PSI_S) = r.min_psi_s;
  }
  // energy conservation assert, mo_heat_fluxes.f90:265-310: (SUM(H_abs) + H_abs_snow) before + what went in - the same after,
  // with the two sums taken as one sum of per-layer differences
  double bal = esum + (H_abs_snow_before - CL(H_abs_snow));
  bal = bal + (double)Na * (c.frad * dt);
  if (thin_snow || CL(thick_snow) >= thick_min) bal = bal + c.fl_q_bottom * dt - CL(fl_Q_snow) * dt;
  else bal = bal + c.fl_q_bottom * dt - CL(fl_Q1) * dt;
  // (the reference evaluates the heat fluxes, mo_grotz.f90:584, before the second getT sweep, :598: a column that fails both reports 431)
  if (fabs(bal / dt) > 0.00001) STOPC(431, 0);
  if (rc) STOPC(rc, rc_layer);
}

}  // namespace

#endif
