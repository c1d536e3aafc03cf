// samsim_tracers.h -- advection of the passive tracers (bgc_flag 2) with the brine fluxes the sweeps of the step left in the flux block.
// Part of the translation unit samsim_kernels.hip: expects samsim_step_types.h (`c`, `x`; LAY, BGC, BGC_BOT, BFL) and samsim_thermo.h.
#ifndef SAMSIM_TRACERS_H
#define SAMSIM_TRACERS_H

namespace {

// ---------------------------------------------------------------- bgc_advection, mo_mass.f90:150-209
// The reference collects the step's brine fluxes in the (N+1)^2 matrix fl_brine_bgc and loops over all of it; at most
// four entries per row are ever set:   (i, i-1) fl_up(i-1)                    return flow of the gravity drainage
//                                      (i, i+1) -fl_m(i+1) + flush_v(i)       expulsion, vertical flushing
//                                      (i, N_active) flush_h(i)               horizontal flushing   [same entry for i = N_active-1]
//                                      (i, N_active+1) fl_down(i) [+ the expulsion part of (N_active-1, N_active), sic]
//                                      (N_active, 1) flood_brine,  (N_active+1, N_active) flood_brine + fl_up(N_active)
// Every flux is upwind (brine concentration of the source layer), limited to a third of the source's content.  One pass
// top -> bottom: what a layer gives to the layer above is added before that layer is stored (one layer of delay), what it
// gives to the layer below / to the bottom layer is carried along.
template <class K>
__device__ RARE void bgc_advection(Col &c, const Ctx &x) {
  const int Na = c.Na;
  for (int t = 0; t < x.n_bgc; ++t) {
    const double bottom = BGC_BOT(t);
    double carry_dn = 0.0, to_bottom = 0.0, to_top = 0.0, pend = 0.0;
    for (int i = 1; i <= Na; ++i) {
      const double q = BGC(t, i);
      const double br = q / dmax(LAY(SAMSIM_A_PSI_L, i) * LAY(SAMSIM_A_THICK, i) * rho_l, 0.000000000000001);
      const double lim = q / 3.0;
      const double E = BFL(BFL_E, i), V = BFL(BFL_V, i);
      double F_up = (i >= 2) ? BFL(BFL_U, i - 1) : 0.0;
      double F_dn = E + V, F_h = (i <= Na - 2) ? BFL(BFL_H, i) : 0.0, F_out = 0.0, F_top = 0.0;
      if (i == Na - 1) F_dn = F_dn + BFL(BFL_H, i);                       // (N_active-1, N_active) holds both
      if (i <= Na - 1) { if (c.bgc_grav) F_out = ((i == Na - 1) ? E : 0.0) + BFL(BFL_D, i); }
      else {                                                               // i = N_active: (i, i+1) leaves the domain
        double sh = 0.0;
        for (int k = 1; k <= Na - 1; ++k) sh += BFL(BFL_H, k);
        F_out = F_dn + sh; F_dn = 0.0;
        if (Na == 2) F_up = F_up + c.bgc_flood; else F_top = c.bgc_flood;  // (N_active, 1)
      }
      const double f_up = dmin(F_up * br, lim), f_dn = dmin(F_dn * br, lim), f_h = dmin(F_h * br, lim);
      const double f_out = dmin(F_out * br, lim), f_top = dmin(F_top * br, lim);
      double temp = q;
      if (i == Na && Na > 2) temp = temp - f_top;
      if (i >= 2) temp = temp - f_up;
      if (i < Na) temp = temp - f_dn;
      if (i <= Na - 2) temp = temp - f_h;
      temp = temp + carry_dn;                                              // from the layer above
      if (i == Na) {
        temp = temp + to_bottom;                                           // horizontal flushing of the layers above
        temp = temp - f_out;
        temp = temp + (c.bgc_flood + BFL(BFL_U, Na)) * bottom;            // (N_active+1, N_active): from the water below
      } else {
        temp = temp - f_out;
      }
      if (i >= 2) BGC(t, i - 1) = pend + f_up;                             // the layer above is complete now
      pend = temp;
      carry_dn = f_dn; to_bottom = to_bottom + f_h; to_top = f_top;
    }
    BGC(t, Na) = pend;
    if (Na > 2 && to_top != 0.0) BGC(t, 1) = BGC(t, 1) + to_top;
  }
  for (int r = 0; r < BFL_NROW; ++r)                                       // fl_brine_bgc = 0, mo_grotz.f90:745
    for (int k = 1; k <= Na; ++k) BFL(r, k) = 0.0;
}

}  // namespace

#endif
