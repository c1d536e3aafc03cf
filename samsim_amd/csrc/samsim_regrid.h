// samsim_regrid.h -- the semi-adaptive grid: top_melt, top_grow, bottom_melt, bottom_growth and their driver layer_dynamics, each also
// replayed per passive tracer.  Part of the translation unit samsim_kernels.hip: expects samsim_step_types.h (`c`, `x`, `g`; CL, GS,
// LAY, BGC*, CFG, STOPC) and samsim_thermo.h.
#ifndef SAMSIM_REGRID_H
#define SAMSIM_REGRID_H

namespace {

// ---------------------------------------------------------------- layer_dynamics, mo_layer_dynamics.f90:64-716
// Regridding with tracers.  In the reference every statement of the regrid routines on S_abs / S_bu / S_bu_bottom has a twin
// on bgc_temp / bgc_bulk / bgc_bottom (mo_layer_dynamics.f90:205-373).  Each routine below therefore takes `tr`: tr < 0 is
// the routine proper; tr >= 0 replays it for tracer tr -- same control flow, the tracer standing in for S_abs, and nothing
// else written (m, H_abs, thick, N_active stay as they are, so every replay and then the proper pass see the old profile).
template <class K>
__device__ __forceinline__ gdouble &salt_at(Col &c, const Ctx &x, int tr, int k) {
  if (K::bgc && tr >= 0) return BGC(tr, k);
  return LAY(SAMSIM_A_S_ABS, k);
}
template <class K>
__device__ __forceinline__ double salt_below(Col &c, const Ctx &x, int tr) {
  if (K::bgc && tr >= 0) return BGC_BOT(tr);
  return x.S_bu_bottom;
}
struct LayerVals { double rho, S_bu, H; };
template <class K>
__device__ __forceinline__ LayerVals layer_vals(Col &c, const Ctx &x, int tr, int k) {
  const double m = LAY(SAMSIM_A_M, k);
  LayerVals v;
  v.rho = m / LAY(SAMSIM_A_THICK, k);
  v.S_bu = salt_at<K>(c, x, tr, k) / m;
  v.H = LAY(SAMSIM_A_H_ABS, k) / m;
  return v;
}
template <class K>
__device__ __forceinline__ void set_layer(Col &c, const Ctx &x, int tr, int k, const LayerVals &v, double thick_0) {
  if (tr < 0) LAY(SAMSIM_A_M, k) = v.rho * thick_0;
  salt_at<K>(c, x, tr, k) = v.S_bu * v.rho * thick_0;
  if (tr < 0) LAY(SAMSIM_A_H_ABS, k) = v.H * v.rho * thick_0;
}
template <class K>
__device__ __forceinline__ void zero_layer(Col &c, const Ctx &x, int tr, int k) {
  salt_at<K>(c, x, tr, k) = 0.0;
  if (tr < 0) { LAY(SAMSIM_A_M, k) = 0.0; LAY(SAMSIM_A_H_ABS, k) = 0.0; LAY(SAMSIM_A_THICK, k) = 0.0; }
}

// top_melt, mo_layer_dynamics.f90:191-327
template <class K>
__device__ __forceinline__ void top_melt(Col &c, const Ctx &x, int tr) {
  const samsim_config &g = x.p->cfg;
  const int N = c.N, N_top = g.n_top, N_middle = g.n_middle;
  const double thick_0 = g.thick_0;
  int Na = c.Na;
  // layer 1 absorbs layer 2
  salt_at<K>(c, x, tr, 1) = salt_at<K>(c, x, tr, 1) + salt_at<K>(c, x, tr, 2);
  if (tr < 0) {
    LAY(SAMSIM_A_M, 1) = LAY(SAMSIM_A_M, 1) + LAY(SAMSIM_A_M, 2);
    LAY(SAMSIM_A_H_ABS, 1) = LAY(SAMSIM_A_H_ABS, 1) + LAY(SAMSIM_A_H_ABS, 2);
    LAY(SAMSIM_A_THICK, 1) = LAY(SAMSIM_A_THICK, 1) + LAY(SAMSIM_A_THICK, 2);
  }
  // the layer values that later branches need from the OLD profile
  const bool have_mid = (Na == N);
  LayerVals old_top1 = {0, 0, 0};
  if (have_mid) old_top1 = layer_vals<K>(c, x, tr, N_top + 1);
  const int kend = (N_top - 1 < Na - 1) ? N_top - 1 : Na - 1;
  for (int k = 2; k <= kend; ++k) set_layer<K>(c, x, tr, k, layer_vals<K>(c, x, tr, k + 1), thick_0);  // reads old k+1 (not yet modified)
  if (Na <= N_top) {
    zero_layer<K>(c, x, tr, Na);
    Na = Na - 1;
  } else if (Na > N_top && Na <= N && LAY(SAMSIM_A_THICK, N_top + 1) / thick_0 < 1.00001) {
    for (int k = N_top; k <= Na - 1; ++k) set_layer<K>(c, x, tr, k, layer_vals<K>(c, x, tr, k + 1), thick_0);
    zero_layer<K>(c, x, tr, Na);
    Na = Na - 1;
  }
  if (Na == N && LAY(SAMSIM_A_THICK, N_top + 1) - thick_0 >= 0.000001) {
    double loss_m = thick_0 * old_top1.rho, loss_S = loss_m * old_top1.S_bu, loss_H = loss_m * old_top1.H;
    salt_at<K>(c, x, tr, N_top) = loss_S;
    if (tr < 0) { LAY(SAMSIM_A_M, N_top) = loss_m; LAY(SAMSIM_A_H_ABS, N_top) = loss_H; }
    for (int k = N_top + 1; k <= N_middle + N_top; ++k) {
      const LayerVals below = layer_vals<K>(c, x, tr, k + 1);  // old values of k+1
      double m = LAY(SAMSIM_A_M, k), H_abs = LAY(SAMSIM_A_H_ABS, k), S_abs = salt_at<K>(c, x, tr, k);
      m = m - loss_m; H_abs = H_abs - loss_H; S_abs = S_abs - loss_S;
      const double shift = thick_0 * (double)(float)(N_middle - k + N_top) / (double)(float)(N_middle);
      loss_m = shift * below.rho; loss_S = loss_m * below.S_bu; loss_H = loss_m * below.H;
      m = m + loss_m; H_abs = H_abs + loss_H; S_abs = S_abs + loss_S;
      salt_at<K>(c, x, tr, k) = S_abs;
      if (tr < 0) { LAY(SAMSIM_A_M, k) = m; LAY(SAMSIM_A_H_ABS, k) = H_abs; }
    }
    if (tr < 0)
      for (int k = N_top + 1; k <= N_top + N_middle; ++k) LAY(SAMSIM_A_THICK, k) = LAY(SAMSIM_A_THICK, k) - thick_0 / (double)(float)(N_middle);
  }
  if (tr >= 0) return;
  c.Na = Na;
  double sth = 0.0;
  for (int k = 1; k <= N; ++k) sth += LAY(SAMSIM_A_THICK, k);
  if (thick_0 * (Na + 0.501) <= sth && Na < N) STOPC(7889, 0);
}

// top_grow, mo_layer_dynamics.f90:607-716
template <class K>
__device__ __forceinline__ void top_grow(Col &c, const Ctx &x, int tr) {
  const samsim_config &g = x.p->cfg;
  const int N = c.N, N_top = g.n_top, N_middle = g.n_middle;
  const double thick_0 = g.thick_0;
  int Na = c.Na;
  LayerVals carry = layer_vals<K>(c, x, tr, 1);  // old values of layer k-1
  {
    const double loss_m = thick_0 * carry.rho, loss_S = loss_m * carry.S_bu, loss_H = loss_m * carry.H;
    salt_at<K>(c, x, tr, 1) = salt_at<K>(c, x, tr, 1) - loss_S;
    if (tr < 0) {
      LAY(SAMSIM_A_M, 1) = LAY(SAMSIM_A_M, 1) - loss_m;
      LAY(SAMSIM_A_H_ABS, 1) = LAY(SAMSIM_A_H_ABS, 1) - loss_H;
      LAY(SAMSIM_A_THICK, 1) = LAY(SAMSIM_A_THICK, 1) - thick_0;
    }
  }
  int kend = (N_top < Na) ? N_top : Na;
  if (Na > N_top && Na < N) kend = Na;  // second branch continues the same shift over N_top+1..Na
  for (int k = 2; k <= kend; ++k) {
    const LayerVals old_k = layer_vals<K>(c, x, tr, k);
    set_layer<K>(c, x, tr, k, carry, thick_0);
    carry = old_k;
  }
  if (Na <= N_top || (Na > N_top && Na < N)) {
    Na = Na + 1;
    set_layer<K>(c, x, tr, Na, carry, thick_0);  // S_bu*thick_0*rho and S_bu*rho*thick_0 differ in association:
    salt_at<K>(c, x, tr, Na) = carry.S_bu * thick_0 * carry.rho;  // mo_layer_dynamics.f90:660-661,674-675
    if (tr < 0) { LAY(SAMSIM_A_H_ABS, Na) = carry.H * thick_0 * carry.rho; LAY(SAMSIM_A_THICK, Na) = thick_0; }
  } else if (Na == N) {
    // carry holds the old values of layer N_top
    double loss_m = thick_0 * carry.rho, loss_S = loss_m * carry.S_bu, loss_H = loss_m * carry.H;
    for (int k = N_top + 1; k <= N_middle + N_top; ++k) {
      const LayerVals own = layer_vals<K>(c, x, tr, k);  // old values of k
      double m = LAY(SAMSIM_A_M, k), H_abs = LAY(SAMSIM_A_H_ABS, k), S_abs = salt_at<K>(c, x, tr, k);
      m = m + loss_m; H_abs = H_abs + loss_H; S_abs = S_abs + loss_S;
      const double shift = thick_0 * (double)(float)(N_middle - k + N_top) / (double)(float)(N_middle);
      loss_m = shift * own.rho; loss_S = loss_m * own.S_bu; loss_H = loss_m * own.H;
      m = m - loss_m; H_abs = H_abs - loss_H; S_abs = S_abs - loss_S;
      salt_at<K>(c, x, tr, k) = S_abs;
      if (tr < 0) { LAY(SAMSIM_A_M, k) = m; LAY(SAMSIM_A_H_ABS, k) = H_abs; }
    }
    if (tr < 0)
      for (int k = N_top + 1; k <= N_top + N_middle; ++k) LAY(SAMSIM_A_THICK, k) = LAY(SAMSIM_A_THICK, k) + thick_0 / (double)(float)(N_middle);
  }
  if (tr < 0) c.Na = Na;
}

// bottom_melt, mo_layer_dynamics.f90:341-427 (N_active == Nlayer)
template <class K>
__device__ __forceinline__ void bottom_melt(Col &c, const Ctx &x, int tr) {
  const samsim_config &g = x.p->cfg;
  const int N = c.N, N_top = g.n_top, N_middle = g.n_middle;
  const double thN = LAY(SAMSIM_A_THICK, N);
  double loss_m = 0.0, loss_S = 0.0, loss_H = 0.0;
  LayerVals carry = {0, 0, 0};
  for (int k = N_top + 1; k <= N_top + N_middle; ++k) {
    const LayerVals own = layer_vals<K>(c, x, tr, k);
    double m = LAY(SAMSIM_A_M, k), H_abs = LAY(SAMSIM_A_H_ABS, k), S_abs = salt_at<K>(c, x, tr, k);
    m = m + loss_m; H_abs = H_abs + loss_H; S_abs = S_abs + loss_S;
    const double shift = thN * (k - N_top) / (double)(float)(N_middle);
    loss_m = shift * own.rho; loss_H = loss_m * own.H; loss_S = loss_m * own.S_bu;
    m = m - loss_m; H_abs = H_abs - loss_H; S_abs = S_abs - loss_S;
    salt_at<K>(c, x, tr, k) = S_abs;
      if (tr < 0) { LAY(SAMSIM_A_M, k) = m; LAY(SAMSIM_A_H_ABS, k) = H_abs; }
    if (tr < 0) LAY(SAMSIM_A_THICK, k) = LAY(SAMSIM_A_THICK, k) - thN / (double)(float)(N_middle);
    carry = own;
  }
  for (int k = N_top + N_middle + 1; k <= N; ++k) {
    const LayerVals own = layer_vals<K>(c, x, tr, k);
    const double thick = LAY(SAMSIM_A_THICK, k);
    salt_at<K>(c, x, tr, k) = carry.rho * thick * carry.S_bu;
    if (tr < 0) { LAY(SAMSIM_A_H_ABS, k) = carry.rho * thick * carry.H; LAY(SAMSIM_A_M, k) = carry.rho * thick; }
    carry = own;
  }
}

// bottom_growth, mo_layer_dynamics.f90:438-523 (N_active == Nlayer)
template <class K>
__device__ __forceinline__ void bottom_growth(Col &c, const Ctx &x, int tr) {
  const samsim_config &g = x.p->cfg;
  const int N = c.N, N_top = g.n_top, N_middle = g.n_middle, N_bottom = g.n_bottom;
  const double thN = LAY(SAMSIM_A_THICK, N);
  double gain_m = 0.0, gain_S = 0.0, gain_H = 0.0;
  for (int k = N_top + 1; k <= N_top + N_middle; ++k) {
    const LayerVals below = layer_vals<K>(c, x, tr, k + 1);
    double m = LAY(SAMSIM_A_M, k), H_abs = LAY(SAMSIM_A_H_ABS, k), S_abs = salt_at<K>(c, x, tr, k);
    m = m - gain_m; H_abs = H_abs - gain_H; S_abs = S_abs - gain_S;
    const double shift = thN * (k - N_top) / (double)(float)(N_middle);
    gain_m = shift * below.rho; gain_H = gain_m * below.H; gain_S = gain_m * below.S_bu;
    m = m + gain_m; H_abs = H_abs + gain_H; S_abs = S_abs + gain_S;
    salt_at<K>(c, x, tr, k) = S_abs;
      if (tr < 0) { LAY(SAMSIM_A_M, k) = m; LAY(SAMSIM_A_H_ABS, k) = H_abs; }
  }
  if (tr < 0)
    for (int k = N_top + 1; k <= N_top + N_middle; ++k) LAY(SAMSIM_A_THICK, k) = LAY(SAMSIM_A_THICK, k) + thN / (double)(float)(N_middle);
  for (int k = N - N_bottom + 1; k <= N - 1; ++k) {
    salt_at<K>(c, x, tr, k) = salt_at<K>(c, x, tr, k + 1);
    if (tr < 0) { LAY(SAMSIM_A_H_ABS, k) = LAY(SAMSIM_A_H_ABS, k + 1); LAY(SAMSIM_A_M, k) = LAY(SAMSIM_A_M, k + 1); }
  }
  const double mN = thN * rho_l;
  salt_at<K>(c, x, tr, N) = mN * salt_below<K>(c, x, tr);
  if (tr < 0) { LAY(SAMSIM_A_M, N) = mN; LAY(SAMSIM_A_H_ABS, N) = mN * g.T_bottom * c_l; }
}

// layer_dynamics, mo_layer_dynamics.f90:64-175: exactly one branch per call, in priority order
template <class K>
__device__ RARE void layer_dynamics(Col &c, const Ctx &x) {
  const samsim_config &g = x.p->cfg;
  const int N = c.N, Na = c.Na, N_top = g.n_top, bf = CFG(bottom_flag);
  const double thick_0 = g.thick_0;
  const int km1 = (Na - 1 > 1) ? Na - 1 : 1;
  const double phi_Na = LAY(SAMSIM_A_PHI, Na), phi_km1 = LAY(SAMSIM_A_PHI, km1);
  const double phi_Nm1 = LAY(SAMSIM_A_PHI, N - 1), phi_N = LAY(SAMSIM_A_PHI, N);
  const double th_mid = LAY(SAMSIM_A_THICK, N_top + 1), th1 = LAY(SAMSIM_A_THICK, 1);
  const int nt = HAS_BGC ? x.n_bgc : 0;   // tracer replays (tr = nt-1 .. 0) come first, the routine proper (tr = -1) last
  if (phi_Nm1 <= psi_s_min / 2.0 && phi_Na < 0.00001 && Na == N && th_mid / thick_0 > 1.000001 && bf == 1) {
    for (int tr = nt - 1; tr >= -1; --tr) bottom_melt<K>(c, x, tr);
  } else if (Na > 1 && Na < N && phi_Na < 0.00001 && phi_km1 <= psi_s_min / 2.0 && bf == 1) {
    for (int tr = nt - 1; tr >= -1; --tr) zero_layer<K>(c, x, tr, Na);  // bottom_melt_simple, :573-591
    c.Na = Na - 1;
  } else if (Na > 1 && phi_Na < 0.00001 && phi_km1 <= psi_s_min / 2.0 && (th_mid / thick_0) < 1.01 && bf == 1) {
    for (int tr = nt - 1; tr >= -1; --tr) zero_layer<K>(c, x, tr, Na);
    c.Na = Na - 1;
  } else if (phi_Na > psi_s_min && Na < N && bf == 1) {
    // bottom_growth_simple, :537-560
    const double mnew = thick_0 * rho_l;
    c.Na = Na + 1;
    LAY(SAMSIM_A_THICK, Na + 1) = thick_0;
    LAY(SAMSIM_A_M, Na + 1) = mnew;
    LAY(SAMSIM_A_H_ABS, Na + 1) = mnew * g.T_bottom * c_l;
    for (int tr = nt - 1; tr >= -1; --tr) salt_at<K>(c, x, tr, Na + 1) = mnew * salt_below<K>(c, x, tr);
  } else if (phi_N > psi_s_min && bf == 1) {
    for (int tr = nt - 1; tr >= -1; --tr) bottom_growth<K>(c, x, tr);
  } else if (th1 > 1.5 * thick_0) {
    GS(MELT_OUT3) = GS(MELT_OUT3) - th1;
    for (int tr = nt - 1; tr >= -1; --tr) top_grow<K>(c, x, tr);
    GS(MELT_OUT3) = GS(MELT_OUT3) + LAY(SAMSIM_A_THICK, 1);
  } else if (th1 < 0.5 * thick_0) {
    GS(MELT_OUT3) = GS(MELT_OUT3) - th1;
    for (int tr = nt - 1; tr >= -1; --tr) top_melt<K>(c, x, tr);
    if (c.status) return;
    GS(MELT_OUT3) = GS(MELT_OUT3) + LAY(SAMSIM_A_THICK, 1);
  }
}

}  // namespace

#endif
