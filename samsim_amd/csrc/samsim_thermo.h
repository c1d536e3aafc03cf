// samsim_thermo.h -- arithmetic helpers (dmax / dmin / fma_c / max_c, the reciprocals of samsim_div.h, the powers of samsim_pow.h) and
// the thermodynamic functions of one layer: liquidus polynomial, Newton step, getT and its wave form getT_chain, phi_from_T, and
// func_density / func_T_freeze / func_albedo / func_k_snow.  Part of the translation unit samsim_kernels.hip: expects
// samsim_step_types.h (constants, Salt, Ctx, wave_any) and the ISA_MARK of samsim_probe.h.
#ifndef SAMSIM_THERMO_H
#define SAMSIM_THERMO_H

namespace {

#include "samsim_div.h"
// MAX / MIN of the reference as one v_max_f64 / v_min_f64 each.  `a > b ? a : b` compiles to a compare and two 32-bit selects
// (the C semantics for NaN and signed zeros differ from the instruction's), and every vector instruction costs the same four
// cycles: the sweeps clamp some twenty times per layer-cell.  For ordered operands the value is the same (max(-0, +0) may come out
// as +0 instead of -0: equal numbers); a NaN operand loses against a number in both forms where the number is the constant.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double dmax(double a, double b) {
  double r;
  if (__builtin_constant_p(b) && b == 0.0) asm("v_max_f64 %0, %1, 0" : "=v"(r) : "v"(a));
  else asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double dmin(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
#else
__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double dmin(double a, double b) { return a < b ? a : b; }
#endif
// a*b + C and max(a, C) with the constant C read from a scalar register pair.  Left to itself the compiler picks the accumulating
// form (v_fmac) for a*b + constant and first copies the constant into the accumulator -- two v_mov_b32 per fused multiply-add, and a
// vector move costs the SIMD the same four cycles as the arithmetic it feeds.  (One scalar operand per instruction is what the
// encoding allows, so a step with two constants is a multiply and an add.)
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double fma_c(double a, double b, double c_const) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c_const));
  return r;
}
__device__ __forceinline__ double max_c(double a, double c_const) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(c_const));
  return r;
}
#else
__device__ __forceinline__ double fma_c(double a, double b, double c_const) { return __builtin_fma(a, b, c_const); }
__device__ __forceinline__ double max_c(double a, double c_const) { return a > c_const ? a : c_const; }
#endif
// S_bu = S_abs/m and H = H_abs/m of one layer, mo_grotz.f90:298-299, 593-594
__device__ __forceinline__ void per_mass(double S_abs, double H_abs, double m, double &S_bu, double &H) {
  const double rm = recip(m);
  S_bu = S_abs * rm;
  H = H_abs * rm;
}

// func_S_br without / with the S_bu clamp, mo_thermo_functions.f90:308-360.  flang lowers T**2._wp and T**3._wp
// to multiplications (verified bit for bit against the flang build), so do we.
__device__ __forceinline__ double S_br_poly(const Salt &s, double T) {
  return T * (s.c2 + T * (s.c3 + T * s.c4));
}
__device__ __forceinline__ double S_br_clamped(const Salt &s, double T, double S_bu) {
  double v = S_br_poly(s, T);
  return dmax(v, S_bu);   // one v_max_f64 for the compare and two 32-bit selects of `v < S_bu ? S_bu : v`: the same number for numbers
}
// func_ddT_S_br, mo_thermo_functions.f90:380-414 (derivative-only clamp below -20 C)
__device__ __forceinline__ double ddT_S_br(const Salt &s, double T) {
  const double T_crit = -20.0;
  double d = s.d2 + 2.0 * s.d3 * T + 3.0 * s.d4 * (T * T);
  if (T < T_crit) d = s.d2 + 2.0 * s.d3 * T_crit + 3.0 * s.d4 * (T_crit * T_crit);
  return d;
}

// residual f(T_0) and its derivative of the enthalpy relation, mo_thermo_functions.f90:95-96 / :109-110 (the first evaluation
// clamps S_br at 1e-9, the ones in the loop at 1e-10, as in the reference)
__device__ __forceinline__ void newton_terms(const Salt &s, double H, double S_bu, double T_0, double sb, double sb_floor,
                                             double &f, double &ddT_f) {
  if (sb > 0.0001) {  // neither clamp is active: one reciprocal serves both quotients
    const double inv = recip(sb);
    f = -latent_heat - H + latent_heat * S_bu * inv + c_s * T_0 + c_s_beta * T_0 * T_0 / 2.0;
    ddT_f = c_s + c_s_beta * T_0 - latent_heat * S_bu * ddT_S_br(s, T_0) * (inv * inv);
    return;
  }
  f = -latent_heat - H + latent_heat * S_bu / dmax(sb, sb_floor) + c_s * T_0 + c_s_beta * T_0 * T_0 / 2.0;
  ddT_f = c_s + c_s_beta * T_0 - latent_heat * S_bu * ddT_S_br(s, T_0) / dmax(sb * sb, 0.0000000001);
}

// One division per Newton step of getT instead of two: with f = N/sb**2 and f' = D/sb**2 (N = A*sb**2 + L*S_bu*sb, D = B*sb**2 -
// L*S_bu*S_br'(T), A and B the polynomial parts) the step is T_0 - N/D and the stopping rule |f| > 1 reads |N| > sb**2: the same
// iteration in exact arithmetic.  getT runs 3.6 evaluations per layer-cell on the bench ensemble, all of them on the critical path
// of the up sweep.
// One evaluation of the Newton step of getT from T_0 in the one-division form, with fused multiply-adds (one rounding per a*b+c
// instead of two; each iterate within an ulp or two of the reference's, like the shared reciprocals): T_new = T_0 - N/D, more =
// |N| > sb**2 (the reference's |f| > 1), ok = the liquidus salinity at T_0 is above 1e-4, i.e. the reference's clamps of S_br
// (1e-9 / 1e-10) are inactive and this form is the step.  A0 = -latent_heat - H and LS = latent_heat * S_bu are the caller's
// (the same for every evaluation of a layer).  Straight-line: no branch, 23 vector instructions.
// Three of its fused multiply-adds have a constant multiplier AND a constant addend (c3, c_s twice, 2*d3); the instruction takes one
// operand from a scalar register, so the compiler copies the other into a vector register pair first -- two v_mov_b32 per constant
// and evaluation, re-done inside getT's loop (no hoisting: Makefile).  NewtonConsts holds those three as vector values the caller
// forms once per layer.
struct NewtonConsts { double c3, cs, d3x2; };
__device__ __forceinline__ NewtonConsts newton_consts(const Salt &s) {
  NewtonConsts n = {s.c3, c_s, 2.0 * s.d3};
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(n.c3), "+v"(n.cs), "+v"(n.d3x2));   // (vector registers from here on: not rematerialised per use)
#endif
  return n;
}
__device__ __forceinline__ void newton_eval(const Salt &s, const NewtonConsts &n, double A0, double LS, double T_0, double &T_new, bool &more, bool &ok) {
  const double sbf = T_0 * fma_c(T_0, __builtin_fma(T_0, s.c4, n.c3), s.c2);      // (fma_c: the addend from a scalar register pair)
  const double sb2 = sbf * sbf;
  const double A = __builtin_fma(T_0, __builtin_fma(T_0, 0.5 * c_s_beta, n.cs), A0);
  const double B = __builtin_fma(c_s_beta, T_0, n.cs);
  const double num = __builtin_fma(A, sb2, LS * sbf);
  const double Tc = max_c(T_0, -20.0);                       // derivative-only clamp below -20 C, mo_thermo_functions.f90:408-412
  const double dd = fma_c(Tc, __builtin_fma(Tc, 3.0 * s.d4, n.d3x2), s.d2);
  const double den = __builtin_fma(B, sb2, -(LS * dd));
  T_new = T_0 - quot(num, den);
  more = fabs(num) > sb2;
  ok = sbf > 0.0001;
}

// one Newton step from T_0: returns the new iterate and whether |f(T_0)| > 1 (general routine: any S_br)
__device__ __forceinline__ bool newton_step(const Salt &s, double H, double S_bu, double T_0, double sb_floor, double &T_new) {
  {
    bool more, ok;
    double Tn;
    newton_eval(s, newton_consts(s), -latent_heat - H, latent_heat * S_bu, T_0, Tn, more, ok);
    if (ok) { T_new = Tn; return more; }
  }
  const double sb = S_br_poly(s, T_0);
  double f, ddT_f;
  newton_terms(s, H, S_bu, T_0, sb, sb_floor, f, ddT_f);
  T_new = T_0 - quot(f, ddT_f);
  return fabs(f) > 1.0;
}

// H/c_l: the temperature of pure brine of enthalpy H (first line of getT, mo_thermo_functions.f90:84)
__device__ __forceinline__ double T_liquid(double H) {
  return H * (1.0 / c_l);
}

// the temperature at which brine of salinity S_bu starts to freeze, mo_thermo_functions.f90:85-92 (Newton from -1 C)
__device__ __forceinline__ double T_freeze_of(const Salt &s, double S_bu) {
  double T_fr = -1.0;
  while (fabs(S_br_poly(s, T_fr) / S_bu - 1.0) > (double)0.0001f) {  // tolerance is a float32 literal (:87)
    const double t0 = T_fr;
    T_fr = t0 - (S_br_poly(s, t0) - S_bu) / ddT_S_br(s, t0);
  }
  return T_fr;
}

// getT, mo_thermo_functions.f90:62-143: guarded Newton iteration for T and the solid mass fraction phi.
// Returns 99 (the reference's STOP code) when 260 iterations do not converge.
__device__ __forceinline__ int getT(const Salt &s, double H, double S_bu, double T_in, double &T_out, double &phi_out, int *evals = nullptr) {
  double T = T_liquid(H), phi = phi_out;
  int rc = 0;
  if (S_br_clamped(s, T, S_bu) > S_bu && S_bu > 0.001) {
    double T_fr = 0.0, T_0;
    bool have_T_fr = false;
    T_0 = T_in;
    bool more = newton_step(s, H, S_bu, T_0, 0.000000001, T);
    int i = 0;
    while (more) {
      T_0 = T;
      if (T_0 > 0.0 || T_0 < -200.0) {
        // The reference computes the freezing temperature T_fr up front (mo_thermo_functions.f90:85-92) and only reads it
        // here.  It has no other effect, so it is evaluated on first use: same value, no Newton loop in the common case.
        if (!have_T_fr) {
          T_fr = T_freeze_of(s, S_bu);
          have_T_fr = true;
        }
        T_0 = T_fr;
      }
      more = newton_step(s, H, S_bu, T_0, 0.0000000001, T);
#if SAMSIM_STAMPS == 2
      if (evals) *evals += 1;
#endif
      if (++i == 260) { rc = 99; break; }
    }
    phi = 1.0 - quot(S_bu, S_br_clamped(s, T, S_bu));
  } else if (S_bu < 0.001) {
    if (H > 0.0) { phi = 0.0; T = H / c_l; }
    else if (H <= -latent_heat) { phi = 1.0; T = (H + latent_heat) / c_s; }
    else if (H <= 0.0 && -latent_heat < H) { T = 0.0; phi = -H / latent_heat; }
  } else {
    phi = 0.0;
  }
  T_out = T;
  phi_out = phi;
  return rc;
}

// getT for the layers of a sweep (the up sweeps, the full first sweep): the same iteration, arranged for a wave.  Winter columns
// are mushy layers whose iterates stay inside (-200, 0) and whose liquidus salinity stays above 1e-4: for them getT is a first
// evaluation and a loop of further ones, and every lane of the wave runs that loop together -- `while (some lane wants more)`, the
// update selected per lane -- so that the loop is straight-line vector code under ONE scalar branch, without the exec-mask
// bookkeeping of a per-lane `while` (a wave runs as many trips as its slowest lane either way: 3.57 against a lane mean of 3.33
// in winter, 7.1 against 4.4 in the melt season).  A lane that is anything else -- fresh ice, pure brine, an iterate that leaves
// the interval and needs T_fr, S_br under 1e-4, no convergence -- is redone by the general routine above, on its own: what a lane
// gets depends on its own column only, and the arithmetic (newton_eval) is the general routine's.
// WARM (the sweeps of a melt season: the full first sweep, the up sweep of a flushing wave): an iterate that leaves (-200, 0) is
// replaced by the freezing temperature inside the loop, exactly where the general routine does it, instead of sending the lane
// through the general routine afterwards -- near 0 C a third of the layers of a wave hold such a lane, and each cost the wave a
// second, slower iteration from the start.  The winter sweeps keep the loop without it (three registers less in their layer loop).
// S_br_out (the fused up sweep's full layers): the clamped liquidus salinity at the temperature returned, which the first sweep of the
// next step needs as well, is formed ONCE, after the redo, and handed out: a lane that was not redone keeps the loop's temperature, so
// its phi comes from the same operands as before, and the polynomial is not evaluated a second time behind the redo.
// The pure-brine test `above` (the liquidus salinity at H/c_l exceeds S_bu) holds for every layer that has ice in it, and only its
// wave-level vote is used.  Both liquidus cubics fall strictly with T (the derivative has no real root: 1.038**2 < 4*0.01605*18.7,
// 0.778**2 < 4*0.01086*17.6) and are 51.6 and 49.4 at -3 C: where every active lane has H/c_l < -3 and S_bu < 40 the test holds in
// all of them -- nine units of margin against a rounding error of 1e-14 -- and the cubic is not evaluated.  A NaN fails either
// compare and takes the evaluation.
// nc_in: NewtonConsts the caller formed (the fused up sweep: once per stretch of layers instead of once per layer).
template <bool WARM = false>
__device__ __forceinline__ int getT_chain(const Salt &s, double H, double S_bu, double T_in, double &T_out, double &phi_out, int *evals = nullptr,
                                          double *S_br_out = nullptr, const NewtonConsts *nc_in = nullptr) {
  const double Tl = T_liquid(H);
  const bool salty = S_bu > 0.001;   // mushy = above && salty
  const double A0 = -latent_heat - H, LS = latent_heat * S_bu;
  const NewtonConsts nc = nc_in ? *nc_in : newton_consts(s);
  const bool short_cut = (__builtin_amdgcn_ballot_w64(!(Tl < -3.0)) | __builtin_amdgcn_ballot_w64(!(S_bu < 40.0))) == 0ull;
  unsigned long long brine_m = 0ull;   // ballot(!above)
  if (!short_cut) brine_m = __builtin_amdgcn_ballot_w64(!(S_br_clamped(s, Tl, S_bu) > S_bu));
#if SAMSIM_STAMPS == 2
  if (short_cut && evals) *evals = (int)((unsigned)*evals | 0x80000000u);   // (decoded by the caller: CT_ABOVE_FAST)
#endif
  double T;
  bool more0, ok;
  newton_eval(s, nc, A0, LS, T_in, T, more0, ok);
  // `more` and `odd` travel through the loop as 64-bit lane masks in scalar register pairs, one bit per lane: their bookkeeping
  // (and / or / andn2, the loop test `more_m == 0`) issues on the scalar unit beside the vector work of the evaluation, and the
  // select of T reads the pair as its mask directly; every vector instruction costs the SIMD four cycles, a 0 / 1 word per lane
  // cost six per trip.  Two things this rests on, both true of every caller:
  //  * partial exec -- a ballot only sees active lanes, and getT_chain runs under partial exec everywhere (`if (k <= Na)` in the up
  //    sweep, the last wave of a handle whose column count is no multiple of 64, prologue_top_layer, the full first sweep): an
  //    inactive lane's bit is 0 in every mask, so it neither keeps the loop alive nor is marked odd;
  //  * uniform control flow -- every call site reaches the loop in wave-uniform control flow (the masks are the wave's, the branch
  //    on `more_m == 0` is scalar), as the `ballot == 0` break of the 0 / 1-word form already required.
  // odd_m = ballot(!mushy || !ok), as the ballot of each compare, OR-ed on the scalar side (the ballot of an OR of compares is formed
  // through a 0 / 1 word in a vector register: a v_cndmask and a v_cmp more)
  unsigned long long odd_m = brine_m | __builtin_amdgcn_ballot_w64(!salty) | __builtin_amdgcn_ballot_w64(!ok);
  unsigned long long more_m = __builtin_amdgcn_ballot_w64(more0) & ~odd_m;
  int i = 0;
  double T_fr = 0.0;
  bool have_T_fr = false;
  ISA_MARK("NEWTON_LOOP");
  for (;;) {
    if (more_m == 0ull) break;
    const bool more = __builtin_amdgcn_inverse_ballot_w64(more_m);
    if (WARM) {
      // (wave_any(more && (T > 0 || T < -200)), the ballots combined on the scalar side like left_m below)
      const unsigned long long out_m = more_m & (__builtin_amdgcn_ballot_w64(T > 0.0) | __builtin_amdgcn_ballot_w64(T < -200.0));
      if (out_m != 0ull) {
        if (__builtin_amdgcn_inverse_ballot_w64(out_m)) {
          if (!have_T_fr) { T_fr = T_freeze_of(s, S_bu); have_T_fr = true; }
          T = T_fr;
        }
      }
    }
    double Tn;
    bool m2, ok2;
    newton_eval(s, nc, A0, LS, T, Tn, m2, ok2);
    // (the test is on the iterate the evaluation started from; the ballot of each compare, OR-ed on the scalar side: the ballot of
    // their OR goes through a 0 / 1 word in a vector register)
    unsigned long long left_m = __builtin_amdgcn_ballot_w64(!ok2);
    if (!WARM) left_m |= __builtin_amdgcn_ballot_w64(T > 0.0) | __builtin_amdgcn_ballot_w64(T < -200.0);
    const unsigned long long m2_m = __builtin_amdgcn_ballot_w64(m2);
#if SAMSIM_STAMPS == 2
    if (evals && more) *evals += 1;
#endif
    T = more ? Tn : T;
    odd_m |= left_m & more_m;
    more_m &= m2_m & ~left_m;
    if (++i == 260) { odd_m |= more_m; break; }       // no convergence in 260 evaluations: the general routine reports it (STOP 99)
  }
  const bool odd = __builtin_amdgcn_inverse_ballot_w64(odd_m);
  ISA_MARK("NEWTON_LOOP_END");
  double phi = S_br_out ? 0.0 : 1.0 - quot(S_bu, S_br_clamped(s, T, S_bu));
  int rc = 0;
  if (odd) {
    phi = phi_out;
#if SAMSIM_STAMPS == 2
    int ev0 = evals ? *evals : 0;
#endif
    rc = getT(s, H, S_bu, T_in, T, phi, evals);
#if SAMSIM_STAMPS == 2
    if (evals) *evals += ((*evals - ev0) << 16) | (1 << 30);   // (decoded by the caller: redone by the general routine, its evaluations)
#endif
  }
  if (S_br_out) {
    const double S_br_T = S_br_clamped(s, T, S_bu);
    if (!odd) phi = 1.0 - quot(S_bu, S_br_T);
    *S_br_out = S_br_T;
  }
  T_out = T;
  phi_out = phi;
  return rc;
}

// The solid fraction getT returned for a layer, recomputed from the temperature it returned and the values it was called
// with (mo_thermo_functions.f90:84,129,131-143): same operands, same operations, so the same phi bit for bit.  The down sweeps
// use it instead of loading phi (one array less to hand over).
__device__ __forceinline__ double phi_from_T(const Salt &s, double H, double S_bu, double S_br_T) {
  // S_bu > 0.001 is a mushy layer or pure brine.  getT gives pure brine phi = 0 and T = H/c_l, whose clamped liquidus salinity
  // S_br_T is S_bu itself -- and quot(x, x) is exactly 1 (samsim_div.h: the residual correction removes what the rounded
  // product x*r is off by) -- so the mushy layer's formula serves both and the liquidus need not be evaluated at H/c_l again.
  if (S_bu > 0.001) return 1.0 - quot(S_bu, S_br_T);
  if (S_bu < 0.001) {
    if (H > 0.0) return 0.0;
    if (H <= -latent_heat) return 1.0;
    return -H / latent_heat;
  }
  return 0.0;
}

// x**3.10 of the permeability law (mo_grav_drain.f90:105, mo_flush.f90:119,128, mo_flood.f90:73) as exp(3.1*log(x)):
// within ~4e-15 relative of the correctly rounded pow() the reference links (|3.1*log x| <= 22 for x <= 1000), at a
// third of its instructions and without the double-double constant tables that push the layer loops into spills.
}  // namespace
#define SP_QUOT(a, b) quot(a, b)
#include "samsim_pow.h"
namespace {
// x*x*x * exp(0.1*log(x)) with a plain logarithm: within ~4 ulp of the correctly rounded power (samsim_pow.h)
__device__ __forceinline__ double pow_3p1(double x) { return sp_pow_3p1(x); }

__device__ __forceinline__ double pow_1p5(double x) { return sp_pow_1p5(x); }   // samsim_pow.h
__device__ __forceinline__ double pow_4(double x) { return sp_pow_4(x); }

// func_density, mo_functions.f90:51-62
__device__ double func_density(double T, double S) {
  double density_0 = 999.842594 + 6.8 / 100.0 * T;
  return density_0 + 0.825 * S + (-5.7 / 1000.0) * pow_1p5(dmax(S, 0.0));
}

// func_T_freeze, mo_functions.f90:239-250 (float32 products of default-REAL literals)
__device__ double func_T_freeze(double S_bu, int salt_flag, double tf_c3) {
  if (salt_flag == 2) {
    return -0.0592 * S_bu - (double)9.37f * (S_bu * S_bu) - tf_c3 * (S_bu * S_bu * S_bu);
  } else {
    const float a = 1.710523f * 1e-3f, b = 2.154996f * 1e-4f;
    return -0.0575 * S_bu + (double)a * pow_1p5(S_bu) - (double)b * (S_bu * S_bu);
  }
}

// func_albedo, mo_functions.f90:157-208 (float32 literals)
__device__ double func_albedo(double thick_snow, double T_snow, double psi_l, double thick_min, int albedo_flag) {
  const double ice_dry = (double)0.75f, ice_wet = (double)0.6f, snow_dry = (double)0.85f, snow_wet = (double)0.75f,
               water = (double)0.2f;
  double albedo;
  if (thick_snow > thick_min) {
    albedo = (T_snow < (double)(-0.01f)) ? snow_dry : snow_wet;
    albedo = ice_dry + (albedo - ice_dry) * dmin(1.0, quot(thick_snow, 0.3));
  } else {
    if (psi_l > 0.9) albedo = water;
    else if (psi_l > 0.6) albedo = ice_wet + (water - ice_wet) * ((psi_l - 0.6) / 0.3);
    else if (psi_l > 0.2) albedo = ice_wet;
    else albedo = ice_dry;
  }
  if (albedo_flag == 1) {
    if (thick_snow > thick_min) albedo = (T_snow < (double)(-0.01f)) ? snow_dry : snow_wet;
    else albedo = (psi_l < (double)0.8f) ? ice_dry : water;
  }
  return albedo;
}

// func_k_snow, mo_snow.f90:560-573
__device__ double func_k_snow(double m_snow, double thick_snow) {
  const double c0 = 0.138, c1 = -1.01 / 1000.0, c2 = 3.233 / 1000000.0;
  double r = quot(m_snow, thick_snow);
  double k_snow = c0 + quot(c1 * m_snow, thick_snow) + c2 * (r * r);
  return k_snow + (double)0.15f;
}

// 3-hourly table time axis, mo_functions.f90:323-325
__device__ __forceinline__ double time_input(int k) { return ((double)(float)k - 1.0) * 3600.0 * 3.0; }

// density of the water below the ice (sub_turb_flux, mo_functions.f90:355): the same number in every step of every column unless
// the tank budget (tank_flag 2) moves S_bu_bottom
template <class K>
__device__ __forceinline__ double ocean_density(const Ctx &x) {
  if ((K::fixed ? K::tank_flag : x.p->cfg.tank_flag) == 2 || (K::sites && x.ocean_sbu)) return func_density(x.p->cfg.T_bottom, x.S_bu_bottom);
  return x.rho_bottom;
}

}  // namespace

#endif
