// Perfusion response and Arrhenius damage of the bioheat model (fus_thermal_set_response, fus_thermal_set_damage; fusmi.h
// "bioheat", perfusion response and damage): the parameter structs that travel by value in the arguments of
// k_thermal_response (thermal_kernels.hpp), and the checks of the caller's arguments.  Plain C++: no HIP header is needed, a
// host program may include this file (tests/cpp/thermal_response_driver.cpp).
//
//   P(T)    1 without knots; factor[0] for T <= temp[0], factor[n-1] for T >= temp[n-1]; between them, with j the largest
//           index with temp[j] <= T:  factor[j] + (factor[j+1] - factor[j]) * ((T - temp[j]) / (temp[j+1] - temp[j]))
//   S(D)    1 if dose_hi <= 0; else 1 for D <= dose_lo, 0 for D >= dose_hi, (dose_hi - D) / (dose_hi - dose_lo) between
//   r(T)    exp(lnA - Ea / (R (T + 273.15))),  R = 8.314462618 J/mol/K,  lnA = log(A) taken once here
// A check that fails leaves *out untouched.
#ifndef FUS_THERMAL_RESPONSE_HPP
#define FUS_THERMAL_RESPONSE_HPP

#include <cmath>

// the three laws below serve the kernel and the host alike; every operation is rounded by itself on both
#ifdef __HIPCC__
#define FUS_RESPONSE_FN __host__ __device__ inline
#else
#define FUS_RESPONSE_FN inline
#endif
#ifdef __clang__
#define FUS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FUS_NO_CONTRACT
#endif

namespace fus
{
constexpr int THERMAL_MAX_KNOTS = 8;
constexpr double GAS_CONSTANT = 8.314462618;

enum ThermalResponseError
{
  TRS_OK = 0,
  TRS_NKNOTS = 1,      // nknots outside 0..8, or knots without both arrays
  TRS_TEMP = 2,        // temp not finite or not strictly ascending
  TRS_FACTOR = 3,      // a factor negative or not finite
  TRS_DOSE = 4,        // neither 0 <= dose_lo <= dose_hi (both finite) nor dose_hi <= 0
  TRS_DAMAGE = 5,      // A or Ea not finite, A < 0, or A > 0 without Ea > 0
};

inline const char* thermal_response_message(int err)
{
  switch (err)
  {
  case TRS_NKNOTS: return "nknots must lie in 0..8, with temp and factor given when it is not 0";
  case TRS_TEMP: return "temp must be finite and strictly ascending";
  case TRS_FACTOR: return "factor must be >= 0 and finite";
  case TRS_DOSE: return "the dose range must satisfy 0 <= dose_lo <= dose_hi (finite), or dose_hi <= 0 for no shutdown";
  case TRS_DAMAGE: return "A and Ea must be positive and finite (A = 0 switches the damage off)";
  default: return "";
  }
}

// The response law.  The slots behind nknots repeat the last knot's factor under a temperature of +infinity, so the
// kernel walks all eight without reading nknots; t_last / f_last repeat the last knot for the same reason.
struct ThermalResponse
{
  double temp[THERMAL_MAX_KNOTS], factor[THERMAL_MAX_KNOTS];
  double t_last = 0.0, f_last = 1.0;
  double dose_lo = 0.0, dose_hi = 0.0;   // dose_hi <= 0: no shutdown
  double phi_max = 1.0;                  // max_j factor[j], 1 without knots: the step rule's bound of phi
  int nknots = 0;
  ThermalResponse()
  {
    for (int j = 0; j < THERMAL_MAX_KNOTS; ++j)
      temp[j] = HUGE_VAL, factor[j] = 1.0;
  }
  bool active() const { return nknots > 0 || dose_hi > 0.0; }
  bool same(const ThermalResponse& o) const
  {
    bool eq = nknots == o.nknots && (dose_hi > 0.0) == (o.dose_hi > 0.0);
    if (eq && dose_hi > 0.0)
      eq = dose_lo == o.dose_lo && dose_hi == o.dose_hi;
    for (int j = 0; eq && j < nknots; ++j)
      eq = temp[j] == o.temp[j] && factor[j] == o.factor[j];
    return eq;
  }
};

inline int thermal_response_check(int nknots, const double* temp, const double* factor, double dose_lo, double dose_hi,
                                  ThermalResponse* out)
{
  if (nknots < 0 || nknots > THERMAL_MAX_KNOTS || (nknots > 0 && (!temp || !factor)))
    return TRS_NKNOTS;
  for (int j = 0; j < nknots; ++j)
  {
    if (!std::isfinite(temp[j]) || (j > 0 && !(temp[j] > temp[j - 1])))
      return TRS_TEMP;
    if (!std::isfinite(factor[j]) || !(factor[j] >= 0.0))
      return TRS_FACTOR;
  }
  if (std::isnan(dose_hi) || (dose_hi > 0.0 && !(std::isfinite(dose_hi) && dose_lo >= 0.0 && dose_lo <= dose_hi)))
    return TRS_DOSE;
  ThermalResponse R;
  R.nknots = nknots;
  for (int j = 0; j < nknots; ++j)
  {
    R.temp[j] = temp[j], R.factor[j] = factor[j];
    R.phi_max = j == 0 ? factor[0] : std::fmax(R.phi_max, factor[j]);
  }
  if (nknots > 0)
  {
    R.t_last = temp[nknots - 1], R.f_last = factor[nknots - 1];
    for (int j = nknots; j < THERMAL_MAX_KNOTS; ++j)
      R.factor[j] = R.f_last;
  }
  if (dose_hi > 0.0)
    R.dose_lo = dose_lo, R.dose_hi = dose_hi;
  *out = R;
  return TRS_OK;
}

// The damage law; A == 0: off
struct ThermalDamage
{
  double A = 0.0, Ea = 0.0, lnA = 0.0;
  bool on() const { return A > 0.0; }
  bool same(const ThermalDamage& o) const { return A == o.A && (A == 0.0 || Ea == o.Ea); }
};

inline int thermal_damage_check(double A, double Ea, ThermalDamage* out)
{
  if (!std::isfinite(A) || A < 0.0 || !std::isfinite(Ea) || (A > 0.0 && !(Ea > 0.0)))
    return TRS_DAMAGE;
  ThermalDamage D;
  if (A > 0.0)
    D.A = A, D.Ea = Ea, D.lnA = std::log(A);
  *out = D;
  return TRS_OK;
}

// The three laws, for the kernel and for the host (the driver prints them).  P walks the eight slots in ascending order
// and keeps the ends of the last segment whose left knot lies at or below T, by compare and select: no index is computed,
// so the table stays in the scalar registers the kernel arguments arrive in, and one division follows.  A slot behind
// nknots is never taken (its temperature is +infinity); the segment that starts at the last knot is overridden by f_last.
FUS_RESPONSE_FN double thermal_response_P(const ThermalResponse& R, double T)
{
  FUS_NO_CONTRACT
  if (R.nknots == 0)
    return 1.0;
  double t0 = R.temp[0], t1 = R.temp[1], f0 = R.factor[0], f1 = R.factor[1];
  for (int j = 1; j + 1 < THERMAL_MAX_KNOTS; ++j)
  {
    const bool take = T >= R.temp[j];
    t0 = take ? R.temp[j] : t0, t1 = take ? R.temp[j + 1] : t1;
    f0 = take ? R.factor[j] : f0, f1 = take ? R.factor[j + 1] : f1;
  }
  const double w = (T - t0) / (t1 - t0);
  const double seg = f0 + (f1 - f0) * w;
  const double p = T >= R.temp[0] ? seg : R.factor[0];
  return T >= R.t_last ? R.f_last : p;
}

FUS_RESPONSE_FN double thermal_response_S(const ThermalResponse& R, double D)
{
  FUS_NO_CONTRACT
  if (!(R.dose_hi > 0.0) || D <= R.dose_lo)
    return 1.0;
  return D >= R.dose_hi ? 0.0 : (R.dose_hi - D) / (R.dose_hi - R.dose_lo);
}

FUS_RESPONSE_FN double thermal_damage_rate(double lnA, double Ea, double T)
{
  FUS_NO_CONTRACT
  const double TK = T + 273.15;
  const double RT = GAS_CONSTANT * TK;
  const double q = Ea / RT;
  return exp(lnA - q);
}
} // namespace fus

#endif
