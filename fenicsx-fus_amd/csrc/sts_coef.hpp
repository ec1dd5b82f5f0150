// Coefficients of the stabilised Runge-Kutta-Legendre scheme of second order (RKL2: Meyer, Balsara and Aslam,
// J. Comput. Phys. 257, 2014) behind fus_thermal_steps_sts (fusmi.h "bioheat").  Plain C++: no HIP header is needed, a
// host program may include this file (tests/cpp/sts_coef_driver.cpp).
//
// For s stages, all in double and in exactly this order of operations (thermal.rkl2_coefficients mirrors it bit for bit):
//   b_0 = b_1 = b_2 = 1/3,   b_j = (j^2 + j - 2) / (2 j (j + 1)) for j >= 3,   a_j = 1 - b_j
//   w1 = 4 / (s^2 + s - 2),  mut_1 = b_1 w1
//   mu_j  = (2j - 1) / j * b_j / b_{j-1}        nu_j  = -((j - 1) / j) * b_j / b_{j-2}
//   mut_j = mu_j w1                             gat_j = -(a_{j-1} mut_j)                      j = 2..s
// One step of size dt of y' = f(y):
//   Y_0 = y,  F_0 = f(Y_0),  Y_1 = Y_0 + mut_1 dt F_0
//   Y_j = mu_j Y_{j-1} + nu_j Y_{j-2} + (1 - mu_j - nu_j) Y_0 + mut_j dt f(Y_{j-1}) + gat_j dt F_0,   y <- Y_s
// stable on the negative real axis for dt lambda <= beta_s = (s^2 + s - 2) / 2.  The stage count is held to 2..32: the
// range over which max |R| <= 1 on [-beta_s, 0] and the rounding behaviour of the recurrence have been checked.
#ifndef FUS_STS_COEF_HPP
#define FUS_STS_COEF_HPP

namespace fus
{
constexpr int STS_MIN_STAGES = 2, STS_MAX_STAGES = 32;

// entries 1..s are used (mu, nu and gat of stage 1 are 0); entry 0 stays 0
struct StsCoef
{
  int s;
  double mu[STS_MAX_STAGES + 1], nu[STS_MAX_STAGES + 1], mut[STS_MAX_STAGES + 1], gat[STS_MAX_STAGES + 1];
};

inline bool sts_stages_ok(int s) { return s >= STS_MIN_STAGES && s <= STS_MAX_STAGES; }

inline double sts_b(int j)
{
  const double x = (double)j;
  return j < 3 ? 1.0 / 3.0 : (x * x + x - 2.0) / (2.0 * x * (x + 1.0));
}

// beta_s: the scheme is stable for dt lambda_max <= beta_s
inline double sts_beta(int s)
{
  const double x = (double)s;
  return (x * x + x - 2.0) / 2.0;
}

// false (and *c untouched) when s is outside 2..32
inline bool sts_coefficients(int s, StsCoef* c)
{
  if (!sts_stages_ok(s))
    return false;
  const double x = (double)s;
  const double w1 = 4.0 / (x * x + x - 2.0);
  c->s = s;
  for (int j = 0; j <= STS_MAX_STAGES; ++j)
    c->mu[j] = c->nu[j] = c->mut[j] = c->gat[j] = 0.0;
  c->mut[1] = sts_b(1) * w1;
  for (int j = 2; j <= s; ++j)
  {
    const double y = (double)j;
    c->mu[j] = (2.0 * y - 1.0) / y * sts_b(j) / sts_b(j - 1);
    c->nu[j] = -((y - 1.0) / y) * sts_b(j) / sts_b(j - 2);
    c->mut[j] = c->mu[j] * w1;
    c->gat[j] = -((1.0 - sts_b(j - 1)) * c->mut[j]);
  }
  return true;
}
} // namespace fus

#endif
