// cpp_transducer.cpp -- the Rayleigh integral through include/fusmi.hpp: the on-axis field of a circular piston against
// its closed form.  A piston of radius a = 10 mm, uniformly driven with the normal velocity v0 at 0.5 MHz in water, is
// sampled by n = 2000 equal-area Fibonacci points (radius a sqrt((i + 1/2) / n), azimuth i pi (3 - sqrt 5), dA = pi a^2 / n,
// q = v0 dA); on its axis
//   |P(z)| = 2 rho c v0 |sin(k (sqrt(z^2 + a^2) - z) / 2)|.
// Prints  peak=<2 rho c v0> axis_err=<max | |P| - closed form | / peak, double> mixed_err=<the same with FUS_RAY_MIXED>
// chunks=<source chunks the call used> grad_err=<max |dP/dz - central difference| / max |dP/dz|>  and exits 0 when
// axis_err <= 1e-5, mixed_err <= 1e-4 and grad_err <= 1e-5.   Usage: cpp_transducer
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "fusmi.hpp"

int main()
{
  const double pi = 3.14159265358979323846;
  const double f = 0.5e6, c = 1500.0, rho = 1000.0, v0 = 1.0, a = 0.010, k = 2 * pi * f / c;
  const int n = 2000, nz = 81;
  std::vector<double> xyz((size_t)n * 3), q((size_t)n * 2), tgt((size_t)nz * 3, 0.0);
  for (int i = 0; i < n; ++i)
  {
    const double r = a * std::sqrt((i + 0.5) / n), phi = i * pi * (3.0 - std::sqrt(5.0));
    xyz[3 * i] = r * std::cos(phi), xyz[3 * i + 1] = r * std::sin(phi), xyz[3 * i + 2] = 0.0;
    q[2 * i] = v0 * pi * a * a / n, q[2 * i + 1] = 0.0;
  }
  for (int j = 0; j < nz; ++j)
    tgt[3 * j + 2] = 0.020 + 0.001 * j;

  try
  {
    fusmi::Context ctx(0);
    const double peak = 2 * rho * c * v0;
    double err[2] = {0, 0};
    for (int prec = 0; prec < 2; ++prec)
    {
      const std::vector<double> P = fusmi::rayleigh(ctx, xyz, q, tgt, f, c, rho, 0.0, FUS_RAY_P, prec ? FUS_RAY_MIXED : FUS_RAY_F64);
      for (int j = 0; j < nz; ++j)
      {
        const double z = tgt[3 * j + 2], ref = peak * std::fabs(std::sin(0.5 * k * (std::sqrt(z * z + a * a) - z)));
        err[prec] = std::fmax(err[prec], std::fabs(std::hypot(P[j], P[nz + j]) - ref) / peak);
      }
    }
    // dP/dz on the axis against central differences of P
    const double h = 1e-6;
    std::vector<double> tp(tgt), tm(tgt);
    for (int j = 0; j < nz; ++j)
      tp[3 * j + 2] += h, tm[3 * j + 2] -= h;
    const std::vector<double> G = fusmi::rayleigh(ctx, xyz, q, tgt, f, c, rho, 0.0, FUS_RAY_P | FUS_RAY_GRAD);
    const std::vector<double> Pp = fusmi::rayleigh(ctx, xyz, q, tp, f, c, rho), Pm = fusmi::rayleigh(ctx, xyz, q, tm, f, c, rho);
    double ge = 0, gmax = 0;
    for (int j = 0; j < nz; ++j)
    {
      const std::complex<double> gz(G[6 * nz + j], G[7 * nz + j]);
      const std::complex<double> fd((Pp[j] - Pm[j]) / (2 * h), (Pp[nz + j] - Pm[nz + j]) / (2 * h));
      ge = std::fmax(ge, std::abs(gz - fd)), gmax = std::fmax(gmax, std::abs(gz));
    }
    const fusmi::RayleighPlan plan = fusmi::rayleigh_plan(ctx, n, nz);
    printf("peak=%.17g axis_err=%.3e mixed_err=%.3e chunks=%lld grad_err=%.3e\n", peak, err[0], err[1], (long long)plan.chunks,
           ge / gmax);
    return (err[0] <= 1e-5 && err[1] <= 1e-4 && ge / gmax <= 1e-5) ? 0 : 1;
  }
  catch (const fusmi::Error& e)
  {
    fprintf(stderr, "fusmi error %d: %s\n", e.code, e.what());
    return 3;
  }
}
