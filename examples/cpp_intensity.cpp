// cpp_intensity.cpp -- the gradient operator's pair form through the classes of include/fusmi.hpp: the time-averaged
// intensity of a plane wave.  On a box one wavelength long (12 x 2 x 2 cells of degree 4) the harmonic maps of
// p = A cos(w t - kappa x) are C = A cos(kappa x), S = A sin(kappa x); with the coefficient 1 / (2 rho w) the pair form
//   I = (C grad S - S grad C) / (2 rho w)
// is A^2 / (2 rho c) along +x and zero across.  After a monitored run the same maps come from the model
// (model.intensity(nharm) reads them on the device); here they are set analytically, so the value can be checked.
// Prints  I0=<A^2/(2 rho c)> err_x=<max |I_x - I0| / I0> transverse=<max |I_y|, |I_z| / I0> velocity_err=<max | |w| - A/(rho c) |
// / (A/(rho c))> and exits 0 when all three errors are below 1e-4.   Usage: cpp_intensity
#include <cmath>
#include <cstdio>
#include <vector>

#include "fusmi.hpp"

int main()
{
  using T = double;
  constexpr int P = 4, N = P + 1, Nd = N * N * N;
  const double A = 6e4, rho = 1000.0, c = 1500.0, f0 = 0.5e6, pi = 3.14159265358979323846;
  const double lam = c / f0, kappa = 2 * pi / lam, w = 2 * pi * f0;
  const int n[3] = {12, 2, 2};
  const double h[3] = {lam / n[0], lam / 8, lam / 8};
  // GLL points of degree 4 on [0, 1]
  const double g = std::sqrt(3.0 / 7.0);
  const double nodes[N] = {0.0, 0.5 * (1 - g), 0.5, 0.5 * (1 + g), 1.0};

  // vertices (x fastest in the cell's vertex order v = vx + 2 vy + 4 vz), DOF lattice, tensor dofmap
  const int nvx[3] = {n[0] + 1, n[1] + 1, n[2] + 1}, ndx[3] = {n[0] * P + 1, n[1] * P + 1, n[2] * P + 1};
  const int64_t nnodes = (int64_t)nvx[0] * nvx[1] * nvx[2], ndofs = (int64_t)ndx[0] * ndx[1] * ndx[2];
  const int64_t ncells = (int64_t)n[0] * n[1] * n[2];
  std::vector<double> gx((size_t)nnodes * 3), xdof((size_t)ndofs);
  for (int i = 0; i < nvx[0]; ++i)
    for (int j = 0; j < nvx[1]; ++j)
      for (int k = 0; k < nvx[2]; ++k)
      {
        const size_t v = ((size_t)i * nvx[1] + j) * nvx[2] + k;
        gx[3 * v] = i * h[0], gx[3 * v + 1] = j * h[1], gx[3 * v + 2] = k * h[2];
      }
  std::vector<int32_t> gdm((size_t)ncells * 8), tdm((size_t)ncells * Nd);
  int64_t e = 0;
  for (int ci = 0; ci < n[0]; ++ci)
    for (int cj = 0; cj < n[1]; ++cj)
      for (int ck = 0; ck < n[2]; ++ck, ++e)
      {
        for (int v = 0; v < 8; ++v)
          gdm[e * 8 + v] = (int32_t)((((size_t)ci + (v & 1)) * nvx[1] + cj + ((v >> 1) & 1)) * nvx[2] + ck + (v >> 2));
        for (int a = 0; a < N; ++a)
          for (int b = 0; b < N; ++b)
            for (int d = 0; d < N; ++d)
            {
              const int64_t dof = (((int64_t)ci * P + a) * ndx[1] + cj * P + b) * ndx[2] + ck * P + d;
              tdm[e * Nd + (a * N + b) * N + d] = (int32_t)dof;
              xdof[dof] = (ci + nodes[a]) * h[0];
            }
      }

  try
  {
    auto ctx = std::make_shared<fusmi::Context>(0);
    fusmi::SpaceView<T> V;
    V.tdim = 3, V.ncells = ncells, V.ndofs = ndofs, V.nnodes = nnodes;
    V.tensor_dofmap = tdm.data(), V.nodes1d = nodes, V.geom_x = gx.data(), V.geom_dofmap = gdm.data();
    fusmi::SpectralOperatorData<T, P> data(ctx, V);

    std::vector<T> C(ndofs), S(ndofs), coef((size_t)ncells, 1.0 / (2 * rho * w));
    for (int64_t i = 0; i < ndofs; ++i)
      C[i] = A * std::cos(kappa * xdof[i]), S[i] = A * std::sin(kappa * xdof[i]);
    const std::vector<T> I = data.gradient_pairs(1, C.data(), S.data(), coef.data());

    // the particle velocity amplitude of the same wave from the nodal gradients of the maps: A / (rho c)
    const std::vector<T> gC = data.gradient(C.data()), gS = data.gradient(S.data());
    const double I0 = A * A / (2 * rho * c);
    double ex = 0, et = 0, ev = 0;
    for (int64_t i = 0; i < ndofs; ++i)
    {
      ex = std::fmax(ex, std::fabs(I[i] - I0) / I0);
      et = std::fmax(et, std::fmax(std::fabs(I[ndofs + i]), std::fabs(I[2 * ndofs + i])) / I0);
      double s = 0;
      for (int d = 0; d < 3; ++d)
        s += gC[d * ndofs + i] * gC[d * ndofs + i] + gS[d * ndofs + i] * gS[d * ndofs + i];
      ev = std::fmax(ev, std::fabs(std::sqrt(s) / (rho * w) - A / (rho * c)) / (A / (rho * c)));
    }
    printf("I0=%.17g err_x=%.3e transverse=%.3e velocity_err=%.3e\n", I0, ex, et, ev);
    return (ex < 1e-4 && et < 1e-4 && ev < 1e-4) ? 0 : 1;
  }
  catch (const fusmi::Error& err)
  {
    fprintf(stderr, "fusmi error %d: %s\n", err.code, err.what());
    return 3;
  }
}
