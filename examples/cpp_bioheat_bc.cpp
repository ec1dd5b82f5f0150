// cpp_bioheat_bc.cpp -- the bioheat class of include/fusmi.hpp with boundary conditions: one face of a heated block of
// tissue is held at a fixed temperature, another is cooled by water, the rest stay insulating; a few RK4 steps at the
// step stable_dt() gives for that boundary, then the values are printed.  Mesh, materials, heat field and the two facet
// lists come from a flat binary file (written by tests/test_gpu_thermal_bc.py).  Usage: cpp_bioheat_bc <in.bin>
//   int64  tdim, P, ncells, ndofs, nnodes, nsteps, nfixed_facets, nconv_facets
//   double fixed_rise, h_c, coolant_rise          (K over t_base, W/m^2/K, K over t_base)
//   int32  tensor_dofmap[ncells * (P+1)^tdim];  double nodes1d[P+1];  double geom_x[nnodes * 3];
//   int32  geom_dofmap[ncells * 2^tdim];  double conductivity, rho_c, perfusion [ncells];  double q[ndofs]
//   int32  fixed_cells, fixed_local_facets [nfixed_facets];  int32 conv_cells, conv_local_facets [nconv_facets]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fusmi.hpp"

namespace
{
template <typename U>
std::vector<U> arr(FILE* f, size_t n)
{
  std::vector<U> v(n);
  if (n && fread(v.data(), sizeof(U), n, f) != n)
  {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}

template <int P>
int run(FILE* f, const std::vector<int64_t>& h)
{
  using T = double;
  const int tdim = (int)h[0];
  const int64_t ncells = h[2], ndofs = h[3], nnodes = h[4], nsteps = h[5], nfx = h[6], ncv = h[7];
  const int N = P + 1, Nd = tdim == 3 ? N * N * N : N * N, nv = tdim == 3 ? 8 : 4;
  const auto par = arr<double>(f, 3);
  const double fixed_rise = par[0], h_c = par[1], coolant_rise = par[2];
  auto tdm = arr<int32_t>(f, (size_t)ncells * Nd);
  auto nodes = arr<double>(f, N);
  auto gx = arr<double>(f, (size_t)nnodes * 3);
  auto gdm = arr<int32_t>(f, (size_t)ncells * nv);
  auto k = arr<double>(f, ncells), rho_c = arr<double>(f, ncells), w = arr<double>(f, ncells);
  auto q = arr<double>(f, ndofs);
  auto fxc = arr<int32_t>(f, nfx), fxl = arr<int32_t>(f, nfx), cvc = arr<int32_t>(f, ncv), cvl = arr<int32_t>(f, ncv);

  auto ctx = std::make_shared<fusmi::Context>(0);
  fusmi::SpaceView<T> V;
  V.tdim = tdim, V.ncells = ncells, V.ndofs = ndofs, V.nnodes = nnodes;
  V.tensor_dofmap = tdm.data(), V.nodes1d = nodes.data(), V.geom_x = gx.data(), V.geom_dofmap = gdm.data();
  auto data = std::make_shared<fusmi::SpectralOperatorData<T, P>>(ctx, V);

  // the facet diagonal sum_facets c |J_f| w_a w_b: with c = 1 its support is the set of DOFs on the fixed face, with
  // c = h_c it is the convective face's m_H
  std::vector<T> one(ncells, 1.0), hc(ncells, h_c), on_fixed(ndofs, 0.0), m_h(ndofs, 0.0);
  fusmi::check(fus_facet_diag(data->handle(), nfx, fxc.data(), fxl.data(), one.data(), on_fixed.data()));
  fusmi::check(fus_facet_diag(data->handle(), ncv, cvc.data(), cvl.data(), hc.data(), m_h.data()));
  std::vector<std::uint8_t> fixed(ndofs);
  for (int64_t i = 0; i < ndofs; ++i)
    fixed[i] = on_fixed[i] > 0.0;
  std::vector<T> rise_d(ndofs, fixed_rise), rise_ext(ndofs, coolant_rise);

  fusmi::BioheatSpectral3D<T, P> bio(data, k.data(), rho_c.data(), w.data(), 37.0);
  const double dt_insulating = bio.stable_dt();
  bio.set_boundary(fixed.data(), rise_d.data(), m_h.data(), rise_ext.data());
  const auto info = bio.boundary_info();
  bio.init();
  bio.set_heat(q.data());
  const double dt = bio.stable_dt();   // of the operator with the surface term and without the fixed DOFs
  bio.steps(dt, nsteps);

  const auto theta = bio.rise();
  const auto dose = bio.dose();
  double held_lo = 1e300, held_hi = -1e300, cooled_lo = 1e300;
  for (int64_t i = 0; i < ndofs; ++i)
  {
    if (fixed[i])
      held_lo = std::min(held_lo, theta[i]), held_hi = std::max(held_hi, theta[i]);
    else if (m_h[i] > 0.0)
      cooled_lo = std::min(cooled_lo, theta[i]);
  }
  printf("nfixed %lld nconvective %lld\n", (long long)info.first, (long long)info.second);
  printf("stable_dt %.17g insulating_stable_dt %.17g\n", dt, dt_insulating);
  printf("held_min %.17g held_max %.17g coolest_convective %.17g\n", held_lo, held_hi, cooled_lo);
  printf("peak_rise %.17g min_rise %.17g peak_cem43 %.17g\n", *std::max_element(theta.begin(), theta.end()),
         *std::min_element(theta.begin(), theta.end()), *std::max_element(dose.begin(), dose.end()));
  bio.clear_boundary();
  printf("after_clear %lld %lld\n", (long long)bio.boundary_info().first, (long long)bio.boundary_info().second);
  return 0;
}
} // namespace

int main(int argc, char** argv)
{
  if (argc < 2)
  {
    fprintf(stderr, "usage: %s <in.bin>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f)
  {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  const auto h = arr<int64_t>(f, 8);
  try
  {
    switch (h[1])
    {
    case 2: return run<2>(f, h);
    case 3: return run<3>(f, h);
    case 4: return run<4>(f, h);
    default: fprintf(stderr, "degree %lld not built into this example\n", (long long)h[1]); return 2;
    }
  }
  catch (const fusmi::Error& e)
  {
    fprintf(stderr, "fusmi error %d: %s\n", e.code, e.what());
    return 3;
  }
}
