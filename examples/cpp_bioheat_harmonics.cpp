// cpp_bioheat_harmonics.cpp -- the per-harmonic heat load of include/fusmi.hpp (fusmi.h "per-harmonic heat load"): a
// Westervelt model runs with the field monitor keeping nharm harmonics, a bioheat object on the same operator data takes
// its heat from them with the absorption alpha k^y of harmonic k, and a few thermal steps follow.  Prints the load summed
// over the DOFs next to the load of the fundamental alone.  Mesh, facets and materials come from a flat binary file
// (written by tests/test_gpu_harmonic_heat.py).  Usage: cpp_bioheat_harmonics <in.bin>
//   int64  tdim, P, ncells, ndofs, nnodes, nfacets, nwave (wave steps), nharm, nheat (thermal steps)
//   double freq, amp, speed, wave dt, y, thermal dt
//   int32  tensor_dofmap[ncells * (P+1)^tdim];  double nodes1d[P+1];  double geom_x[nnodes * 3];
//   int32  geom_dofmap[ncells * 2^tdim];  int32 facet cell, local facet, tag [nfacets]
//   double c0, rho0, delta0, beta0, conductivity, rho_c, perfusion, alpha [ncells];  double u0, v0 [ndofs]
#include <algorithm>
#include <cmath>
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
  const int tdim = (int)h[0], nharm = (int)h[7];
  const int64_t ncells = h[2], ndofs = h[3], nnodes = h[4], nfacets = h[5], nwave = h[6], nheat = h[8];
  const int N = P + 1, Nd = tdim == 3 ? N * N * N : N * N, nv = tdim == 3 ? 8 : 4;
  const auto s = arr<double>(f, 6);
  const double freq = s[0], amp = s[1], speed = s[2], wdt = s[3], y = s[4], dt = s[5];
  auto tdm = arr<int32_t>(f, (size_t)ncells * Nd);
  auto nodes = arr<double>(f, N);
  auto gx = arr<double>(f, (size_t)nnodes * 3);
  auto gdm = arr<int32_t>(f, (size_t)ncells * nv);
  auto fc = arr<int32_t>(f, nfacets), fl = arr<int32_t>(f, nfacets), ft = arr<int32_t>(f, nfacets);
  auto c0 = arr<double>(f, ncells), rho0 = arr<double>(f, ncells), delta0 = arr<double>(f, ncells),
       beta0 = arr<double>(f, ncells);
  auto k = arr<double>(f, ncells), rho_c = arr<double>(f, ncells), w = arr<double>(f, ncells), alpha = arr<double>(f, ncells);
  auto u0 = arr<double>(f, ndofs), v0 = arr<double>(f, ndofs);

  auto ctx = std::make_shared<fusmi::Context>(0);
  fusmi::SpaceView<T> V;
  V.tdim = tdim, V.ncells = ncells, V.ndofs = ndofs, V.nnodes = nnodes;
  V.tensor_dofmap = tdm.data(), V.nodes1d = nodes.data(), V.geom_x = gx.data(), V.geom_dofmap = gdm.data();
  auto data = std::make_shared<fusmi::SpectralOperatorData<T, P>>(ctx, V, 2);

  fusmi::FacetView facets{nfacets, fc.data(), fl.data(), ft.data()};
  fusmi::WesterveltSpectral3D<T, P> model(data, facets, c0.data(), rho0.data(), delta0.data(), beta0.data(), freq, amp,
                                          speed);
  model.init();
  model.set_state(u0.data(), v0.data());
  model.monitor(FUS_U, nharm);
  model.rk4_steps(0.0, wdt, nwave);

  // row k - 1: the absorption at k times the source frequency, alpha k^y
  std::vector<T> rows((size_t)nharm * ncells);
  for (int j = 1; j <= nharm; ++j)
    for (int64_t e = 0; e < ncells; ++e)
      rows[(size_t)(j - 1) * ncells + e] = alpha[e] * std::pow((double)j, y);

  fusmi::BioheatSpectral3D<T, P> bio(data, k.data(), rho_c.data(), w.data(), 37.0);
  bio.init();
  auto total = [&]
  {
    double sum = 0;
    for (const T x : bio.heat())
      sum += x;
    return sum;
  };
  bio.set_heat_from(model, rows.data(), 1);
  const double fundamental = total();
  bio.set_heat_from(model, rows.data(), nharm);
  const double load = total();
  bio.steps(dt, nheat, 1.0);
  const auto theta = bio.rise();
  printf("load %.17g fundamental %.17g\n", load, fundamental);
  printf("peak_rise %.17g\n", *std::max_element(theta.begin(), theta.end()));
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
  const auto h = arr<int64_t>(f, 9);
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
