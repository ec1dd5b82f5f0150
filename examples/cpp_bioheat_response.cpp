// cpp_bioheat_response.cpp -- the bioheat class of include/fusmi.hpp with a perfusion that responds to heat and dose, and
// the Arrhenius damage integral beside CEM43: heat a block of tissue from a given rise, once with the passive perfusion
// and once with the response, and print what the response changes.  Mesh, materials, the heat field and the start state
// come from a flat binary file (written by tests/test_gpu_thermal_response.py).  Usage: cpp_bioheat_response <in.bin>
//   int64  tdim, P, ncells, ndofs, nnodes, nsteps, nknots
//   double dose_lo, dose_hi, A, Ea;  double temp[nknots], factor[nknots]
//   int32  tensor_dofmap[ncells * (P+1)^tdim];  double nodes1d[P+1];  double geom_x[nnodes * 3];
//   int32  geom_dofmap[ncells * 2^tdim];  double conductivity, rho_c, perfusion [ncells];  double q[ndofs], rise0[ndofs]
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

template <typename U>
double peak(const std::vector<U>& v)
{
  return (double)*std::max_element(v.begin(), v.end());
}

template <int P>
int run(FILE* f, const std::vector<int64_t>& h)
{
  using T = double;
  const int tdim = (int)h[0];
  const int64_t ncells = h[2], ndofs = h[3], nnodes = h[4], nsteps = h[5], nknots = h[6];
  const int N = P + 1, Nd = tdim == 3 ? N * N * N : N * N, nv = tdim == 3 ? 8 : 4;
  auto s = arr<double>(f, 4);
  auto temp = arr<double>(f, (size_t)nknots), factor = arr<double>(f, (size_t)nknots);
  auto tdm = arr<int32_t>(f, (size_t)ncells * Nd);
  auto nodes = arr<double>(f, N);
  auto gx = arr<double>(f, (size_t)nnodes * 3);
  auto gdm = arr<int32_t>(f, (size_t)ncells * nv);
  auto k = arr<double>(f, ncells), rho_c = arr<double>(f, ncells), w = arr<double>(f, ncells);
  auto q = arr<double>(f, ndofs), rise0 = arr<double>(f, ndofs);

  auto ctx = std::make_shared<fusmi::Context>(0);
  fusmi::SpaceView<T> V;
  V.tdim = tdim, V.ncells = ncells, V.ndofs = ndofs, V.nnodes = nnodes;
  V.tensor_dofmap = tdm.data(), V.nodes1d = nodes.data(), V.geom_x = gx.data(), V.geom_dofmap = gdm.data();
  auto data = std::make_shared<fusmi::SpectralOperatorData<T, P>>(ctx, V);

  fusmi::BioheatSpectral3D<T, P> bio(data, k.data(), rho_c.data(), w.data(), 37.0);
  bio.set_heat(q.data());
  bio.set_damage(s[2], s[3]);

  // the passive tissue first, at its own stable step
  bio.init();
  bio.set_state(rise0.data());
  const double dt_passive = bio.stable_dt();
  bio.steps(dt_passive, nsteps);
  printf("passive_dt %.17g passive_peak_rise %.17g\n", dt_passive, peak(bio.rise()));

  // then the responding one: the response is set BEFORE stable_dt, whose operator takes the largest factor
  bio.set_response(temp, factor, s[0], s[1]);
  bio.init();   // rise, dose and damage back to zero
  bio.set_state(rise0.data());
  const double dt = bio.stable_dt();
  bio.steps(dt, nsteps);
  const auto w_eff = bio.perfusion();
  bio.clear_response();
  const auto w_passive = bio.perfusion();
  double lo = 1e300, hi = 0;
  for (int64_t i = 0; i < ndofs; ++i)
    if (w_passive[i] > 0)
      lo = std::min(lo, w_eff[i] / w_passive[i]), hi = std::max(hi, w_eff[i] / w_passive[i]);
  printf("stable_dt %.17g peak_rise %.17g peak_cem43 %.17g peak_damage %.17g\n", dt, peak(bio.rise()), peak(bio.dose()),
         peak(bio.damage()));
  printf("phi_min %.17g phi_max %.17g\n", lo, hi);
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
  const auto h = arr<int64_t>(f, 7);
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
