// cpp_bioheat_sts.cpp -- the bioheat class of include/fusmi.hpp with super-time-stepping: heat a block of tissue with
// a given power density and let it cool, in RKL2 steps of `stages` stages at the step stable_dt(stages) gives, and
// print the energy balance and the peak dose.  Mesh, materials and the heat field come from a flat binary file (written
// by tests/test_gpu_sts.py).  Usage: cpp_bioheat_sts <in.bin>
//   int64  tdim, P, ncells, ndofs, nnodes, nheat (steps with the heat on), ncool (steps with it off), stages
//   int32  tensor_dofmap[ncells * (P+1)^tdim];  double nodes1d[P+1];  double geom_x[nnodes * 3];
//   int32  geom_dofmap[ncells * 2^tdim];  double conductivity, rho_c, perfusion [ncells];  double q[ndofs]
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
  const int64_t ncells = h[2], ndofs = h[3], nnodes = h[4], nheat = h[5], ncool = h[6];
  const int stages = (int)h[7];
  const int N = P + 1, Nd = tdim == 3 ? N * N * N : N * N, nv = tdim == 3 ? 8 : 4;
  auto tdm = arr<int32_t>(f, (size_t)ncells * Nd);
  auto nodes = arr<double>(f, N);
  auto gx = arr<double>(f, (size_t)nnodes * 3);
  auto gdm = arr<int32_t>(f, (size_t)ncells * nv);
  auto k = arr<double>(f, ncells), rho_c = arr<double>(f, ncells), w = arr<double>(f, ncells);
  auto q = arr<double>(f, ndofs);

  auto ctx = std::make_shared<fusmi::Context>(0);
  fusmi::SpaceView<T> V;
  V.tdim = tdim, V.ncells = ncells, V.ndofs = ndofs, V.nnodes = nnodes;
  V.tensor_dofmap = tdm.data(), V.nodes1d = nodes.data(), V.geom_x = gx.data(), V.geom_dofmap = gdm.data();
  auto data = std::make_shared<fusmi::SpectralOperatorData<T, P>>(ctx, V);

  fusmi::BioheatSpectral3D<T, P> bio(data, k.data(), rho_c.data(), w.data(), 37.0);
  bio.init();
  bio.set_heat(q.data());
  const double dt = bio.stable_dt(stages);   // 0.72 (s^2 + s - 2) / 2 over the power iteration's lambda_max
  bio.steps(dt, nheat, 1.0, stages);   // sonication
  bio.steps(dt, ncool, 0.0, stages);   // cooling

  // energy balance: sum m_C theta against the heat put in, m_C = M(rho_c) 1
  std::vector<T> one(ndofs, 1.0), m_c(ndofs, 0.0);
  fusmi::MassSpectral3D<T, P> mass(data);
  mass(one.data(), rho_c.data(), m_c.data());
  const auto theta = bio.rise(), heat = bio.heat();
  const auto dose = bio.dose();
  double energy = 0, power = 0;
  for (int64_t i = 0; i < ndofs; ++i)
    energy += m_c[i] * theta[i], power += heat[i];
  printf("stages %d stable_dt %.17g rk4_stable_dt %.17g\n", stages, dt, bio.stable_dt());
  printf("energy %.17g heat_in %.17g\n", energy, power * dt * (double)nheat);
  printf("peak_rise %.17g peak_cem43 %.17g\n", *std::max_element(theta.begin(), theta.end()),
         *std::max_element(dose.begin(), dose.end()));
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
