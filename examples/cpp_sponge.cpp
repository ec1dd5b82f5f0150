// cpp_sponge.cpp -- the Linear model with absorbing layers through the classes of include/fusmi.hpp: set_sponge gives
// every DOF a damping rate sigma (1/s, zero outside the layers; fenicsxfus_amd.sponge.layer_sigma builds such profiles),
// the default source on the tag-1 boundary drives the model for nsteps steps from rest, the first-order condition stays
// on the tag-2 faces behind the layers.  Mesh and materials come from a flat binary file (written by
// tests/test_sponge_cpp.py).  Usage: cpp_sponge <in.bin> <out.bin>
//   int64  tdim, P, ncells, ndofs, nnodes, nfacets, nsteps
//   double dt, freq, amp, speed
//   int32  tensor_dofmap[ncells * (P+1)^tdim];  double nodes1d[P+1];  double geom_x[nnodes * 3];
//   int32  geom_dofmap[ncells * 2^tdim];  int32 facet cells, local facets, tags [nfacets each];  double c, rho [ncells]
//   double sigma[ndofs]
// out.bin: double u[ndofs], v[ndofs] after nsteps steps, then u[ndofs], v[ndofs] after clear_sponge, set_sponge and one
// more sub-step of length dt by sponge_apply.
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
int run(FILE* f, const std::vector<int64_t>& h, const char* outpath)
{
  using T = double;
  const int tdim = (int)h[0];
  const int64_t ncells = h[2], ndofs = h[3], nnodes = h[4], nfacets = h[5], nsteps = h[6];
  const int N = P + 1, Nd = tdim == 3 ? N * N * N : N * N, nv = tdim == 3 ? 8 : 4;
  const auto par = arr<double>(f, 4);
  const double dt = par[0], freq = par[1], amp = par[2], speed = par[3];
  auto tdm = arr<int32_t>(f, (size_t)ncells * Nd);
  auto nodes = arr<double>(f, N);
  auto gx = arr<double>(f, (size_t)nnodes * 3);
  auto gdm = arr<int32_t>(f, (size_t)ncells * nv);
  auto fc = arr<int32_t>(f, nfacets), fl = arr<int32_t>(f, nfacets), ft = arr<int32_t>(f, nfacets);
  auto c0 = arr<double>(f, ncells), rho0 = arr<double>(f, ncells);
  auto sigma = arr<double>(f, (size_t)ndofs);

  auto ctx = std::make_shared<fusmi::Context>(0);
  fusmi::SpaceView<T> V;
  V.tdim = tdim, V.ncells = ncells, V.ndofs = ndofs, V.nnodes = nnodes;
  V.tensor_dofmap = tdm.data(), V.nodes1d = nodes.data(), V.geom_x = gx.data(), V.geom_dofmap = gdm.data();
  auto data = std::make_shared<fusmi::SpectralOperatorData<T, P>>(ctx, V);
  fusmi::FacetView F;
  F.nfacets = nfacets, F.cells = fc.data(), F.local_facets = fl.data(), F.tags = ft.data();
  fusmi::LinearSpectral3D<T, P> model(data, F, c0.data(), rho0.data(), freq, amp, speed);
  model.init();
  model.set_sponge(sigma);
  model.rk4_steps(0.0, dt, nsteps);

  const auto u = model.u_sol(), v = model.v_sol();
  double vmax = 0.0;
  for (T x : v)
    vmax = std::fmax(vmax, std::fabs(x));
  model.clear_sponge();   // off: u and v are kept
  model.set_sponge(sigma);
  model.sponge_apply(dt);
  const auto u2 = model.u_sol(), v2 = model.v_sol();
  printf("steps %lld max|v| %.17g\n", (long long)nsteps, vmax);
  FILE* o = fopen(outpath, "wb");
  if (!o)
    return 2;
  for (const auto* x : {&u, &v, &u2, &v2})
    fwrite(x->data(), sizeof(T), x->size(), o);
  fclose(o);
  return 0;
}
} // namespace

int main(int argc, char** argv)
{
  if (argc < 3)
  {
    fprintf(stderr, "usage: %s <in.bin> <out.bin>\n", argv[0]);
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
    case 2: return run<2>(f, h, argv[2]);
    case 3: return run<3>(f, h, argv[2]);
    case 4: return run<4>(f, h, argv[2]);
    default: fprintf(stderr, "degree %lld not built into this example\n", (long long)h[1]); return 2;
    }
  }
  catch (const fusmi::Error& e)
  {
    fprintf(stderr, "fusmi error %d: %s\n", e.code, e.what());
    return 3;
  }
}
