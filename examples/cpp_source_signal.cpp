// cpp_source_signal.cpp -- a point source inside a small box, driven by a sampled Gaussian pulse, through the classes of
// include/fusmi.hpp: set_source_weights puts the source at a located point (cell + reference coordinates, the weights
// are the cell's Lagrange basis values there), set_source_signals plays one channel of samples at every weighted DOF.
// The tag-1 boundary, if the file lists one, plays the same channel.  Mesh, materials and the point come from a flat
// binary file (written by tests/test_gpu_volume_source.py).  Usage: cpp_source_signal <in.bin> <out.bin>
//   int64  tdim, P, ncells, ndofs, nnodes, nfacets, nsteps, nsamp, point_cell
//   double dt, ds, t_first, pulse_centre, pulse_width, strength, point_X[3]
//   int32  tensor_dofmap[ncells * (P+1)^tdim];  double nodes1d[P+1];  double geom_x[nnodes * 3];
//   int32  geom_dofmap[ncells * 2^tdim];  int32 facet cells, local facets, tags [nfacets each];  double c, rho [ncells]
// out.bin: double u[ndofs], v[ndofs] after nsteps steps from rest.
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
  const int64_t ncells = h[2], ndofs = h[3], nnodes = h[4], nfacets = h[5], nsteps = h[6], nsamp = h[7], cell = h[8];
  const int N = P + 1, Nd = tdim == 3 ? N * N * N : N * N, nv = tdim == 3 ? 8 : 4;
  const auto par = arr<double>(f, 9);
  const double dt = par[0], ds = par[1], t_first = par[2], centre = par[3], width = par[4], strength = par[5];
  auto tdm = arr<int32_t>(f, (size_t)ncells * Nd);
  auto nodes = arr<double>(f, N);
  auto gx = arr<double>(f, (size_t)nnodes * 3);
  auto gdm = arr<int32_t>(f, (size_t)ncells * nv);
  auto fc = arr<int32_t>(f, nfacets), fl = arr<int32_t>(f, nfacets), ft = arr<int32_t>(f, nfacets);
  auto c0 = arr<double>(f, ncells), rho0 = arr<double>(f, ncells);

  auto ctx = std::make_shared<fusmi::Context>(0);
  fusmi::SpaceView<T> V;
  V.tdim = tdim, V.ncells = ncells, V.ndofs = ndofs, V.nnodes = nnodes;
  V.tensor_dofmap = tdm.data(), V.nodes1d = nodes.data(), V.geom_x = gx.data(), V.geom_dofmap = gdm.data();
  auto data = std::make_shared<fusmi::SpectralOperatorData<T, P>>(ctx, V);
  fusmi::FacetView F;
  F.nfacets = nfacets, F.cells = fc.data(), F.local_facets = fl.data(), F.tags = ft.data();
  // (frequency, amplitude and speed describe the default waveform, which the signals replace)
  fusmi::LinearSpectral3D<T, P> model(data, F, c0.data(), rho0.data(), 1.0 / (8.0 * dt), 1.0, 1500.0);
  model.init();

  // the point source: w_d = strength * phi_d(X), phi_d the tensor-product Lagrange basis of the located cell
  std::vector<double> l((size_t)tdim * N);
  for (int d = 0; d < tdim; ++d)
    for (int i = 0; i < N; ++i)
    {
      double v = 1.0;
      for (int j = 0; j < N; ++j)
        if (j != i)
          v *= (par[6 + d] - nodes[j]) / (nodes[i] - nodes[j]);
      l[(size_t)d * N + i] = v;
    }
  std::vector<T> w((size_t)ndofs, 0.0);
  for (int k = 0; k < Nd; ++k)
  {
    const int i0 = tdim == 3 ? k / (N * N) : k / N, i1 = tdim == 3 ? (k / N) % N : k % N, i2 = k % N;
    const double phi = tdim == 3 ? l[i0] * l[N + i1] * l[2 * N + i2] : l[i0] * l[N + i1];
    w[(size_t)tdm[(size_t)cell * Nd + k]] += strength * phi;
  }
  model.set_source_weights(w.data());

  // one channel: a Gaussian pulse, sampled
  std::vector<double> pulse((size_t)nsamp);
  for (int64_t j = 0; j < nsamp; ++j)
  {
    const double s = (t_first + (double)j * ds - centre) / width;
    pulse[(size_t)j] = std::exp(-0.5 * s * s);
  }
  model.set_source_signals(1, nsamp, t_first, ds, pulse.data());
  model.rk4_steps(0.0, dt, nsteps);

  const auto u = model.u_sol(), v = model.v_sol();
  double umax = 0.0;
  for (T x : u)
    umax = std::fmax(umax, std::fabs(x));
  printf("steps %lld max|u| %.17g\n", (long long)nsteps, umax);
  FILE* o = fopen(outpath, "wb");
  if (!o)
    return 2;
  fwrite(u.data(), sizeof(T), u.size(), o);
  fwrite(v.data(), sizeof(T), v.size(), o);
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
  const auto h = arr<int64_t>(f, 9);
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
