// Host driver for csrc/thermal_response.hpp (tests/test_response_host.py): the header is plain C++, so this file is built
// with the host compiler alone, under AddressSanitizer + UBSan.
//   thermal_response_driver <in.bin>
//   in.bin:  int64 nknots, has_arrays, npts;  double dose_lo, dose_hi, A, Ea;  double temp[max(nknots, 0)], factor[same]
//            (read only if has_arrays);  double T[npts], D[npts]
//   out:     "err E" (the header's code for the response); for E != 0 "untouched U message ...", else
//            "active a nknots n phi_max x" and npts lines "V P S" with P(T[i]) and S(D[i]);
//            then "derr E" for the damage; for E != 0 "untouched U message ...", else "on o lnA x" and, if on, npts lines
//            "R r" with r(T[i]).  Values as hexadecimal floats.  Both structs hold a sentinel before the call, so that an
//            error that touched them would show.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "thermal_response.hpp"

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
} // namespace

int main(int argc, char** argv)
{
  if (argc != 2)
  {
    fprintf(stderr, "usage: %s <in.bin>\n", argv[0]);
    return 1;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f)
  {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 1;
  }
  const auto h = arr<int64_t>(f, 3);
  const auto s = arr<double>(f, 4);
  const size_t nk = h[0] > 0 ? (size_t)h[0] : 0, npts = (size_t)h[2];
  const auto temp = arr<double>(f, h[1] ? nk : 0), factor = arr<double>(f, h[1] ? nk : 0);
  const auto T = arr<double>(f, npts), D = arr<double>(f, npts);
  fclose(f);

  fus::ThermalResponse R;
  R.nknots = -7, R.phi_max = -7.0;
  const int err = fus::thermal_response_check((int)h[0], h[1] ? temp.data() : nullptr, h[1] ? factor.data() : nullptr, s[0],
                                              s[1], &R);
  printf("err %d\n", err);
  if (err != fus::TRS_OK)
    printf("untouched %d message %s\n", R.nknots == -7 && R.phi_max == -7.0 ? 1 : 0, fus::thermal_response_message(err));
  else
  {
    printf("active %d nknots %d phi_max %a\n", R.active() ? 1 : 0, R.nknots, R.phi_max);
    for (size_t i = 0; i < npts; ++i)
      printf("V %a %a\n", fus::thermal_response_P(R, T[i]), fus::thermal_response_S(R, D[i]));
  }
  fus::ThermalDamage G;
  G.A = -7.0;
  const int derr = fus::thermal_damage_check(s[2], s[3], &G);
  printf("derr %d\n", derr);
  if (derr != fus::TRS_OK)
    printf("untouched %d message %s\n", G.A == -7.0 ? 1 : 0, fus::thermal_response_message(derr));
  else
  {
    printf("on %d lnA %a\n", G.on() ? 1 : 0, G.lnA);
    for (size_t i = 0; G.on() && i < npts; ++i)
      printf("R %a\n", fus::thermal_damage_rate(G.lnA, G.Ea, T[i]));
  }
  return 0;
}
