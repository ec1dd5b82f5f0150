// Host driver for csrc/sts_coef.hpp (tests/test_sts_host.py): the header is plain C++, so this file is built with the
// host compiler alone, under AddressSanitizer + UBSan.
//   sts_coef_driver lo hi   ->   for every stage count s in lo..hi one line "s j mu nu mut gat beta" (hexadecimal
//   floats) per stage j = 1..s; exit code 2 at the first s the header refuses, nothing printed for it.
#include <cstdio>
#include <cstdlib>

#include "sts_coef.hpp"

int main(int argc, char** argv)
{
  if (argc != 3)
  {
    std::fprintf(stderr, "usage: %s lo hi\n", argv[0]);
    return 1;
  }
  const int lo = std::atoi(argv[1]), hi = std::atoi(argv[2]);
  for (int s = lo; s <= hi; ++s)
  {
    fus::StsCoef c;
    if (!fus::sts_coefficients(s, &c))
      return 2;
    for (int j = 1; j <= c.s; ++j)
      std::printf("%d %d %a %a %a %a %a\n", s, j, c.mu[j], c.nu[j], c.mut[j], c.gat[j], fus::sts_beta(s));
  }
  return 0;
}
