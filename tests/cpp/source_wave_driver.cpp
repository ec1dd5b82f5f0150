// Host driver for csrc/source_wave.hpp (tests/test_source_host.py): the header is plain C++, so this file is built
// with the host compiler alone, once plainly and once under AddressSanitizer + UBSan.
//   source_wave_driver f p0 s0 scale D a in.bin   ->   one line "g dg" (%.17g) per local time s in in.bin (doubles);
//   exit code 2 when the duration is refused (0 < D < 2 Lr), nothing printed then.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "source_wave.hpp"

int main(int argc, char** argv)
{
  if (argc != 8)
  {
    std::fprintf(stderr, "usage: %s f p0 s0 scale D a in.bin\n", argv[0]);
    return 1;
  }
  const double f = std::atof(argv[1]), p0 = std::atof(argv[2]), s0 = std::atof(argv[3]), scale = std::atof(argv[4]),
               D = std::atof(argv[5]), a = std::atof(argv[6]);
  if (!fus::source_duration_ok(f, D))
    return 2;
  std::FILE* in = std::fopen(argv[7], "rb");
  if (!in)
    return 1;
  std::vector<double> s;
  double x;
  while (std::fread(&x, sizeof x, 1, in) == 1)
    s.push_back(x);
  std::fclose(in);
  const fus::SourceWave W = fus::source_wave_make(f, p0, s0, scale, D);
  for (double si : s)
  {
    double g, dg;
    fus::source_wave(W, a, si, &g, &dg);
    std::printf("%.17g %.17g\n", g, dg);
  }
  return 0;
}
