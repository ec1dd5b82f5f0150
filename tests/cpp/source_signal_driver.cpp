// Host driver for csrc/source_signal.hpp (tests/test_source_signal_host.py): the header is plain C++, so this file is
// built with the host compiler alone, once plainly and once under AddressSanitizer + UBSan.
//   source_signal_driver nchan nsamp t_first ds a table.bin chan.bin t.bin
//     table.bin  doubles, time-major [nsamp][nchan] (the device layout);  chan.bin  int32 channel per evaluation;
//     t.bin      doubles, one time per evaluation
//   ->   one line "g dg" (%.17g) per evaluation;  exit code 2 when (nsamp, t_first, ds) is refused, nothing printed then.
// The table is copied into an allocation of exactly nsamp * nchan doubles: a read outside it is the sanitizer's to find.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "source_signal.hpp"

template <typename U>
static bool read_all(const char* path, std::vector<U>& out)
{
  std::FILE* in = std::fopen(path, "rb");
  if (!in)
    return false;
  U x;
  while (std::fread(&x, sizeof x, 1, in) == 1)
    out.push_back(x);
  std::fclose(in);
  return true;
}

int main(int argc, char** argv)
{
  if (argc != 9)
  {
    std::fprintf(stderr, "usage: %s nchan nsamp t_first ds a table.bin chan.bin t.bin\n", argv[0]);
    return 1;
  }
  const int64_t nchan = std::atoll(argv[1]), nsamp = std::atoll(argv[2]);
  const double t_first = std::atof(argv[3]), ds = std::atof(argv[4]), a = std::atof(argv[5]);
  if (!fus::source_signal_ok(nsamp, t_first, ds))
    return 2;
  std::vector<double> table, t;
  std::vector<int32_t> chan;
  if (!read_all(argv[6], table) || !read_all(argv[7], chan) || !read_all(argv[8], t))
    return 1;
  if (nchan < 1 || (int64_t)table.size() != nchan * nsamp || chan.size() != t.size())
    return 1;
  double* exact = new double[table.size()];
  for (size_t i = 0; i < table.size(); ++i)
    exact[i] = table[i];
  const fus::SourceSignal P{t_first, ds, nsamp, nchan};
  for (size_t i = 0; i < t.size(); ++i)
  {
    if (chan[i] < 0 || chan[i] >= nchan)
    {
      delete[] exact;
      return 1;
    }
    double g, dg;
    fus::source_signal(P, exact, chan[i], a, t[i], &g, &dg);
    std::printf("%.17g %.17g\n", g, dg);
  }
  delete[] exact;
  return 0;
}
