// Host driver for csrc/thermal_bc.hpp (tests/test_thermal_bc_host.py): the header is plain C++, so this file is built
// with the host compiler alone, under AddressSanitizer + UBSan.
//   thermal_bc_driver <in.bin>
//   in.bin:  int64 ndofs, bits (32 | 64), has_fixed, has_fixed_rise, has_conv_diag, has_conv_rise;  int32 dof_perm[ndofs];
//            then the arrays that are present, in that order: uint8 fixed[ndofs], T fixed_rise, conv_diag, conv_rise [ndofs]
//   out:     "err E" (the header's error code); for E = 0 then "nfix F nconv C", F lines "F idx val" and C lines
//            "C idx hw r" in list order, values as hexadecimal floats.  The lists are filled with a sentinel before the
//            call, so that an error that touched them would show.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "thermal_bc.hpp"

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

template <typename T>
int run(FILE* f, const std::vector<int64_t>& h)
{
  const int64_t n = h[0];
  const auto perm = arr<int32_t>(f, (size_t)n);
  const auto fixed = arr<uint8_t>(f, h[2] ? (size_t)n : 0);
  const auto rise = arr<T>(f, h[3] ? (size_t)n : 0);
  const auto diag = arr<T>(f, h[4] ? (size_t)n : 0);
  const auto ext = arr<T>(f, h[5] ? (size_t)n : 0);
  fus::ThermalBcLists<T> L;
  L.fix_idx.assign(1, -7), L.conv_idx.assign(1, -7);
  const int err = fus::thermal_bc_lists<T>(n, perm.data(), h[2] ? fixed.data() : nullptr, h[3] ? rise.data() : nullptr,
                                           h[4] ? diag.data() : nullptr, h[5] ? ext.data() : nullptr, &L);
  printf("err %d\n", err);
  if (err != fus::TBC_OK)
  {
    const bool untouched = L.fix_idx.size() == 1 && L.fix_idx[0] == -7 && L.conv_idx.size() == 1 && L.conv_idx[0] == -7
                           && L.fix_val.empty() && L.hw.empty() && L.r.empty();
    printf("untouched %d message %s\n", untouched ? 1 : 0, fus::thermal_bc_message(err));
    return 0;
  }
  printf("nfix %zu nconv %zu\n", L.fix_idx.size(), L.conv_idx.size());
  if (L.fix_val.size() != L.fix_idx.size() || L.hw.size() != L.conv_idx.size() || L.r.size() != L.conv_idx.size())
    return 3;
  for (size_t k = 0; k < L.fix_idx.size(); ++k)
    printf("F %d %a\n", (int)L.fix_idx[k], (double)L.fix_val[k]);
  for (size_t k = 0; k < L.conv_idx.size(); ++k)
    printf("C %d %a %a\n", (int)L.conv_idx[k], (double)L.hw[k], (double)L.r[k]);
  return 0;
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
  const auto h = arr<int64_t>(f, 6);
  const int rc = h[1] == 64 ? run<double>(f, h) : run<float>(f, h);
  fclose(f);
  return rc;
}
