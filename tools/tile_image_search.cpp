// Search for an image of the fp64 exchange tile at N = 5 with fewer modelled LDS-array cycles per element trip
// (csrc/tile_bank_model.hpp; host only, no GPU):
//   entry(i0, i1, i2) = i0 TS + ((i1 + r10 i0) mod 5) RS + ((i2 + r21 i1 + r20 i0) mod 5),  slots of S entries,
// plane strides TS = 25..40, row strides RS = 5..8, rotations 0..4, S up to 190 (two blocks of 32 elements per CU: at
// most 80 KB of LDS per block, 72.5 KB with S = 130).  Prints the image in use, the best padded image without a
// rotation and the best images with one (profiles/lds_trips.md, Part 2).
//   g++ -std=c++17 -O2 -I fenicsx-fus_amd/csrc tools/tile_image_search.cpp -o tools/_bin/tile_image_search
#include <cstdio>
#include <set>
#include <vector>

#include "tile_bank_model.hpp"

struct Cand
{
  int TS, RS, r10, r21, r20, S;
  int operator()(int i0, int i1, int i2) const
  {
    return i0 * TS + ((i1 + r10 * i0) % 5) * RS + ((i2 + r21 * i1 + r20 * i0) % 5);
  }
};

static bool injective(const Cand& c)
{
  std::set<int> seen;
  for (int i0 = 0; i0 < 5; ++i0)
    for (int i1 = 0; i1 < 5; ++i1)
      for (int i2 = 0; i2 < 5; ++i2)
      {
        const int e = c(i0, i1, i2);
        if (e >= c.S || !seen.insert(e).second)
          return false;
      }
  return true;
}

static void report(const char* what, const Cand& c)
{
  const fus::LdsForm rd = fus::lds_read_single(8), st = fus::lds_store_or_paired(8);
  printf("%-28s TS %2d RS %d rot(i1+=%d i0, i2+=%d i1+%d i0) S %3d: reads %2d stores %2d per 15, trip %3d (paired reads %3d)\n",
         what, c.TS, c.RS, c.r10, c.r21, c.r20, c.S, fus::tile_pattern_set_cycles(5, 8, c.S, c, rd),
         fus::tile_pattern_set_cycles(5, 8, c.S, c, st), fus::tile_trip_cycles(5, 8, c.S, c, rd, st),
         fus::tile_trip_cycles(5, 8, c.S, c, st, st));
}

int main()
{
  const fus::LdsForm rd = fus::lds_read_single(8), st = fus::lds_store_or_paired(8);
  const Cand now{fus::tile_plane_stride(5, 8), 5, 0, 0, 0, fus::tile_slot_entries(5, 8, 3)};
  report("in use", now);
  Cand best_pad = now, best_rot = now;
  int cyc_pad = fus::tile_trip_cycles(5, 8, now.S, now, rd, st), cyc_rot = cyc_pad;
  for (int TS = 25; TS <= 40; ++TS)
    for (int RS = 5; RS <= 8; ++RS)
      for (int r10 = 0; r10 < 5; ++r10)
        for (int r21 = 0; r21 < 5; ++r21)
          for (int r20 = 0; r20 < 5; ++r20)
            for (int S = 4 * TS + 4 * RS + 5; S <= 190; ++S)
            {
              const Cand c{TS, RS, r10, r21, r20, S};
              if (!injective(c))
                continue;
              const int cyc = fus::tile_trip_cycles(5, 8, S, c, rd, st);
              if (r10 == 0 && r21 == 0 && r20 == 0 && cyc < cyc_pad)
                cyc_pad = cyc, best_pad = c;
              if (cyc < cyc_rot)
                cyc_rot = cyc, best_rot = c;
            }
  report("best without a rotation", best_pad);
  report("best with rotations", best_rot);
  printf("ideal: reads 30 stores 60 per 15, trip %d\n", 40 * 2 + 35 * 4);
  return 0;
}
