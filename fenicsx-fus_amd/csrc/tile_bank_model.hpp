// tile_bank_model.hpp -- host-side model of the LDS-array cycles that the exchange tile's accesses take (one wave
// instruction of the re-mapped contractions, kernels.hpp elem_compute), for any image of the tile: the image in use
// (tile_index.hpp) and candidates for it (tools/tile_image_search.cpp).
//
// The LDS serves a wave instruction in fixed groups of consecutive lanes, one cycle per group when no two lanes of the
// group ask one bank for different addresses; a k-way conflict takes k cycles; lanes that read one address share it;
// idle lanes take no part.  The groups and the bank modulus depend on the instruction (gfx950):
//   ds_read_b64 / ds_read_b32                        2 groups of 32 lanes, 64 banks of 4 bytes (b32: 32 banks)
//   ds_write_b64, each half of ds_read2_b64          4 groups of 16 lanes, 32 banks of 4 bytes
// The probe (tools/lds_probe.hip, profiles/lds_trips.md Part 0) gives 0.92 of these cycles for the single reads and
// 0.6-0.8 for the stores and the paired reads at N = 5: the order of the forms and of the patterns is the model's.
#pragma once
#include <algorithm>
#include <map>
#include <set>

#include "tile_index.hpp"

namespace fus
{

struct LdsForm
{
  int group_lanes, banks;   // lanes per group, 4-byte banks
};
constexpr LdsForm lds_read_single(int scalar_bytes) { return LdsForm{32, scalar_bytes == 8 ? 64 : 32}; }
constexpr LdsForm lds_store_or_paired(int) { return LdsForm{16, 32}; }

enum TilePattern
{
  TILE_OWN = 0,   // (a, b, c): the lane's own column, a = k
  TILE_IDX1 = 1,  // (b, k, c)
  TILE_IDX2 = 2   // (b, c, k)
};

// cycles of one wave instruction: access k of the pattern by every active lane of a wave.  image(i0, i1, i2) -> entry
// of the slot, slot_entries apart for the wave's element slots.
template <class Image>
int tile_access_cycles(int N, int scalar_bytes, int slot_entries, const Image& image, TilePattern pat, int k, LdsForm f)
{
  const int epw = tile_slots_per_wave(N), words = scalar_bytes / 4;
  int cycles = 0;
  for (int g0 = 0; g0 < 64; g0 += f.group_lanes)
  {
    std::map<int, std::set<long>> per_bank;   // bank -> distinct 4-byte words asked of it
    for (int lane = g0; lane < g0 + f.group_lanes; ++lane)
    {
      const TileLane t = tile_lane(N, lane);
      if (t.s >= epw)
        continue;
      const int e = pat == TILE_OWN ? image(k, t.b, t.c) : (pat == TILE_IDX1 ? image(t.b, k, t.c) : image(t.b, t.c, k));
      const long word = ((long)t.s * slot_entries + e) * words;
      for (int w = 0; w < words; ++w)
        per_bank[(int)((word + w) % f.banks)].insert(word + w);
    }
    size_t worst = 1;   // a group costs its cycle whoever takes part
    for (const auto& kv : per_bank)
      worst = std::max(worst, kv.second.size());
    cycles += (int)worst;
  }
  return cycles;
}

// the 3 N accesses of one kind: every k of the three patterns
template <class Image>
int tile_pattern_set_cycles(int N, int scalar_bytes, int slot_entries, const Image& image, LdsForm f)
{
  int cycles = 0;
  for (int pat = 0; pat < 3; ++pat)
    for (int k = 0; k < N; ++k)
      cycles += tile_access_cycles(N, scalar_bytes, slot_entries, image, (TilePattern)pat, k, f);
  return cycles;
}

// one element trip of the re-mapped stiffness action: 8 N reads (4 N of the lane's own column, 2 N of each re-mapped
// pattern) and 7 N stores (3 N, 2 N, 2 N)
template <class Image>
int tile_trip_cycles(int N, int scalar_bytes, int slot_entries, const Image& image, LdsForm rd, LdsForm st)
{
  static const int reads[3] = {4, 2, 2}, stores[3] = {3, 2, 2};
  int cycles = 0;
  for (int pat = 0; pat < 3; ++pat)
    for (int k = 0; k < N; ++k)
      cycles += reads[pat] * tile_access_cycles(N, scalar_bytes, slot_entries, image, (TilePattern)pat, k, rd)
                + stores[pat] * tile_access_cycles(N, scalar_bytes, slot_entries, image, (TilePattern)pat, k, st);
  return cycles;
}

}   // namespace fus
