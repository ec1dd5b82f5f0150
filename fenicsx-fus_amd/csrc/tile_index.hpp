// tile_index.hpp -- where an entry of an element's exchange tile lives in LDS (the re-mapped contractions of
// kernels.hpp elem_compute), as plain constexpr functions without device types: the kernels, Layout::lds_bytes and the
// host-side bank model (tile_bank_model.hpp) all read the image from here.
//
// The tile of an element with N points per direction is read and written by lane (b, c) as (a, b, c) for every a (the
// lane's own column), as (b, k, c) for every k (index 1 along the lane's registers) and as (b, c, k) for every k
// (index 2 along them).  Lane N^2 s + N b + c of a wave works on the wave's element slot s (64 / N^2 slots per wave,
// at least one; the lanes beyond the last slot are idle).
//
// Image: planes of tile_plane_stride entries, rows of N, except N = 8 (XOR swizzle, no padding).  N = 4: one entry of
// padding per plane; fp32 at N = 7: planes of 56 (63 -> 56 bank-conflict cycles per element over the three read
// patterns, by enumeration; ideal 42).  N = 8: with a linear image two of the three patterns put the 32 lanes of an LDS
// lane group on 4-8 banks (42 % of the LDS cycles of the p=7 kernels were bank conflicts,
// profiles/r02_p7_remap_counters.json); XOR-ing index 1 with the low bits of index 0 and index 2 with index 1 makes all
// three conflict free.  fp64 at N = 5: the linear image costs 50 read and 85 store cycles per 15 accesses under the
// bank model; what was searched and what it gave is in profiles/lds_trips.md.
#pragma once

namespace fus
{

constexpr int tile_plane_stride(int N, int scalar_bytes)
{
  return (N == 8 || N == 4) ? N * N + 1 : ((N == 7 && scalar_bytes == 4) ? 56 : N * N);
}

// entries reserved per element slot (tdim = 2: quadrilaterals, one plane)
constexpr int tile_slot_entries(int N, int scalar_bytes, int tdim)
{
  return (tdim == 3 && N == 7 && scalar_bytes == 4) ? N * 56 : (tdim == 3 ? N * N * N : N * N) + N;
}

// entry (i0, i1, i2) of a slot; TS = tile_plane_stride
constexpr int tile_index(int N, int TS, int i0, int i1, int i2)
{
  return N == 8 ? i0 * 64 + ((i1 ^ (i0 & 3)) << 3) + (i2 ^ i1) : i0 * TS + i1 * N + i2;
}

// lane -> element slot of the wave and tensor column (s >= slots per wave: idle lane)
struct TileLane
{
  int s, b, c;
};
constexpr TileLane tile_lane(int N, int lane)
{
  return TileLane{lane / (N * N), (lane % (N * N)) / N, lane % N};
}
constexpr int tile_slots_per_wave(int N) { return 64 / (N * N) > 0 ? 64 / (N * N) : 1; }

}   // namespace fus
