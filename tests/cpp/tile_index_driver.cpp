// tile_index_driver.cpp -- checks the exchange-tile image (csrc/tile_index.hpp) and the LDS reservation that goes with
// it on the host; built by tests/test_tile_index_host.py with -fsanitize=address,undefined.  For every N = 2..8 and both
// scalar types: the image is injective over a slot and stays inside tile_slot_entries; Layout::lds_bytes covers the
// block kernel's carve (the mirror of kernels.hpp FUS_PHASE_LDS below) for blocks of the default size and for
// one-element blocks.  fp64 at N = 5: the bank model (csrc/tile_bank_model.hpp) gives the linear image of 130-entry
// slots 50 read and 85 store cycles per 15 accesses, and the image in use no more.
// Prints "ok ..." and returns 0, or the first failure and 1.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "layout.hpp"
#include "tile_bank_model.hpp"

static int fail(const char* what, int N, int bytes, long a = 0, long b = 0)
{
  printf("FAIL %s N=%d bytes=%d (%ld, %ld)\n", what, N, bytes, a, b);
  return 1;
}

// end of the block kernel's LDS carve (kernels.hpp FUS_PHASE_LDS): x_l, y_l (fp64), x2_l, tiles, derivative table,
// coefficients, per-cell geometry, weights + points, local dofmaps, round table
static size_t kernel_carve(const fus::Layout& L, size_t T, int NF, int GCS)
{
  const int N = L.N, Nd = L.Nd;
  const size_t lds_nloc = (size_t)((L.max_nloc + 1) & ~1), lds_nelem = (size_t)((L.max_nelem + 7) & ~7);
  size_t off = lds_nloc * T;                                                    // x_l
  off += lds_nloc * 8;                                                          // y_l
  off += (NF == 2 ? lds_nloc : 0) * T;                                          // x2_l
  off += (size_t)L.slots * fus::tile_slot_entries(N, (int)T, L.tdim) * T;       // tiles
  off += (size_t)N * N * T;                                                     // D_l
  off += lds_nelem * T * NF;                                                    // cf_l (, cf2_l)
  off += (size_t)GCS * lds_nelem * T;                                           // gc_l
  off += (GCS ? (size_t)(N <= 8 ? 16 : 24) : 0) * T;                            // w_l, pt_l
  off += lds_nelem * Nd * 2;                                                    // ldm_l
  off += (size_t)L.max_rounds * L.slots * 2;                                    // rt_l
  return off;
}

static int check_lds(int P, int bytes, int n, int be, int waves)
{
  const int N = P + 1, Nd = N * N * N, G = n * P + 1;
  std::vector<int32_t> dm((size_t)n * n * n * Nd);
  std::vector<double> cen((size_t)n * n * n * 3);
  for (int ez = 0, e = 0; ez < n; ++ez)
    for (int ey = 0; ey < n; ++ey)
      for (int ex = 0; ex < n; ++ex, ++e)
      {
        cen[3 * e] = ex + 0.5, cen[3 * e + 1] = ey + 0.5, cen[3 * e + 2] = ez + 0.5;
        for (int a = 0; a < N; ++a)
          for (int b = 0; b < N; ++b)
            for (int c = 0; c < N; ++c)
              dm[(size_t)e * Nd + (a * N + b) * N + c] = ((ex * P + a) * G + (ey * P + b)) * G + (ez * P + c);
      }
  fus::Layout L;
  const std::string err = fus::build_layout(L, P, (int64_t)n * n * n, (int64_t)G * G * G, dm.data(), cen.data(), be, waves);
  if (!err.empty())
  {
    printf("FAIL build_layout P=%d be=%d: %s\n", P, be, err.c_str());
    return 1;
  }
  for (int NF = 1; NF <= 2; ++NF)
    for (int GCS : {0, 7, 21})
    {
      const size_t have = L.lds_bytes((size_t)bytes, NF, GCS), need = kernel_carve(L, (size_t)bytes, NF, GCS);
      if (have < need)
        return fail("lds_bytes < carve", N, bytes, (long)have, (long)need);
    }
  return 0;
}

int main()
{
  int checked = 0;
  for (int N = 2; N <= 8; ++N)
    for (int bytes : {4, 8})
    {
      const int TS = fus::tile_plane_stride(N, bytes), S = fus::tile_slot_entries(N, bytes, 3);
      std::set<int> seen;
      for (int i0 = 0; i0 < N; ++i0)
        for (int i1 = 0; i1 < N; ++i1)
          for (int i2 = 0; i2 < N; ++i2)
          {
            const int e = fus::tile_index(N, TS, i0, i1, i2);
            if (e < 0 || e >= S)
              return fail("entry outside the slot", N, bytes, e, S);
            if (!seen.insert(e).second)
              return fail("image not injective", N, bytes, e);
          }
      if (fus::tile_slot_entries(N, bytes, 2) < N * N)
        return fail("2-D slot too small", N, bytes);
      // every lane belongs to one slot and column; the slots of a wave do not overlap
      for (int lane = 0; lane < 64; ++lane)
      {
        const fus::TileLane t = fus::tile_lane(N, lane);
        if (t.s * N * N + t.b * N + t.c != lane || t.b >= N || t.c >= N)
          return fail("lane map", N, bytes, lane);
      }
      // default block sizes of the per-cell geometry paths (fusmi.hip) and one-element blocks, on a 4^3 (3^3) mesh
      const int P = N - 1;
      const int be = P == 1 ? 64 : P == 2 ? 64 : P == 3 ? 32 : P == 4 ? 32 : 8, waves = P == 4 ? 8 : 4;
      const int n = P <= 4 ? 4 : 3;
      if (check_lds(P, bytes, n, be, waves) || check_lds(P, bytes, n, 1, waves) || check_lds(P, bytes, n, 17, 4))
        return 1;
      ++checked;
    }
  // fp64, N = 5: the model's figures for the linear image of 130-entry slots, and the image in use against them
  {
    const fus::LdsForm rd = fus::lds_read_single(8), st = fus::lds_store_or_paired(8);
    auto linear = [](int i0, int i1, int i2) { return i0 * 25 + i1 * 5 + i2; };
    const int r0 = fus::tile_pattern_set_cycles(5, 8, 130, linear, rd), s0 = fus::tile_pattern_set_cycles(5, 8, 130, linear, st);
    if (r0 != 50 || s0 != 85)
      return fail("model of the linear image", 5, 8, r0, s0);
    const int TS = fus::tile_plane_stride(5, 8), S = fus::tile_slot_entries(5, 8, 3);
    auto used = [TS](int i0, int i1, int i2) { return fus::tile_index(5, TS, i0, i1, i2); };
    const int r1 = fus::tile_pattern_set_cycles(5, 8, S, used, rd), s1 = fus::tile_pattern_set_cycles(5, 8, S, used, st);
    if (r1 > 50 || s1 > 85)
      return fail("image in use costs more than the linear one", 5, 8, r1, s1);
    if (fus::tile_trip_cycles(5, 8, S, used, rd, st) > fus::tile_trip_cycles(5, 8, 130, linear, rd, st))
      return fail("trip cycles", 5, 8);
    printf("ok checked=%d read15=%d store15=%d trip=%d slot=%d\n", checked, r1, s1,
           fus::tile_trip_cycles(5, 8, S, used, rd, st), S);
  }
  return 0;
}
