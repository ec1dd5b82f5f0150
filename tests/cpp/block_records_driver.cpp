// block_records_driver.cpp -- builds the host-side block layout (csrc/layout.cpp) on a dofmap read from a binary
// file and reports the per-block record table the device reads (Layout::blk_rec) beside the Layout vectors it was
// made from; built by tests/test_block_records_host.py with -fsanitize=address,undefined (and, without sanitizers,
// by tests/test_gpu_block_records.py for the facts its meshes must show).
// File: int64 {tdim, P, ncells, ndofs, block_elems, waves, nbnd}; int32 dofmap[ncells*Nd]; double centroids[ncells*3];
// int32 bnd[nbnd] (caller dofs that carry a boundary term).
// Writes <file>.rec (the record table, raw) and <file>.vec (int64 [nblocks][9]: elem_off, int_off, sh_off and the
// block's shape fields, read from the Layout vectors), prints one line of facts.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "layout.hpp"

int main(int argc, char** argv)
{
  if (argc != 2)
    return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f)
    return 2;
  int64_t h[7];
  if (fread(h, 8, 7, f) != 7)
    return 2;
  const int tdim = (int)h[0], P = (int)h[1], N = P + 1;
  const int64_t nc = h[2], nd = h[3], nbnd = h[6];
  const int Nd = tdim == 3 ? N * N * N : N * N;
  std::vector<int32_t> dm((size_t)nc * Nd), bnd((size_t)nbnd);
  std::vector<double> cen((size_t)nc * 3);
  if (fread(dm.data(), 4, dm.size(), f) != dm.size() || fread(cen.data(), 8, cen.size(), f) != cen.size()
      || (nbnd && fread(bnd.data(), 4, bnd.size(), f) != bnd.size()))
    return 2;
  fclose(f);
  fus::Layout L;
  std::string err = fus::build_layout(L, P, nc, nd, dm.data(), cen.data(), (int)h[4], (int)h[5], nullptr, tdim);
  if (err.empty())
    err = fus::verify_layout(L, dm.data());
  if (!err.empty())
  {
    printf("layout: %s\n", err.c_str());
    return 1;
  }
  if ((int64_t)L.blk_rec.size() != L.nblocks)
  {
    printf("record table has %zu entries for %d blocks\n", L.blk_rec.size(), L.nblocks);
    return 1;
  }
  std::vector<int64_t> vec((size_t)L.nblocks * 9);
  int64_t odd_int = 0, even_int = 0;
  for (int32_t b = 0; b < L.nblocks; ++b)
  {
    const fus::Layout::Shape& sh = L.shapes[L.blk_shape[b]];
    const int64_t row[9] = {L.blk_elem_off[b], L.blk_int_off[b], L.blk_sh_off[b], sh.nelem,     sh.nloc,
                            sh.nint,           sh.nrounds,       sh.rounds_off,   sh.ldm_off};
    for (int k = 0; k < 9; ++k)
      vec[(size_t)b * 9 + k] = row[k];
    (sh.nint & 1 ? odd_int : even_int) += 1;
  }
  // blocks with / without a boundary term on one of their interior dofs (what the fused epilogue branches on)
  std::vector<char> has(L.nblocks, 0);
  for (int64_t k = 0; k < nbnd; ++k)
  {
    const int32_t i = L.dof_perm[bnd[k]];
    if (i >= L.n_int_pad)
      continue;
    for (int32_t b = 0; b < L.nblocks; ++b)
      if (i >= L.blk_int_off[b] && i < L.blk_int_off[b] + L.shapes[L.blk_shape[b]].nint)
        has[b] = 1;
  }
  int64_t with_bnd = 0;
  for (char c : has)
    with_bnd += c;
  int64_t odd_planes = 0;
  for (int64_t c : L.plane_cnt)
    odd_planes += c & 1;
  const std::string base(argv[1]);
  FILE* fr = fopen((base + ".rec").c_str(), "wb");
  FILE* fv = fopen((base + ".vec").c_str(), "wb");
  if (!fr || !fv)
    return 2;
  fwrite(L.blk_rec.data(), sizeof(fus::BlockRecord), L.blk_rec.size(), fr);
  fwrite(vec.data(), 8, vec.size(), fv);
  fclose(fr), fclose(fv);
  printf("ok blocks=%d shapes=%zu interior=%lld shared=%lld pairs=%lld shared_local=%lld planes=%zu odd_planes=%lld "
         "odd_int=%lld even_int=%lld with_bnd=%lld without_bnd=%lld rec_size=%zu rec_base_mod64=%d\n",
         L.nblocks, L.shapes.size(), (long long)L.n_interior, (long long)L.n_shared, (long long)L.npairs,
         (long long)L.n_shared_local, L.plane_cnt.size(), (long long)odd_planes, (long long)odd_int,
         (long long)even_int, (long long)with_bnd, (long long)(L.nblocks - with_bnd), sizeof(fus::BlockRecord),
         (int)(reinterpret_cast<uintptr_t>(L.blk_rec.data()) % 64));
  return 0;
}
