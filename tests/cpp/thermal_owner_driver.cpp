// Stand-alone driver of csrc/thermal_owner.hpp (tests/test_thermal_multirank_host.py builds it with AddressSanitizer +
// UBSan and runs it on the CPU).  Input file: int64 nranks, then per rank int64 ndofs, int64 n_internal,
// int32 perm[ndofs] (internal index of the rank's DOF d) and int64 gid[ndofs] (its global DOF id).  For every rank the
// program builds the halo lists the way fus_op_set_neighbours documents them -- the neighbours in ascending rank order,
// a neighbour's shared DOFs ordered by global id, per interface DOF the addends in ascending rank order with -1 for the
// own value -- calls thermal_owner_mask and checks that over all ranks every global DOF is owned exactly once, and by
// the lowest rank that holds it.  Output: "ok <nglobal> <ninterface> <owned by rank 0> <owned by rank 1> ...", or
// "fail <what>"; then the header's answers to three malformed lists.
#include "thermal_owner.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

struct Rank
{
  int64_t ndofs = 0, n_internal = 0;
  std::vector<int32_t> perm;
  std::vector<int64_t> gid;
  std::vector<int32_t> uidx, uptr, usrc;
  std::vector<uint8_t> mask;
};

template <typename U>
static bool read_n(FILE* f, std::vector<U>& v, size_t n)
{
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(U), n, f) == n;
}

static void halo_lists(std::vector<Rank>& R, int r)
{
  Rank& me = R[r];
  std::map<int64_t, int32_t> mine;
  for (int64_t d = 0; d < me.ndofs; ++d)
    mine[me.gid[d]] = (int32_t)d;
  std::vector<int32_t> pack_idx;
  std::vector<std::pair<int, std::pair<int64_t, int64_t>>> neigh;   // rank, (offset, count)
  for (int q = 0; q < (int)R.size(); ++q)
  {
    if (q == r)
      continue;
    std::vector<int64_t> shared;
    for (int64_t g : R[q].gid)
      if (mine.count(g))
        shared.push_back(g);
    std::sort(shared.begin(), shared.end());
    if (shared.empty())
      continue;
    neigh.push_back({q, {(int64_t)pack_idx.size(), (int64_t)shared.size()}});
    for (int64_t g : shared)
      pack_idx.push_back(me.perm[mine[g]]);
  }
  me.uidx = pack_idx;
  std::sort(me.uidx.begin(), me.uidx.end());
  me.uidx.erase(std::unique(me.uidx.begin(), me.uidx.end()), me.uidx.end());
  std::vector<std::vector<int32_t>> add(me.uidx.size());
  bool own_done = false;
  for (auto& nb : neigh)
  {
    if (nb.first > r && !own_done)
    {
      for (auto& a : add)
        a.push_back(-1);
      own_done = true;
    }
    for (int64_t j = 0; j < nb.second.second; ++j)
    {
      const int32_t slot = (int32_t)(nb.second.first + j);
      const size_t u = std::lower_bound(me.uidx.begin(), me.uidx.end(), pack_idx[slot]) - me.uidx.begin();
      add[u].push_back(slot);
    }
  }
  if (!own_done)
    for (auto& a : add)
      a.push_back(-1);
  me.uptr.assign(1, 0);
  for (auto& a : add)
  {
    me.usrc.insert(me.usrc.end(), a.begin(), a.end());
    me.uptr.push_back((int32_t)me.usrc.size());
  }
}

int main(int argc, char** argv)
{
  if (argc != 2)
    return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f)
    return 2;
  int64_t nranks = 0;
  if (fread(&nranks, 8, 1, f) != 1 || nranks < 1 || nranks > 64)
    return 2;
  std::vector<Rank> R((size_t)nranks);
  for (auto& rk : R)
  {
    int64_t hd[2];
    if (fread(hd, 8, 2, f) != 2 || hd[0] < 0 || hd[1] < hd[0])
      return 2;
    rk.ndofs = hd[0], rk.n_internal = hd[1];
    if (!read_n(f, rk.perm, (size_t)rk.ndofs) || !read_n(f, rk.gid, (size_t)rk.ndofs))
      return 2;
  }
  fclose(f);
  std::map<int64_t, std::vector<int>> holders, owners;
  std::vector<int64_t> owned((size_t)nranks, 0);
  for (int r = 0; r < (int)nranks; ++r)
  {
    halo_lists(R, r);
    Rank& me = R[r];
    const int err = fus::thermal_owner_mask(me.n_internal, (int64_t)me.uidx.size(), me.uidx.data(), me.uptr.data(),
                                            me.usrc.data(), &me.mask);
    if (err != fus::TOWN_OK || (int64_t)me.mask.size() != me.n_internal)
      return printf("fail rank %d: error %d\n", r, err), 1;
    std::vector<uint8_t> used((size_t)me.n_internal, 0);
    for (int64_t d = 0; d < me.ndofs; ++d)
    {
      used[(size_t)me.perm[d]] = 1;
      holders[me.gid[d]].push_back(r);
      if (me.mask[(size_t)me.perm[d]])
        owners[me.gid[d]].push_back(r), ++owned[(size_t)r];
    }
    for (int64_t i = 0; i < me.n_internal; ++i)
      if (!used[(size_t)i] && me.mask[(size_t)i] != 1)
        return printf("fail rank %d: padding slot %lld masked\n", r, (long long)i), 1;
  }
  int64_t ninterface = 0;
  for (auto& kv : holders)
  {
    const std::vector<int>& own = owners[kv.first];
    if (own.size() != 1)
      return printf("fail dof %lld owned %zu times\n", (long long)kv.first, own.size()), 1;
    if (own[0] != *std::min_element(kv.second.begin(), kv.second.end()))
      return printf("fail dof %lld owned by rank %d, not by its lowest sharer\n", (long long)kv.first, own[0]), 1;
    ninterface += kv.second.size() > 1;
  }
  printf("ok %zu %lld", holders.size(), (long long)ninterface);
  for (int64_t o : owned)
    printf(" %lld", (long long)o);
  printf("\n");
  // malformed lists: an index past the vector, a list without the own value, an empty list; the mask stays untouched
  std::vector<uint8_t> keep(3, 7);
  const int32_t uidx_bad[1] = {5}, uidx_ok[1] = {2}, uptr1[2] = {0, 1}, uptr0[2] = {0, 0}, other[1] = {0}, self[1] = {-1};
  printf("errors %d %d %d %d\n", fus::thermal_owner_mask(4, 1, uidx_bad, uptr1, self, &keep),
         fus::thermal_owner_mask(4, 1, uidx_ok, uptr1, other, &keep), fus::thermal_owner_mask(4, 1, uidx_ok, uptr0, self, &keep),
         (int)(keep.size() == 3 && keep[0] == 7));
  return 0;
}
