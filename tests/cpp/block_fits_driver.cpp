// Stand-alone driver of the host decision "does every block fit the first batches of the straight-line block kernel"
// (csrc/block_variant.hpp: block_caps, block_fits, op_traits_fit, block_walk; tests/test_block_fits_host.py builds it
// plainly and with AddressSanitizer + UBSan and runs it on the CPU).
//
// First one line per (P, gcs, nf) with the capacities the header holds -- the numbers k_block_op sizes its batches by:
//   caps P gcs nf : ui us ul gc gc_all cf epi
// then, for every (P, gcs, nthr), the extents around every capacity edge -- each limit at zero, exactly fitting and one
// over while the others fit comfortably, then all of them exactly fitting at once -- one line each:
//   case P gcs nthr max_nint max_nsh max_nelem nd : fits1 fits2 traits_fits : walk1 walk2 walk1_short walk_stream
// walk<nf>: block_walk for a trilinear / affine fp64 variant with nf inputs; _short: with fewer workgroups than blocks;
// _stream: the streamed-geometry variant.
#include "block_variant.hpp"

#include <cstdio>
#include <initializer_list>

using namespace fus;

static void line(int P, int gcs, const BlockExtents& e)
{
  OpFacts f{P, 8, 3, 1, gcs == 7 ? GEOM_AFFINE : GEOM_TRILINEAR, false, false, -1, -1, 0};
  OpTraits t = op_traits(f);
  t.gcs = gcs;   // (0: not an operator's value; the function itself is still total)
  op_traits_fit(t, P, e);
  const BlockVariant v = block_variant(f, t, OP_STIFFNESS, STAGE_LEAN1);
  const BlockVariant vs{GEOM_STREAM, 3, 1, 0, 0};
  printf("case %d %d %d %d %d %d %d : %d %d %d : %d %d %d %d\n", P, gcs, e.nthr, e.max_nint, e.max_nsh, e.max_nelem, e.nd,
         (int)block_fits(P, gcs, 1, e), (int)block_fits(P, gcs, 2, e), t.fits, block_walk(f, t, v, 1, false),
         block_walk(f, t, v, 2, false), block_walk(f, t, v, 1, true), block_walk(f, t, vs, 1, false));
}

int main()
{
  static_assert(straight_needs_fit(4, 8, GEOM_TRILINEAR) && straight_needs_fit(2, 8, GEOM_AFFINE) && straight_needs_fit(3, 8, GEOM_DIAG)
                    && !straight_needs_fit(5, 8, GEOM_TRILINEAR) && !straight_needs_fit(4, 4, GEOM_TRILINEAR)
                    && !straight_needs_fit(4, 8, GEOM_STREAM),
                "the kernels without leftover loops: fp64, per-cell geometry, degrees <= 4");
  for (int P = 2; P <= 10; ++P)
    for (int gcs : {0, 7, 21})
      for (int nf : {1, 2})
      {
        const BlockCaps c = block_caps(P, gcs, nf);
        printf("caps %d %d %d : %d %d %d %d %d %d %d\n", P, gcs, nf, c.ui, c.us, c.ul, c.gc, (int)c.gc_all, c.cf, c.epi);
      }
  for (int P = 2; P <= 4; ++P)
    for (int gcs : {0, 7, 21})
      for (int nthr : {64, 256, 512})
      {
        const BlockCaps c1 = block_caps(P, gcs, 1), c2 = block_caps(P, gcs, 2);
        const int nd = (P + 1) * (P + 1) * (P + 1);
        // the largest values that fit, per limit (nf = 1: the two-range stage update is the tighter interior limit)
        const int vec1 = (c1.epi && c1.epi < c1.ui ? c1.epi : c1.ui) * nthr, vec2 = c2.ui * nthr;
        const int sh = c1.us * nthr;
        const int ne_gc = (gcs && c1.gc_all) ? c1.gc * nthr / gcs : c1.cf * nthr;
        const int ne_cf = c1.cf * nthr;
        const BlockExtents base{nthr, 8, 8, 1, 1};
        line(P, gcs, base);
        // interior dofs: around the nf = 1 edge and around the nf = 2 edge (an odd count has the same 16-byte vectors)
        for (int nv : {0, vec1, vec1 + 1, vec2, vec2 + 1})
          for (int odd : {0, 1})
          {
            BlockExtents e = base;
            e.max_nint = 2 * nv + odd;
            line(P, gcs, e);
          }
        for (int n : {0, sh, sh + 1})
        {
          BlockExtents e = base;
          e.max_nsh = n;
          line(P, gcs, e);
        }
        // elements against the geometry numbers and against the coefficients (one node per element keeps the dofmap small)
        for (int n : {0, ne_gc, ne_gc + 1, ne_cf, ne_cf + 1})
        {
          BlockExtents e = base;
          e.max_nelem = n;
          line(P, gcs, e);
        }
        // local dofmaps: one element of 8 k nodes has k 16-byte vectors
        for (int k : {0, c1.ul * nthr, c1.ul * nthr + 1})
        {
          BlockExtents e = base;
          e.nd = 8 * k - (k > c1.ul * nthr ? 7 : 0);   // one node past the edge is one vector more
          line(P, gcs, e);
        }
        // a real element size, elements up to the dofmap's edge
        for (int n : {c1.ul * nthr * 8 / nd, c1.ul * nthr * 8 / nd + 1})
        {
          BlockExtents e = base;
          e.nd = nd, e.max_nelem = n;
          line(P, gcs, e);
        }
        // everything exactly fitting at once (the element count by its tightest limit), nf = 1 and nf = 2
        for (int vec : {vec1, vec2})
        {
          BlockExtents e{nthr, 2 * vec + 1, sh, ne_gc < ne_cf ? ne_gc : ne_cf, 1};
          line(P, gcs, e);
        }
        // too few threads for the derivative table
        line(P, gcs, BlockExtents{32, 8, 8, 1, 1});
        line(P, gcs, BlockExtents{0, 0, 0, 0, 1});
      }
  return 0;
}
