// Stand-alone driver of csrc/block_variant.hpp (tests/test_block_variant_host.py builds it plainly and with
// AddressSanitizer + UBSan and runs it on the CPU).  It walks the whole input space of op_traits and block_variant the way
// fusmi.hip uses them: traits of the PREDICTED geometry mode first (op_build: pk and gcs shape the layout), then traits
// of the CONFIRMED mode with the layout's pk as given (op_setup_device), then the variant of every (OP, STAGE).  The
// predicted and the confirmed mode are equal, or one is affine and the other trilinear.
//
// One line per set of facts:
//   P bytes tdim order pred conf ortho det mfma pack32 diag_metric : pk gcs_pred : mfma diag gcs_conf : V V V ...
// with one V = geom,td,atomic,mf,pk,exists per (OP, STAGE), OP = stiffness, mass outermost, STAGE = -1 0 1 3 4 5 6 7.
#include "block_variant.hpp"

#include <cstdio>
#include <initializer_list>

int main()
{
  using namespace fus;
  const int modes[5][2] = {{GEOM_STREAM, GEOM_STREAM},       {GEOM_AFFINE, GEOM_AFFINE},   {GEOM_TRILINEAR, GEOM_TRILINEAR},
                           {GEOM_TRILINEAR, GEOM_AFFINE}, {GEOM_AFFINE, GEOM_TRILINEAR}};
  const int stages[8] = {STAGE_NONE,  STAGE_FIRST, STAGE_MID,   STAGE_LAST,
                         STAGE_LEAN0, STAGE_LEAN1, STAGE_LEAN2, STAGE_LEAN3};
  static_assert(STAGE_NONE == -1 && STAGE_FIRST == 0 && STAGE_MID == 1 && STAGE_LAST == 3 && STAGE_LEAN0 == 4 && STAGE_LEAN3 == 7,
                "the stage kinds are template arguments of compiled kernels");
  static_assert(uses_mf4(8, 8, GEOM_TRILINEAR, 0) == (FUS_MF4 != 0) && !uses_mf4(8, 8, GEOM_TRILINEAR, 1) && !uses_mf4(8, 4, GEOM_TRILINEAR, 0)
                    && !uses_mf4(7, 8, GEOM_TRILINEAR, 0) && !uses_mf4(8, 8, GEOM_AFFINE, 0),
                "uses_mf4");
  for (int P = 2; P <= 10; ++P)
    for (int bytes : {8, 4})
      for (int tdim : {2, 3})
        for (int order : {1, 2})
          for (const auto& md : modes)
            for (int ortho : {0, 1})
              for (int det : {0, 1})
                for (int mfma : {-1, 0, 1})
                  for (int pack32 : {-1, 0, 1})
                    for (int dm : {0, 1})
                    {
                      OpFacts f{P, bytes, tdim, order, md[0], ortho != 0, det != 0, mfma, pack32, dm};
                      const OpTraits pred = op_traits(f);
                      f.mode = md[1];
                      const OpTraits conf = op_traits(f, pred.pk);
                      if (conf.pk != pred.pk)
                        return printf("fail: the confirmed traits re-decided pk\n"), 1;
                      printf("%d %d %d %d %d %d %d %d %d %d %d : %d %d : %d %d %d :", P, bytes, tdim, order, md[0], md[1], ortho, det,
                             mfma, pack32, dm, (int)pred.pk, pred.gcs, (int)conf.mfma, (int)conf.diag, conf.gcs);
                      for (int op : {(int)OP_STIFFNESS, (int)OP_MASS})
                        for (int st : stages)
                        {
                          const BlockVariant v = block_variant(f, conf, op, st);
                          const BlockVariant back = block_variant_of_key(block_variant_key(v));
                          if (back.geom != v.geom || back.td != v.td || back.atomic != v.atomic || back.mf != v.mf || back.pk != v.pk
                              || block_variant_key(v) < 0 || block_variant_key(v) >= block_variant_nkeys)
                            return printf("fail: variant key does not round-trip\n"), 1;
                          printf(" %d,%d,%d,%d,%d,%d", v.geom, v.td, v.atomic, v.mf, v.pk, (int)block_variant_exists(P, bytes, op, st, v));
                        }
                      printf("\n");
                    }
  return 0;
}
