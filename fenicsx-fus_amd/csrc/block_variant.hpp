// Which instantiation of the block kernel k_block_op (kernels.hpp) runs for an operator: the one place where that is
// decided.  Plain C++: no HIP header is needed, a host program may include this file
// (tests/cpp/block_variant_driver.cpp prints both functions over their whole input space).
//
// The decision has two steps.
//   op_traits(facts)                        per operator, at set-up: which kernel families the operator uses at all
//                                           (matrix-core, packed fp32, diagonal metric) and the per-cell geometry count
//   block_variant(facts, traits, OP, STAGE) per launch: the template arguments (GEOM, TD, ATOMIC, MF, PK) of the kernel
// op_build (fusmi.hip) calls op_traits with the geometry mode it predicts on the host, because the packed kernel's two
// exchange-tile slots and the LDS budget shape the layout; op_setup_device calls it again with the mode the device
// confirmed and with the layout's `pk` as given, then op_traits_fit with the layout's largest block; block_walk() turns
// that and the launch's grid into the kernel's WALK argument.  block_variant_exists() names the instantiations a library holds: the
// launch dispatcher compiles exactly those, and block_variant() returns no other.
#ifndef FUS_BLOCK_VARIANT_HPP
#define FUS_BLOCK_VARIANT_HPP

namespace fus
{
// operator of the block kernel (template parameter OP)
enum
{
  OP_STIFFNESS = 0,
  OP_MASS = 1
};

// Geometry source of the block operator (template parameter GEOM)
//   GEOM_STREAM: per-point factors G / detJw streamed from HBM (any trilinear mesh; the reference's
//                data path, precompute.hpp:101-213)
//   GEOM_AFFINE: every cell is a parallelepiped (J constant per cell): 6 + 1 numbers per CELL,
//                G(q) = Gc * w_q and detJw(q) = detc * w_q rebuilt in registers
//   GEOM_TRILINEAR: any first-order hexahedron: 21 numbers per CELL (the coefficients of the trilinear
//                map without its constant), J(q) and from it G(q) / detJw(q) recomputed per point
//                in registers (the formulas of geom.hpp); trades the 6 N^3 streamed numbers per
//                cell for ~65 flops per point
// The first three are also the geometry MODE of an operator (OpFacts::mode, fus_op_geometry_mode).
enum
{
  GEOM_STREAM = 0,
  GEOM_AFFINE = 1,
  GEOM_TRILINEAR = 2,
  // GEOM_AFFINE data on cells with mutually orthogonal edges (J^T J diagonal): the stiffness action in its
  // diagonal-metric form (elem_compute); everything else as GEOM_AFFINE
  GEOM_DIAG = 3
};

// Fused stage-update variants (template parameter STAGE of the block and shared-dof kernels; what each one computes:
// kernels.hpp, StageArgs).  There is no kind 2.
enum
{
  STAGE_NONE = -1,   // plain operator action: b / partial slab are written, no update
  STAGE_FIRST = 0,   // first stage, accumulators u_, v_ kept in HBM (Runge-Kutta orders 1-3, option "lean_rk4" = 0)
  STAGE_MID = 1,     // middle stage of those schemes
  STAGE_LAST = 3,    // last stage of RK4 in that form
  STAGE_LEAN0 = 4,   // stages 0-3 of the classical RK4 without accumulators
  STAGE_LEAN1 = 5,
  STAGE_LEAN2 = 6,
  STAGE_LEAN3 = 7
};

// N = 8, fp64: index-1 contractions on the matrix cores straight from the registers (kernels.hpp, mf4_contract_b)
#ifndef FUS_MF4
#define FUS_MF4 1
#endif
// ... in the trilinear kernel, where it measured +5 ... +7 % (the general affine kernel and the diagonal-metric form were
// even: profiles/r03_experiments.md section 6); not in the MF variant, which has its own 16x16x4 form
constexpr bool uses_mf4(int N, int scalar_bytes, int geom, int mf)
{
  return N == 8 && scalar_bytes == 8 && FUS_MF4 && geom == GEOM_TRILINEAR && !mf;
}

// What the decision rests on
struct OpFacts
{
  int P;              // polynomial degree
  int scalar_bytes;   // 8: fp64, 4: fp32
  int tdim;           // 3: hexahedra, 2: quadrilaterals
  int geom_order;     // 1: 2^tdim vertices per cell, 2: second-order geometry
  int mode;           // GEOM_STREAM, GEOM_AFFINE or GEOM_TRILINEAR: predicted on the host or confirmed by the device
  bool ortho;         // every cell a parallelepiped with mutually orthogonal edges
  bool deterministic; // conflict-free rounds instead of LDS atomics
  int opt_mfma;       // option "mfma": -1 auto, 0 never, 1 wherever a variant exists
  int opt_pack32;     // option "pack32": -1 auto, 0, 1
  int opt_diag_metric;// option "diag_metric": 0, 1
};

struct OpTraits
{
  bool mfma;  // MFMA contraction variants of the block kernel in use (degrees 6, 7)
  bool pk;    // packed fp32 variants in use (degrees 5-7: two elements per wave, layout slots doubled)
  bool diag;  // GEOM_AFFINE in its diagonal-metric form
  int gcs;    // per-cell geometry numbers the block keeps in LDS: 7 (affine), 21 (trilinear), 0 (streamed)
  int fits = 0;   // bit nf - 1: every block of the layout fits the first batches of the kernels with nf operator
                  // inputs (block_fits below; op_traits_fit sets it once the layout exists)
};

// ---- what one thread of the block kernel moves in its unrolled first batches (kernels.hpp, k_block_op) ----
// first-batch prologue registers per thread at p = 7 (interior vectors) and at the degrees 8-10 (interior vectors, shared dofs)
#ifndef FUS_UI_P7
#define FUS_UI_P7 5
#endif
#ifndef FUS_UI_HI
#define FUS_UI_HI 7
#endif
// The one definition of these capacities: the kernel sizes its batches by them, and the host decides by them
// (block_fits) whether a layout may run the kernels that have no loop for what is left over.
struct BlockCaps
{
  int ui;    // 16-byte interior vectors of the operator input
  int us;    // shared dofs (gathered values in the prologue, partial sums in the epilogue)
  int ul;    // 16-byte vectors of the local dofmaps
  int gc;    // per-cell geometry numbers
  bool gc_all;   // ... which are all of a block's (degree 4); false: the kernel keeps the loop for the rest -- the default
                 // blocks of the degrees 2 and 3 (64 and 32 elements on 256 threads) hold more than two batches of them
  int cf;    // cell coefficients
  int epi;   // 16-byte interior ranges of the fused stage update in its two-range form (degrees <= 4, one operator
             // input); 0: the kernel has another form, whose loop stays
};
constexpr BlockCaps block_caps(int P, int gcs, int nf)
{
  return {(P <= 3) ? 3 : ((P == 4) ? 2 : (P <= 6 ? 4 : (P == 7 ? FUS_UI_P7 : FUS_UI_HI))),
          (P <= 3) ? 4 : ((P == 4) ? 3 : (P <= 7 ? 5 : FUS_UI_HI)),
          (P <= 3) ? 2 : ((P == 4) ? 1 : 4),
          gcs > 7 ? 2 : 1,
          P == 4,
          1,
          (P <= 4 && nf == 1) ? 2 : 0};
}

// The kernels whose one-block form (WALK = 0) is compiled without leftover loops: fp64, per-cell geometry, degrees <= 4
// (the kernels with range-checked accesses, k_block_op RANGED_FITS)
constexpr bool straight_needs_fit(int P, int scalar_bytes, int geom)
{
  return geom != GEOM_STREAM && scalar_bytes == 8 && P <= 4;
}

// The largest block of a layout, and the threads of a workgroup
struct BlockExtents
{
  int nthr;        // threads per workgroup (64 x waves)
  int max_nint;    // interior dofs
  int max_nsh;     // shared dofs (nloc - nint)
  int max_nelem;   // elements
  int nd;          // nodes per element
};

// Every block fits the first batches: nothing is left for a loop
constexpr bool block_fits(int P, int gcs, int nf, const BlockExtents& e)
{
  const BlockCaps c = block_caps(P, gcs, nf);
  const long long nthr = e.nthr, nvec = e.max_nint >> 1, n16 = ((long long)e.max_nelem * e.nd * 2 + 15) >> 4;
  return nthr > 0 && nvec <= c.ui * nthr && e.max_nsh <= c.us * nthr && n16 <= c.ul * nthr
         && (!c.gc_all || (long long)e.max_nelem * gcs <= c.gc * nthr) && e.max_nelem <= c.cf * nthr && (c.epi == 0 || nvec <= c.epi * nthr)
         && (P + 1) * (P + 3) <= nthr;   // the derivative table with the 1-D weights and points: one entry per thread
}

// once the layout exists (op_setup_device)
inline void op_traits_fit(OpTraits& t, int P, const BlockExtents& e)
{
  t.fits = (block_fits(P, t.gcs, 1, e) ? 1 : 0) | (block_fits(P, t.gcs, 2, e) ? 2 : 0);
}

// template arguments of k_block_op beside <T, P, OP, STAGE, NF>
struct BlockVariant
{
  int geom, td, atomic, mf, pk;
};

// Measured choice (MI355X, profiles/r02_experiments.md sections 5 and 15) between the vector and the matrix-core
// form of the index-1 / index-2 contractions.
constexpr bool mfma_default(int P, bool f64, bool affine)
{
  // Nowhere at present.  Degree 7, fp64, trilinear geometry was the one case where the matrix-core form won
  // (-5.8 % against the tile-read vector form); with the re-mapped vector contractions at N = 8 (derivative-table
  // rows by scalar loads) the vector form is 2.7 % ahead: 1.423 against 1.469 ms per launch at 64^3.  Affine
  // geometry at degree 7 (+6 %: little vector work to relieve) and fp32 at degree 6 (+45 %: the f32 MFMA issues
  // at the vector-FMA rate) were slower from the start.  Option "mfma" = 1 still selects the variants.
  (void)P, (void)f64, (void)affine;
  return false;
}

// layout_pk < 0: decide `pk` from the facts (before build_layout).  0 / 1: the layout was built without / with the packed
// kernel's second exchange-tile slot -- a fact by then, taken as given.
inline OpTraits op_traits(const OpFacts& f, int layout_pk = -1)
{
  const bool affine = f.mode == GEOM_AFFINE, percell = f.mode != GEOM_STREAM;
  OpTraits t;
  // matrix-core contraction variants: degrees 6 and 7 on the per-cell geometry paths; "auto" follows the
  // A/B measurements on MI355X (profiles/r02_mfma.md)
  t.mfma = (f.P == 6 || f.P == 7) && percell && !f.deterministic
           && (f.opt_mfma == 1 || (f.opt_mfma < 0 && mfma_default(f.P, f.scalar_bytes == 8, affine)));
  // diagonal-metric form of the affine kernel: scalar kernels of the degrees <= 7 (no packed / matrix-core variant)
  const bool diag_mesh = f.ortho && f.opt_diag_metric && f.P <= 7 && !(f.opt_mfma == 1) && !(f.opt_pack32 == 1);
  // packed fp32 kernels (two elements per wave): degrees 5-7, per-cell geometry, LDS atomics, MFMA variants off
  // "auto" = where it measured faster on MI355X (profiles/r02_experiments.md section 7): degree 5 (+4 %) and degree 6
  // on affine cells (+2 %); slower at degree 6 trilinear (-12 %: 137 registers, three waves per SIMD) and degree 7
  t.pk = layout_pk >= 0
             ? layout_pk != 0
             : f.scalar_bytes == 4 && f.tdim == 3 && f.P >= 5 && f.P <= 7 && percell && !f.deterministic && f.opt_mfma != 1
                   && (f.opt_pack32 == 1 || (f.opt_pack32 < 0 && !diag_mesh && (f.P == 5 || (f.P == 6 && affine))));
  t.diag = affine && f.ortho && f.opt_diag_metric && f.P <= 7 && !t.mfma && !t.pk;
  t.gcs = affine ? 7 : (percell ? 21 : 0);
  return t;
}

// The kernel of one launch.  Quadrilaterals and the degrees 8-10 (two waves per element, kernels.hpp elem_compute_hi) have
// the mode's plain kernel only; below, the first of MF, PK, DIAG that the traits and the operator allow, else the plain one.
inline BlockVariant block_variant(const OpFacts& f, const OpTraits& t, int op, int stage)
{
  const int atomic = f.deterministic ? 0 : 1;
  if (f.tdim == 2)   // streamed geometry only
    return {GEOM_STREAM, 2, atomic, 0, 0};
  const bool percell = f.mode != GEOM_STREAM, stiffness = op == OP_STIFFNESS;
  if (f.P <= 7)
  {
    // degrees 6 and 7, per-cell geometry, LDS-atomic accumulation: the index-1 / index-2 contractions on the
    // matrix cores (kernels.hpp, elem_compute_mfma); the variants exist for the stiffness operator as the plain action
    // and as the last / lean RK4 stages -- the mass action and the stage kinds 0-2 run the scalar kernel
    if ((f.P == 6 || f.P == 7) && stiffness && (stage == STAGE_NONE || stage >= 3) && t.mfma && !f.deterministic && percell)
      return {f.mode, 3, 1, 1, 0};
    // fp32, degrees 5-7, per-cell geometry, LDS-atomic accumulation: two elements per wave in packed float2
    // (kernels.hpp, elem_compute_pk); stiffness operator only (the mass action runs through the scalar kernel)
    if (f.scalar_bytes == 4 && f.P >= 5 && stiffness && t.pk && !t.mfma && !f.deterministic && percell)
      return {f.mode, 3, 1, 0, 1};
    // cells with orthogonal edges: diagonal-metric form of the stiffness action
    if (stiffness && f.mode == GEOM_AFFINE && t.diag)
      return {GEOM_DIAG, 3, atomic, 0, 0};
  }
  return {f.mode, 3, atomic, 0, 0};
}

// The template argument WALK of the variant's kernel for one launch with nf operator inputs.  1: the kernel with the
// block loop and every leftover loop -- the only form of the streamed-geometry kernels, the form of a launch with
// fewer workgroups than blocks (option "walk"), and the form of a layout with a block larger than the first batches of
// a kernel whose one-block form has no leftover loops.  0: straight-line code for one block.
inline int block_walk(const OpFacts& f, const OpTraits& t, const BlockVariant& v, int nf, bool fewer_groups_than_blocks)
{
  if (v.geom == GEOM_STREAM || v.td != 3 || fewer_groups_than_blocks)
    return 1;
  if (straight_needs_fit(f.P, f.scalar_bytes, v.geom) && !((t.fits >> (nf - 1)) & 1))
    return 1;
  return 0;
}

// The instantiations k_block_op<T, P, OP, ATOMIC, STAGE, NF, GEOM, TD, MF, PK> a library holds, for any NF
constexpr bool block_variant_exists(int P, int scalar_bytes, int op, int stage, const BlockVariant& v)
{
  if (v.td != 3)
    return v.td == 2 && v.geom == GEOM_STREAM && !v.mf && !v.pk;
  const bool percell = v.geom == GEOM_AFFINE || v.geom == GEOM_TRILINEAR, stiffness = op == OP_STIFFNESS;
  if (v.mf)
    return (P == 6 || P == 7) && stiffness && (stage == STAGE_NONE || stage >= 3) && v.atomic && !v.pk && percell;
  if (v.pk)
    return scalar_bytes == 4 && P >= 5 && P <= 7 && stiffness && v.atomic && percell;
  if (v.geom == GEOM_DIAG)
    return stiffness && P <= 7;
  return v.geom == GEOM_STREAM || percell;
}

// A variant as one small integer and back, so that a single switch over the keys turns it into template arguments
constexpr int block_variant_nkeys = 64;
constexpr int block_variant_key(const BlockVariant& v)
{
  return v.geom | (v.td == 2 ? 4 : 0) | (v.atomic ? 8 : 0) | (v.mf ? 16 : 0) | (v.pk ? 32 : 0);
}
constexpr BlockVariant block_variant_of_key(int k)
{
  return {k & 3, (k & 4) ? 2 : 3, (k >> 3) & 1, (k >> 4) & 1, (k >> 5) & 1};
}
} // namespace fus

#endif
