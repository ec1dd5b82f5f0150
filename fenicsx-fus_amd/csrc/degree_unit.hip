// degree_unit.hip -- the launches whose template arguments hold the polynomial degree: the block kernel k_block_op and
// the per-point geometry kernels.  Compiled once per degree and scalar type (-DFUS_TU_DEGREE=k -DFUS_TU_DTYPE=64|32,
// build.py); fusmi.hip reaches a unit through the three entries of its DegreeImpl (host.hpp).
#include <algorithm>
#include <atomic>
#include <limits>
#include <mutex>
#include <tuple>

#include "host.hpp"

using namespace fus;

template <typename T, int P, int OP, int ATOMIC, int STAGE, int NF, int GEOM, int TD = 3, int MF = 0, int PK = 0>
static int launch_block_op_v(fus_op* op, const T* geo, const T* coef, const T* x, T* bvec,
                             const StageArgs<T>& S, int blk_begin, int blk_count)
{
  if (blk_count <= 0)
    return FUS_OK;
  constexpr int N = P + 1;
  KArgs<T, N> K;
  for (int i = 0; i < N * N; ++i)
    K.Dk.d[i] = (T)op->D[i], K.Dk.dt[i] = (T)op->D[(i % N) * N + i / N];

  for (int i = 0; i < N; ++i)
    K.Dk.w[i] = (T)op->wts[i], K.Dk.x[i] = (T)op->nodes[i];
  // the attribute is per device: one bit per device and instantiation (set again harmlessly if two
  // threads race on the first launch)
  // WALK = 1, the kernel with the block loop, runs where a launch can have fewer workgroups than blocks (option
  // "walk", below); every other launch of a per-cell geometry kernel runs the straight-line kernel WALK = 0
  constexpr bool CAN_WALK = GEOM != GEOM_STREAM && TD == 3;
  // The streamed-geometry kernels (quadrilaterals among them) keep the kernel with the block loop for every launch:
  // the straight-line form measured 0.45 % slower there in every round (profiles/block_overhead.md section 6)
#ifdef FUS_PROBE_WALK_ALWAYS   // developer probe (A/B of the straight-line kernel): every launch runs the kernel with the block loop
  constexpr int W0 = 1;
#else
  constexpr int W0 = CAN_WALK ? 0 : 1;
#endif
  const void* const k_straight = reinterpret_cast<const void*>(&k_block_op<T, P, OP, ATOMIC, STAGE, NF, GEOM, TD, MF, PK, W0>);
  const void* const k_walking = reinterpret_cast<const void*>(&k_block_op<T, P, OP, ATOMIC, STAGE, NF, GEOM, TD, MF, PK, CAN_WALK ? 1 : W0>);
  static std::atomic<uint64_t> attr_set{0};
  const uint64_t dev_bit = 1ull << (op->ctx->device & 63);
  if (!(attr_set.load(std::memory_order_relaxed) & dev_bit))
  {
    HIPCHK(hipFuncSetAttribute(k_straight, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (k_walking != k_straight)
      HIPCHK(hipFuncSetAttribute(k_walking, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set.fetch_or(dev_bit, std::memory_order_relaxed);
  }
  K.A = op->A;
  if (GEOM == GEOM_DIAG)
  {
    // the 1-D stiffness matrix K1 = D^T diag(w) D takes the derivative table's place (symmetric: d = dt)
    for (int q = 0; q < N; ++q)
      for (int i = 0; i < N; ++i)
      {
        double acc = 0;
        for (int m = 0; m < N; ++m)
          acc += op->D[m * N + q] * op->wts[m] * op->D[m * N + i];
        K.Dk.d[q * N + i] = K.Dk.dt[q * N + i] = (T)acc;
      }
  }
  K.A.blk_begin = blk_begin;
  K.A.blk_count = blk_count;
  K.Dg = static_cast<const T*>(op->d_Dg), K.geo = geo, K.coef = coef, K.x = x, K.bvec = bvec;
  K.partial = static_cast<T*>(op->d_partial);
  K.S = S;
  // option "walk" = w > 0: w workgroups per CU, each walking every (w * CUs)-th block of the range with
  // the next block's prologue loads in flight under the current block's epilogue (per-cell geometry
  // kernels; the streamed-geometry kernel keeps one workgroup per block).  Off by default: measured on
  // MI355X (config 2, profiles/r02_experiments.md) one workgroup per block is 13-17 % faster -- the
  // hardware's own dispatch of a fresh workgroup into a freed slot overlaps the phases of different
  // blocks better than the walking workgroup's software pipeline does.
  int grid = blk_count;
  if (CAN_WALK && op->ctx->walk != 0)
  {
    int per_cu = op->ctx->walk;
    if (per_cu < 0)  // as many workgroups per CU as are resident at once, where each then has >= 4 blocks to walk
    {
      // resident workgroups per CU of this instantiation, per (device, waves per workgroup, LDS bytes)
      static std::mutex occ_mu;
      static std::map<std::tuple<int, int, size_t>, int> occ_cache;
      int occ = 0;
      {
        std::lock_guard<std::mutex> lk(occ_mu);
        const auto key = std::make_tuple(op->ctx->device, op->L.waves, op->lds_bytes);
        auto it = occ_cache.find(key);
        if (it == occ_cache.end())
        {
          int nb = 0;
          HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
              &nb, k_walking, 64 * op->L.waves, op->lds_bytes));
          it = occ_cache.emplace(key, std::max(nb, 1)).first;
        }
        occ = it->second;
      }
      per_cu = (blk_count >= 4 * occ * op->ctx->num_cus) ? occ : 0;
    }
    if (per_cu > 0)
      grid = std::min(blk_count, per_cu * op->ctx->num_cus);
  }
  // (block_variant.hpp: the kernel with the block loop also where a block of the layout is larger than the first
  // batches of a straight-line kernel that has no leftover loops)
  if (CAN_WALK && block_walk(op->facts, op->traits, BlockVariant{GEOM, TD, ATOMIC, MF, PK}, NF, grid < blk_count))
    hipLaunchKernelGGL((k_block_op<T, P, OP, ATOMIC, STAGE, NF, GEOM, TD, MF, PK, CAN_WALK ? 1 : W0>), dim3(grid),
                       dim3(64 * op->L.waves), op->lds_bytes, op->ctx->stream, K);
  else
    hipLaunchKernelGGL((k_block_op<T, P, OP, ATOMIC, STAGE, NF, GEOM, TD, MF, PK, W0>), dim3(grid),
                       dim3(64 * op->L.waves), op->lds_bytes, op->ctx->stream, K);
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

// Blocks [blk_begin, blk_begin + blk_count) of the layout; blk_count < 0: all blocks.
template <typename T, int P, int OP, int STAGE, int NF = 1>
static int launch_block_op(fus_op* op, const T* geo, const T* coef, const T* x, T* bvec,
                           const StageArgs<T>& S, int blk_begin = 0, int blk_count = -1)
{
  if (NF > op->nfields)
    return fail(FUS_ERR_STATE, "operator data was not created for two-field models (option fields=2)");
  if (blk_count < 0)
    blk_count = op->L.nblocks - blk_begin;
  // which kernel (block_variant.hpp), then the five integers as template arguments: of the keys only those whose
  // kernel exists for <T, P, OP, STAGE> are compiled in
  const BlockVariant v = block_variant(op->facts, op->traits, OP, STAGE);
  const T* g = v.geom == GEOM_STREAM ? geo : static_cast<const T*>(op->d_Gc);   // streamed per-point arrays or per-cell factors
  constexpr int NO_KERNEL = std::numeric_limits<int>::min();
  const int r = with_kind(block_variant_key(v), [&](auto K) -> int
  {
    constexpr BlockVariant V = block_variant_of_key(decltype(K)::value);
    if constexpr (block_variant_exists(P, sizeof(T), OP, STAGE, V))
      return launch_block_op_v<T, P, OP, V.atomic, STAGE, NF, V.geom, V.td, V.mf, V.pk>(op, g, coef, x, bvec, S, blk_begin, blk_count);
    else
      return NO_KERNEL;
  }, std::make_integer_sequence<int, block_variant_nkeys>{});
  return r != NO_KERNEL ? r : fail(FUS_ERR_STATE, "this library holds no block kernel for the variant asked for");
}

// -------------------------------------------------------------------------------------------------
// the unit's DegreeImpl
// -------------------------------------------------------------------------------------------------
using T = std::conditional_t<FUS_TU_DTYPE == 64, double, float>;
constexpr int P = FUS_TU_DEGREE, N = P + 1;

// (op_kind, stage, nf) as one integer and back; a triple out of range is -1, the key of no kernel
constexpr int triple_key(int op_kind, int stage, int nf)
{
  return (op_kind < 0 || op_kind > 1 || stage < STAGE_NONE || stage > STAGE_LEAN3 || nf < 1 || nf > 2)
             ? -1
             : (op_kind * 16 + stage + 1) * 4 + nf;
}
constexpr int key_op(int k) { return k / 64; }
constexpr int key_stage(int k) { return k / 4 % 16 - 1; }
constexpr int key_nf(int k) { return k % 4; }

template <int... STAGES>
static int block_op_kinds(fus_op* op, int op_kind, int stage, int nf, const void* geo, const void* coef, const void* x,
                          void* b, const void* S, int b0, int nb, std::integer_sequence<int, STAGES...>)
{
  return with_kind<triple_key(OP_STIFFNESS, STAGE_NONE, 1), triple_key(OP_MASS, STAGE_NONE, 1),
                   triple_key(OP_STIFFNESS, STAGES, 1)..., triple_key(OP_STIFFNESS, STAGES, 2)...>(
      triple_key(op_kind, stage, nf), [&](auto K) -> int
      {
        constexpr int k = decltype(K)::value;
        return launch_block_op<T, P, key_op(k), key_stage(k), key_nf(k)>(
            op, static_cast<const T*>(geo), static_cast<const T*>(coef), static_cast<const T*>(x), static_cast<T*>(b),
            *static_cast<const StageArgs<T>*>(S), b0, nb);
      });
}
static int block_op(fus_op* op, int op_kind, int stage, int nf, const void* geo, const void* coef, const void* x, void* b,
                    const void* S, int b0, int nb)
{
  return block_op_kinds(op, op_kind, stage, nf, geo, coef, x, b, S, b0, nb, std::integer_sequence<int, FUS_STAGE_KINDS>{});
}

// Per-point geometry factors in the streaming layouts (precompute.hpp:101-213, 33-94), computed on the device
static int stream_geometry(fus_op* op)
{
  auto launch = [&](auto kernel) -> int
  {
    hipLaunchKernelGGL(kernel, dim3(nblk(op->ncells * op->Nd)), dim3(256), 0, op->ctx->stream,
                       op->ncells, op->d_cell_perm, static_cast<const T*>(op->d_xg), op->d_xdm,
                       static_cast<const double*>(op->d_pts), static_cast<const double*>(op->d_wts),
                       static_cast<T*>(op->d_G), static_cast<T*>(op->d_detJ));
    HIPCHK(hipGetLastError());
    return FUS_OK;
  };
  if (op->tdim == 2)
    return op->geom_order == 1 ? launch(&k_geometry2d<T, N, 1>) : launch(&k_geometry2d<T, N, 2>);
  return op->geom_order == 1 ? launch(&k_geometry<T, N, 1>) : launch(&k_geometry<T, N, 2>);
}

static int export_geometry(fus_op* op, void* dG, void* dd)
{
  hipLaunchKernelGGL((op->tdim == 2 ? &k_geometry_export2d<T, N> : &k_geometry_export<T, N>),
                     dim3(nblk(op->ncells * op->Nd)), dim3(256), 0, op->ctx->stream, op->ncells, op->d_cell_perm,
                     static_cast<const T*>(op->d_G), static_cast<const T*>(op->d_detJ), static_cast<T*>(dG), static_cast<T*>(dd));
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

FUS_HIDDEN const DegreeImpl* FUS_DEGREE_IMPL_FN(FUS_TU_DEGREE, FUS_TU_DTYPE)()
{
  static const DegreeImpl d = {&block_op, &stream_geometry, &export_geometry};
  return &d;
}

#ifndef FUS_TRACE_BITS
#define FUS_TRACE_BITS 64   // scalar type whose unit exports the trace (-DFUS_TRACE_BITS=32 for the fp32 kernels)
#endif
#if defined(FUS_TRACE) && FUS_TU_DTYPE == FUS_TRACE_BITS
// experiment builds: phase timestamps of the last k_block_op launch of this degree's unit
extern "C" int fus_debug_trace(unsigned long long* out, long long nblocks)
{
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(fus::g_fus_trace), (size_t)nblocks * 8 * sizeof(unsigned long long))
                 == hipSuccess
             ? 0
             : -2;
}
#endif
