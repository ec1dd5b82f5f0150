// host.hpp -- what all translation units of libfusmi share on the host: the units compiled once (fusmi.hip: the
// operator and its C ABI; wave.hip: the wave models; thermal.hip: the bioheat model -- the three add core.hpp) and
// degree_unit.hip (compiled once per polynomial degree and scalar type, so that the k_block_op instantiations of the
// degrees compile in parallel: build.py).  The seam between those units and the degree units is DegreeImpl below.
#ifndef FUS_HOST_HPP
#define FUS_HOST_HPP

#include "../../include/fusmi.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "block_variant.hpp"
#include "kernels.hpp"
#include "layout.hpp"

// -------------------------------------------------------------------------------------------------
// errors
// -------------------------------------------------------------------------------------------------
#define FUS_HIDDEN __attribute__((visibility("hidden")))
extern FUS_HIDDEN thread_local std::string g_err;   // defined in fusmi.hip
static int fail(int code, const std::string& msg)
{
  g_err = msg;
  return code;
}
#define HIPCHK(expr)                                                                               \
  do                                                                                               \
  {                                                                                                \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(FUS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
  } while (0)
#define FUSCHK(expr)                                                                               \
  do                                                                                               \
  {                                                                                                \
    int r_ = (expr);                                                                               \
    if (r_ != FUS_OK)                                                                              \
      return r_;                                                                                   \
  } while (0)

// -------------------------------------------------------------------------------------------------
// handles
// -------------------------------------------------------------------------------------------------
struct Prof
{
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  double done_ms = 0;
  int64_t done_count = 0;
  int64_t seen = 0;   // scopes of this name since fus_profile_enable (level 2 samples every prof_sample-th)
};

struct fus_ctx
{
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t comm_stream = nullptr;            // RCCL exchange, overlapped with local shared dofs
  hipEvent_t ev_packed = nullptr, ev_recv = nullptr;
  int deterministic = 0;  // 1: conflict-free rounds (bitwise reproducible); 0: LDS atomics
  int fields = 1;         // operator inputs per block pass the ops are sized for (2: Lossy)
  int graph = 0;          // 1: replay the RK step as one hipGraph (launch-bound sizes)
  int geometry = 0;       // 0: auto (affine cells: 7 numbers per cell; other first-order hexahedra: the
                          // cell's trilinear map, G recomputed per point; else streamed), 1: always
                          // stream G, 2: as auto without the affine shortcut
  // 0 = auto: 32 elements / 4 waves when G is streamed, 16 / 4 on the affine path (measured best
  // on MI355X at p=4 fp64, profiles/r01_block_sweep.txt)
  int block_elems = 0, waves = 0;
  int prof = 0;  // 0 off, 1 all scopes, 2 block-operator kernel only
  int prof_sample = 1;  // level 2: events around every prof_sample-th launch of the block-operator kernel (option "profile_sample")
  std::map<std::string, Prof> profs;
  ncclComm_t comm = nullptr;
  int rank = 0, nranks = 1;
  bool local_group = false;  // in-process transport (single-GPU rehearsal of the multi-rank path)
  // timing rehearsal of the RCCL exchange on one GPU (option "halo_loopback"): the context keeps its
  // logical (rank, nranks) but owns a 1-rank communicator and every send / receive goes to itself,
  // so a middle slab exercises pack -> ncclSend/ncclRecv -> ordered unpack with realistic launch
  // and synchronisation cost (the received planes are its own: results are NOT the physical ones)
  bool loopback = false;
  bool overlap_blocks = false;  // launch interface blocks first, overlap the exchange with the rest
  bool external_transport = false;  // the caller exchanges the packed interface values (e.g. GPU-aware MPI)
  int num_cus = 256;                // hipDeviceProp_t::multiProcessorCount
  // Lossy / Westervelt boundary forms: 0 = the C++ benchmarks (BM7-SC1/forms.py:37-42: absorbing and
  // delta-mass terms on every boundary facet, source doubled, Lossy.hpp:216-220); 1 = the Python
  // package (python/src/fenicsxfus/_lossy.py:107-128, :186-189: those terms on tag 2 only, source
  // not doubled)
  int forms = 0;
  // classical RK4 without the redundant accumulator streams (stage kinds 4-6, kernels.hpp): 1 (default);
  // 0 keeps u_, v_ in HBM at every stage like Linear.hpp:282-294
  int lean_rk4 = 1;
  // index-1 / index-2 contractions of the degrees 6 and 7 on the matrix cores (per-cell geometry kernels):
  // -1 auto (the measured choice per degree, scalar type and geometry), 0 never, 1 wherever a variant exists
  int mfma = -1;
  int pack32 = -1;  // fp32, degrees 5-7, per-cell geometry: two elements per wave in packed float2 (-1 auto, 0, 1)
  // shared-dof stage kernel reads the partial sums as planes at the dof's own index (1, default) or through the
  // shared-dof CSR (0; also taken when a dof has more than FUS_MAX_PLANES = 16 sharing blocks, wave_kernels.hpp): same sums, same order
  int planes = 1;
  // affine meshes whose cells have mutually orthogonal edges (boxes): the stiffness action in its diagonal-metric
  // form (three 1-D stiffness contractions, kernels.hpp elem_compute) -- 1 (default) where the mesh allows, 0 never
  int diag_metric = 1;
  int walk = 0;   // block-kernel workgroups per CU that walk several blocks each (0: one workgroup per block --
                  // the measured best everywhere so far; -1: as many as are resident), see launch_block_op_v
  int rayleigh_chunks = 0;   // source chunks of fus_rayleigh (rayleigh.hip): 0 = as many as fill the device, else forced
};

struct Neigh
{
  int rank;
  int64_t count;
  int64_t off;  // first entry of this neighbour in the send / receive buffers
};

struct fus_op
{
  fus_ctx* ctx;
  int P, N, Nd, dtype;
  int tdim = 3;  // 3: hexahedra, 2: quadrilaterals (Nd = N^tdim)
  size_t ts;  // sizeof(T)
  int64_t ncells, ndofs, nnodes;
  fus::Layout L;
  std::vector<double> nodes, wts, D;
  std::vector<char> h_geom_x;        // caller geometry (host copy, T)
  std::vector<int32_t> h_geom_dm;    // [ncells*geom_nv]
  int geom_order = 1, geom_nv = 8;   // 1: 2^tdim vertices; 2: 27 nodes in tensor order (hexahedra)
  std::vector<int32_t> h_dofmap;     // caller tensor dofmap
  // device
  fus::BlockArgs A{};
  std::vector<void*> allocs;
  int32_t *d_cell_perm = nullptr, *d_dof_perm = nullptr;
  int64_t *d_sh_ptr = nullptr, *d_sh_pairs = nullptr;
  void *d_G = nullptr, *d_detJ = nullptr, *d_Dg = nullptr, *d_partial = nullptr;
  void *d_tmp_x = nullptr, *d_tmp_b = nullptr, *d_tmp_c = nullptr, *d_tmp_coef = nullptr;
  size_t lds_bytes = 0;
  int deterministic = 0;
  int nfields = 1;
  // what decides the block kernel's variant (block_variant.hpp).  op_build fills both with the geometry mode it predicts
  // (facts.mode; facts.ortho is found there); op_setup_device puts in the mode the device confirmed -- GEOM_AFFINE: per-cell
  // factors in d_Gc, streamed G / detJ built only on demand; GEOM_TRILINEAR: d_Gc holds 21 map coefficients per cell --
  // and settles traits.mfma and traits.diag; traits.pk stays what the layout was built with
  fus::OpFacts facts{};
  fus::OpTraits traits{};
  void* d_Gc = nullptr;
  void *d_xg = nullptr, *d_pts = nullptr, *d_wts = nullptr;
  int32_t* d_xdm = nullptr;
  // neighbours (multi-GPU)
  std::vector<Neigh> neigh;
  // halo buffers: concatenated neighbour lists (ascending rank), one send and one receive buffer;
  // unique interface dofs with, per dof, its addends in ascending rank order (-1 = own partial)
  int64_t n_halo = 0, n_uidx = 0;
  int32_t *d_pack_idx = nullptr, *d_uidx = nullptr, *d_uptr = nullptr, *d_usrc = nullptr;
  void *d_sendbuf = nullptr, *d_recvbuf = nullptr;
  // the pseudo partial slots (next-stage boundary terms of shared boundary dofs) live in d_partial,
  // i.e. per op, while several models may share one op: the model that wrote them last
  const struct fus_model* bnd_owner = nullptr;
  // gradient / pair-product kernel (gradient.hip), allocated on its first use (all in allocs): the component sums in internal
  // numbering T[tdim][n_internal], the partial planes of the shared dofs T[tdim][n_partial], the lumped M(1) 1,
  // 16 rows of per-cell coefficients, and the inputs in internal numbering (d_grad_in only grows)
  void *d_grad_y = nullptr, *d_grad_part = nullptr, *d_grad_den = nullptr, *d_grad_coef = nullptr, *d_grad_in = nullptr;
  size_t grad_in_bytes = 0;
};

// -------------------------------------------------------------------------------------------------
// small helpers
// -------------------------------------------------------------------------------------------------
static inline unsigned nblk(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

// A run-time integer as a template argument: f(std::integral_constant<int, K>{}) for the K of the list that equals
// `kind`; f returns a status.  A kind outside the list is an error, never some other kernel.
template <int... Ks, typename F>
static int with_kind(int kind, F&& f)
{
  int r = FUS_OK;
  if (((kind == Ks && ((r = f(std::integral_constant<int, Ks>{})), true)) || ...))
    return r;
  return fail(FUS_ERR_STATE, "no kernel variant of kind " + std::to_string(kind));
}
template <typename F, int... Ks>
static int with_kind(int kind, F&& f, std::integer_sequence<int, Ks...>)
{
  return with_kind<Ks...>(kind, f);
}

// every kind stage_kind (wave.hip) returns: the instantiations of the stage kernels
#define FUS_STAGE_KINDS                                                                            \
  fus::STAGE_FIRST, fus::STAGE_MID, fus::STAGE_LAST, fus::STAGE_LEAN0, fus::STAGE_LEAN1, fus::STAGE_LEAN2, fus::STAGE_LEAN3

// -------------------------------------------------------------------------------------------------
// the degree units: everything whose template arguments hold the polynomial degree
// -------------------------------------------------------------------------------------------------
struct DegreeImpl
{
  // blocks [b0, b0 + nb) of the layout (nb < 0: all from b0) through k_block_op<T, P, op_kind, ., stage, nf, ...>, the
  // variant chosen by block_variant.hpp; S points to a StageArgs<T>.  The triples a unit holds: (OP_STIFFNESS, STAGE_NONE, 1),
  // (OP_MASS, STAGE_NONE, 1) and (OP_STIFFNESS, k, 1 | 2) for the k of FUS_STAGE_KINDS; any other is FUS_ERR_STATE
  int (*block_op)(fus_op*, int op_kind, int stage, int nf, const void* geo, const void* coef, const void* x, void* b,
                  const void* S, int b0, int nb);
  int (*stream_geometry)(fus_op*);   // writes op->d_G / op->d_detJ (allocated by the caller)
  int (*export_geometry)(fus_op*, void* dG, void* dd);   // op->d_G / op->d_detJ in caller cell order (either may be null)
};
// the hidden factory of the unit of degree k and scalar type f<bits>: fus_degree_impl_<k>_f64 | _f32
#define FUS_CAT_(a, b) a##b
#define FUS_CAT(a, b) FUS_CAT_(a, b)
#define FUS_DEGREE_IMPL_FN(k, bits) FUS_CAT(FUS_CAT(FUS_CAT(fus_degree_impl_, k), _f), bits)

#endif
