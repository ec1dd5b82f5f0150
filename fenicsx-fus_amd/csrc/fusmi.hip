// fusmi.hip -- the operator of libfusmi (include/fusmi.h) and its C ABI: context and options, the RCCL binding and the
// fus_comm_* entries, the shared-DOF exchange, op_build / op_setup_device / op_apply and the fus_op_* entries, the
// dispatch over the degree units, the bandwidth probe and the profile entries.  The wave models (wave.hip) and the
// bioheat model (thermal.hip) are units of their own, which call into this one through core.hpp.
//
// Reference counterparts: StiffnessSpectral3D / MassSpectral3D (spectral_op.hpp:29-107, 132-284).  There is no CPU
// fallback in this file: every compute entry point needs the HIP device and fails with FUS_ERR_HIP without one.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "core.hpp"
#include "tables.hpp"

using namespace fus;

FUS_HIDDEN thread_local std::string g_err;   // the last error's text (fail, host.hpp), shared with the degree units
#define NCCLCHK(expr)                                                                              \
  do                                                                                               \
  {                                                                                                \
    ncclResult_t r_ = (expr);                                                                      \
    if (r_ != ncclSuccess)                                                                         \
      return fail(FUS_ERR_RCCL, std::string(#expr) + ": " + g_rccl.GetErrorString(r_));            \
  } while (0)

// -------------------------------------------------------------------------------------------------
// RCCL, bound at run time.  A host process may already carry an RCCL (PyTorch bundles its own
// librccl.so); binding to the resident copy instead of linking a second one keeps a single RCCL
// in the process.  Order: $FUSMI_RCCL (explicit path), an already loaded librccl, the system one.
// -------------------------------------------------------------------------------------------------
struct RcclApi
{
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
FUS_HIDDEN RcclApi g_rccl;

static int rccl_load()
{
  if (g_rccl.handle)
    return FUS_OK;
  void* h = nullptr;
  if (const char* path = getenv("FUSMI_RCCL"))
    h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
  for (const char* name : {"librccl.so.1", "librccl.so"})
    if (!h)
      h = dlopen(name, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
    if (!h)
      h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
  if (!h)
    return fail(FUS_ERR_RCCL, std::string("cannot load librccl: ") + dlerror());
  RcclApi a;
  a.handle = h;
#define FUS_SYM(field, name)                                                                       \
  *reinterpret_cast<void**>(&a.field) = dlsym(h, name);                                            \
  if (!a.field)                                                                                    \
    return fail(FUS_ERR_RCCL, "librccl lacks " name);
  FUS_SYM(GetUniqueId, "ncclGetUniqueId")
  FUS_SYM(CommInitRank, "ncclCommInitRank")
  FUS_SYM(CommDestroy, "ncclCommDestroy")
  FUS_SYM(Send, "ncclSend")
  FUS_SYM(Recv, "ncclRecv")
  FUS_SYM(GroupStart, "ncclGroupStart")
  FUS_SYM(GroupEnd, "ncclGroupEnd")
  FUS_SYM(AllReduce, "ncclAllReduce")
  FUS_SYM(GetErrorString, "ncclGetErrorString")
#undef FUS_SYM
  g_rccl = a;
  return FUS_OK;
}

// -------------------------------------------------------------------------------------------------
// typed implementation
// -------------------------------------------------------------------------------------------------
template <typename T>
static int shared_reduce(fus_op* op, T* bvec)
{
  if (op->L.n_shared > 0)
  {
    ProfScope ps(op->ctx, "shared");
    hipLaunchKernelGGL((k_shared_reduce<T, int64_t>), dim3(nblk(op->L.n_shared)), dim3(256), 0,
                       op->ctx->stream, (int64_t)0, op->L.n_shared, op->d_sh_ptr, op->d_sh_pairs,
                       static_cast<const T*>(op->d_partial), bvec + op->L.n_int_pad);
    HIPCHK(hipGetLastError());
  }
  return FUS_OK;
}

// b_internal = A x_internal  (all dofs: interior written by the block kernel, shared reduced) on device vectors in
// internal numbering, coef in internal cell order; kind = OP_STIFFNESS | OP_MASS
template <typename T>
static int apply_internal(fus_op* op, int kind, const void* coef, const void* x, void* bvec)
{
  fus_ctx* c = op->ctx;
  {
    ProfScope ps(c, kind == OP_STIFFNESS ? "stiffness" : "mass");
    const void* geo = kind == OP_STIFFNESS ? op->d_G : op->d_detJ;
    StageArgs<T> none{};
    FUSCHK(degree_impl(op->dtype, op->P)->block_op(op, kind, STAGE_NONE, 1, geo, coef, x, bvec, &none, 0, -1));
  }
  return shared_reduce<T>(op, static_cast<T*>(bvec));
}

// Shared-DOF exchange of a partial-sum vector (replaces b->scatter_rev(std::plus) +
// the two scatter_fwd of Linear.hpp:196-206): every sharer ends with the identical total because
// each adds the partials in ascending rank order.  Three phases so that the transport can sit
// between them: pack (own partials -> send buffers), exchange (RCCL send/recv over xGMI, or
// device copies for the in-process transport), unpack (ordered sum).
template <typename T>
static int halo_pack(fus_op* op, const void* vec_)
{
  const T* vec = static_cast<const T*>(vec_);
  if (op->neigh.empty())
    return FUS_OK;
  fus_ctx* c = op->ctx;
  hipLaunchKernelGGL((k_pack<T>), dim3(nblk(op->n_halo)), dim3(256), 0, c->stream, op->n_halo,
                     op->d_pack_idx, vec, static_cast<T*>(op->d_sendbuf));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_packed, c->stream));
  return FUS_OK;
}

// grouped send/recv with every neighbour on the comm stream, ordered after the pack by an event
int halo_exchange_rccl(fus_op* op)
{
  fus_ctx* c = op->ctx;
  if (op->neigh.empty())
    return FUS_OK;
  if (!c->comm)
    return fail(FUS_ERR_STATE, "neighbours set but fus_comm_init was not called");
  const ncclDataType_t dt = op->ts == 8 ? ncclDouble : ncclFloat;
  HIPCHK(hipStreamWaitEvent(c->comm_stream, c->ev_packed, 0));
  NCCLCHK(g_rccl.GroupStart());
  for (auto& nb : op->neigh)
  {
    const int peer = c->loopback ? 0 : nb.rank;
    NCCLCHK(g_rccl.Send(static_cast<char*>(op->d_sendbuf) + nb.off * op->ts, nb.count, dt, peer,
                        c->comm, c->comm_stream));
    NCCLCHK(g_rccl.Recv(static_cast<char*>(op->d_recvbuf) + nb.off * op->ts, nb.count, dt, peer,
                        c->comm, c->comm_stream));
  }
  NCCLCHK(g_rccl.GroupEnd());
  HIPCHK(hipEventRecord(c->ev_recv, c->comm_stream));
  return FUS_OK;
}

template <typename T>
static int halo_unpack(fus_op* op, void* vec_)
{
  T* vec = static_cast<T*>(vec_);
  fus_ctx* c = op->ctx;
  if (op->neigh.empty())
    return FUS_OK;
  if (!c->local_group)
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_recv, 0));
  hipLaunchKernelGGL((k_unpack_ordered<T>), dim3(nblk(op->n_uidx)), dim3(256), 0, c->stream,
                     op->n_uidx, op->d_uidx, op->d_uptr, op->d_usrc,
                     static_cast<const T*>(op->d_recvbuf), vec);
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

// RCCL transport: the three phases back to back
template <typename T>
static int halo_sum(fus_op* op, void* vec)
{
  if (op->neigh.empty())
    return FUS_OK;
  if (op->ctx->local_group)
    return fail(FUS_ERR_STATE, "in-process transport: use the fus_group_* entry points");
  ProfScope ps(op->ctx, "halo");
  FUSCHK(halo_pack<T>(op, vec));
  FUSCHK(halo_exchange_rccl(op));
  return halo_unpack<T>(op, vec);
}

// In-process transport: after every member has packed, move each send buffer to the matching
// receive buffer of the peer op (device copy), then every member unpacks.
int halo_exchange_local(fus_op** ops, int n)
{
  for (int i = 0; i < n; ++i)
    HIPCHK(hipStreamSynchronize(ops[i]->ctx->stream));
  for (int i = 0; i < n; ++i)
    for (auto& nb : ops[i]->neigh)
    {
      fus_op* peer = nullptr;
      for (int j = 0; j < n; ++j)
        if (ops[j]->ctx->rank == nb.rank)
          peer = ops[j];
      if (!peer)
        return fail(FUS_ERR_STATE, "neighbour rank not in the local group");
      Neigh* back = nullptr;
      for (auto& pn : peer->neigh)
        if (pn.rank == ops[i]->ctx->rank)
          back = &pn;
      if (!back || back->count != nb.count)
        return fail(FUS_ERR_STATE, "asymmetric neighbour lists");
      HIPCHK(hipMemcpyAsync(static_cast<char*>(peer->d_recvbuf) + back->off * peer->ts,
                            static_cast<const char*>(ops[i]->d_sendbuf) + nb.off * ops[i]->ts,
                            nb.count * ops[i]->ts, hipMemcpyDeviceToDevice, ops[i]->ctx->stream));
    }
  // device-to-device copies need not block the host: wait for them before anyone unpacks
  for (int i = 0; i < n; ++i)
    HIPCHK(hipStreamSynchronize(ops[i]->ctx->stream));
  return FUS_OK;
}

// Per-point geometry factors in the streaming layouts (precompute.hpp:101-213, 33-94), computed on
// the device.  Built at setup for non-affine meshes, on demand (fus_op_get_geometry) otherwise.
template <typename T>
static int ensure_stream_geometry(fus_op* op)
{
  if (op->d_G)
    return FUS_OK;
  hipStream_t st = op->ctx->stream;
  const int Nd = op->Nd, ng = op->tdim == 3 ? 6 : 3;
  FUSCHK(dalloc_bytes(op->allocs, &op->d_G, (size_t)op->ncells * ng * Nd * sizeof(T), false, st));
  FUSCHK(dalloc_bytes(op->allocs, &op->d_detJ, (size_t)op->ncells * Nd * sizeof(T), false, st));
  return degree_impl(op->dtype, op->P)->stream_geometry(op);
}

// The facts behind the block kernel's variant (block_variant.hpp) for geometry mode `mode`, with the options as the
// context holds them now
static OpFacts op_facts(const fus_op* op, int mode, bool ortho, int deterministic)
{
  const fus_ctx* c = op->ctx;
  return {op->P, (int)op->ts, op->tdim, op->geom_order, mode, ortho, deterministic != 0, c->mfma, c->pack32, c->diag_metric};
}

template <typename T>
static int op_setup_device(fus_op* op)
{
  if (!degree_impl(op->dtype, op->P))
    return fail(FUS_ERR_ARG, "unsupported polynomial degree (2..10)");
  const int N = op->N;
  fus_ctx* c = op->ctx;
  hipStream_t st = c->stream;
  Layout& L = op->L;
  auto& pool = op->allocs;

  int32_t* d_sh_gidx;
  BlockRecord* d_blk_rec;
  int16_t* d_rounds;
  uint16_t* d_ldm;
  FUSCHK(upload(pool, &d_blk_rec, L.blk_rec, st));
  FUSCHK(upload(pool, &d_sh_gidx, L.sh_gidx, st));
  FUSCHK(upload(pool, &d_rounds, L.rounds, st));
  L.ldm.resize((L.ldm.size() + 15) & ~(size_t)15);  // 16-byte tail for the vector copy
  FUSCHK(upload(pool, &d_ldm, L.ldm, st));
  FUSCHK(upload(pool, &op->d_cell_perm, L.cell_perm, st));
  FUSCHK(upload(pool, &op->d_dof_perm, L.dof_perm, st));
  FUSCHK(upload(pool, &op->d_sh_ptr, L.sh_ptr, st));
  {
    // the CSR the kernels read holds where each pair's partial sum is stored (Layout::pair_pos), not its pair id
    std::vector<int64_t> pos(L.sh_pairs.size());
    for (size_t k = 0; k < pos.size(); ++k)
      pos[k] = L.pair_pos[L.sh_pairs[k]];
    FUSCHK(upload(pool, &op->d_sh_pairs, pos, st));
  }
  int32_t* d_sh_ppos;
  FUSCHK(upload(pool, &d_sh_ppos, L.pair_pos, st));
  op->A.sh_ppos = d_sh_ppos;
  op->A.blk_rec = d_blk_rec, op->A.sh_gidx = d_sh_gidx;
  op->A.rounds = d_rounds, op->A.ldm = d_ldm, op->A.nblocks = L.nblocks;
  op->A.lds_nloc = (L.max_nloc + 1) & ~1;
  op->A.waves = L.waves;
  op->A.lds_nelem = (L.max_nelem + 7) & ~7;
  op->lds_bytes = L.lds_bytes(sizeof(T), op->nfields);
  if (op->lds_bytes > 160 * 1024)
    return fail(FUS_ERR_LIMIT, "block does not fit 160 KB of LDS; lower block_elems");

  // derivative table followed by the 1-D weights and points (the per-cell geometry paths rebuild
  // w_q / J(q) from them)
  std::vector<T> Dg(N * N + 2 * N);
  for (int i = 0; i < N * N; ++i)
    Dg[i] = (T)op->D[i];
  for (int i = 0; i < N; ++i)
    Dg[N * N + i] = (T)op->wts[i], Dg[N * N + N + i] = (T)op->nodes[i];
  T* d_Dg;
  FUSCHK(upload(pool, &d_Dg, Dg, st));
  op->d_Dg = d_Dg;

  // mesh geometry stays on the device for the (possibly deferred) per-point factors
  T* d_xg;
  FUSCHK(dalloc(pool, &d_xg, (size_t)op->nnodes * 3));
  HIPCHK(hipMemcpyAsync(d_xg, op->h_geom_x.data(), (size_t)op->nnodes * 3 * sizeof(T),
                        hipMemcpyHostToDevice, st));
  double *d_pts, *d_wts;
  FUSCHK(upload(pool, &op->d_xdm, op->h_geom_dm, st));
  FUSCHK(upload(pool, &d_pts, op->nodes, st));
  FUSCHK(upload(pool, &d_wts, op->wts, st));
  op->d_xg = d_xg, op->d_pts = d_pts, op->d_wts = d_wts;
  op->d_G = op->d_detJ = nullptr;

  // per-cell factors + affinity test (every cell a parallelepiped?)
  T* d_Gc;
  unsigned int* d_err;
  FUSCHK(dalloc(pool, &d_Gc, (size_t)op->ncells * 21));
  FUSCHK(dalloc(pool, &d_err, 1));
  HIPCHK(hipMemsetAsync(d_err, 0, sizeof(unsigned int), st));
  float rel_err = 1.0f;
  if (op->geom_order == 1 && op->tdim == 3)
  {
    hipLaunchKernelGGL((k_geometry_affine<T>), dim3(nblk(op->ncells)), dim3(256), 0, st, op->ncells,
                       op->d_cell_perm, d_xg, op->d_xdm, d_Gc, d_err);
    HIPCHK(hipGetLastError());
    unsigned int err_bits = 0;
    HIPCHK(hipMemcpyAsync(&err_bits, d_err, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(&rel_err, &err_bits, sizeof(float));
  }
  op->d_Gc = d_Gc;
  const bool affine = c->geometry == 0 && rel_err <= (sizeof(T) == 8 ? 1e-12f : 1e-6f);
  const bool trilinear = !affine && c->geometry != 1 && op->geom_order == 1 && op->tdim == 3;
  // the confirmed mode settles the traits; the layout's pk is a fact by now
  op->facts = op_facts(op, affine ? GEOM_AFFINE : (trilinear ? GEOM_TRILINEAR : GEOM_STREAM), op->facts.ortho, op->deterministic);
  op->traits = op_traits(op->facts, op->traits.pk);
  if (trilinear)
  {
    hipLaunchKernelGGL((k_geometry_trilinear<T>), dim3(nblk(op->ncells)), dim3(256), 0, st, op->ncells,
                       op->d_cell_perm, d_xg, op->d_xdm, d_Gc);
    HIPCHK(hipGetLastError());
  }
  if (op->traits.gcs)
    op->lds_bytes = L.lds_bytes(sizeof(T), op->nfields, op->traits.gcs);
  else
    FUSCHK(ensure_stream_geometry<T>(op));

  {
    // does every block fit the first batches of the straight-line kernels (block_variant.hpp)?
    BlockExtents e{64 * L.waves, 0, 0, L.max_nelem, L.Nd};
    for (const Layout::Shape& s : L.shapes)
      e.max_nint = std::max(e.max_nint, (int)s.nint), e.max_nsh = std::max(e.max_nsh, (int)(s.nloc - s.nint));
    op_traits_fit(op->traits, op->P, e);
  }
  FUSCHK(dalloc_bytes(pool, &op->d_partial, (size_t)(L.n_partial + L.n_shared) * sizeof(T), true, st));
  FUSCHK(dalloc_bytes(pool, &op->d_tmp_x, (size_t)L.n_internal * sizeof(T), true, st));
  FUSCHK(dalloc_bytes(pool, &op->d_tmp_b, (size_t)L.n_internal * sizeof(T), true, st));
  FUSCHK(dalloc_bytes(pool, &op->d_tmp_c, (size_t)op->ndofs * sizeof(T), true, st));
  FUSCHK(dalloc_bytes(pool, &op->d_tmp_coef, (size_t)op->ncells * sizeof(T) * 2, true, st));
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

// y += A(coeffs) x with caller-numbered vectors (the reference operator call)
template <typename T>
static int op_apply(fus_op* op, int kind, const void* x, const void* coeffs, void* y, int space)
{
  fus_ctx* c = op->ctx;
  hipStream_t st = c->stream;
  T* xin = static_cast<T*>(op->d_tmp_x);
  T* bint = static_cast<T*>(op->d_tmp_b);
  T* tc = static_cast<T*>(op->d_tmp_c);
  T* coef_c = static_cast<T*>(op->d_tmp_coef);
  T* coef_i = coef_c + op->ncells;
  const T* xc = static_cast<const T*>(x);
  const T* cc = static_cast<const T*>(coeffs);
  if (space == FUS_HOST)
  {
    HIPCHK(hipMemcpyAsync(tc, x, op->ndofs * sizeof(T), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(coef_c, coeffs, op->ncells * sizeof(T), hipMemcpyHostToDevice, st));
    xc = tc, cc = coef_c;
  }
  hipLaunchKernelGGL((k_to_internal<T>), dim3(nblk(op->ndofs)), dim3(256), 0, st, op->ndofs,
                     op->d_dof_perm, xc, xin);
  hipLaunchKernelGGL((k_cells_to_internal<T>), dim3(nblk(op->ncells)), dim3(256), 0, st, op->ncells,
                     op->d_cell_perm, cc, coef_i);
  FUSCHK(apply_internal<T>(op, kind, coef_i, xin, bint));
  if (space == FUS_HOST)
  {
    HIPCHK(hipMemcpyAsync(tc, y, op->ndofs * sizeof(T), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_from_internal<T, 1>), dim3(nblk(op->ndofs)), dim3(256), 0, st, op->ndofs,
                       op->d_dof_perm, bint, tc);
    HIPCHK(hipMemcpyAsync(y, tc, op->ndofs * sizeof(T), hipMemcpyDeviceToHost, st));
  }
  else
    hipLaunchKernelGGL((k_from_internal<T, 1>), dim3(nblk(op->ndofs)), dim3(256), 0, st, op->ndofs,
                       op->d_dof_perm, bint, static_cast<T*>(y));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

template <typename T>
static int op_get_geometry(fus_op* op, void* G, void* detJ)
{
  hipStream_t st = op->ctx->stream;
  FUSCHK(ensure_stream_geometry<T>(op));
  const int Nd = op->Nd, ng = op->tdim == 3 ? 6 : 3;
  std::vector<void*> tmp;
  T *dG = nullptr, *dd = nullptr;
  if (G)
    FUSCHK(dalloc(tmp, &dG, (size_t)op->ncells * Nd * ng));
  if (detJ)
    FUSCHK(dalloc(tmp, &dd, (size_t)op->ncells * Nd));
  FUSCHK(degree_impl(op->dtype, op->P)->export_geometry(op, dG, dd));
  if (G)
    HIPCHK(hipMemcpyAsync(G, dG, (size_t)op->ncells * Nd * ng * sizeof(T), hipMemcpyDeviceToHost, st));
  if (detJ)
    HIPCHK(hipMemcpyAsync(detJ, dd, (size_t)op->ncells * Nd * sizeof(T), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (void* q : tmp)
    (void)hipFree(q);
  return FUS_OK;
}

// -------------------------------------------------------------------------------------------------
// dispatch over (dtype, P): the launches that hold the degree live in the per-degree units (degree_unit.hip).
// degree_impl (declared in core.hpp): the unit of a scalar type and degree, nullptr where the library holds none.
// op_setup_device refuses such an operator, so every later call finds its unit.
// -------------------------------------------------------------------------------------------------
#define FUS_DECL_DEGREE(k)                                                                         \
  FUS_HIDDEN const DegreeImpl* FUS_DEGREE_IMPL_FN(k, 64)();                                        \
  FUS_HIDDEN const DegreeImpl* FUS_DEGREE_IMPL_FN(k, 32)();
#define FUS_CASE_DEGREE(k)                                                                         \
  case k:                                                                                          \
    return dtype == FUS_F64 ? FUS_DEGREE_IMPL_FN(k, 64)() : FUS_DEGREE_IMPL_FN(k, 32)();
#ifdef FUS_DEV_BUILD  // developer iteration build: ONE degree (never shipped; build.py --dev)
#ifndef FUS_DEV_DEGREE
#define FUS_DEV_DEGREE 4
#endif
FUS_DECL_DEGREE(FUS_DEV_DEGREE)
const DegreeImpl* degree_impl(int dtype, int P)
{
  switch (P)
  {
    FUS_CASE_DEGREE(FUS_DEV_DEGREE)
  default: return nullptr;
  }
}
#else
FUS_DECL_DEGREE(2) FUS_DECL_DEGREE(3) FUS_DECL_DEGREE(4) FUS_DECL_DEGREE(5) FUS_DECL_DEGREE(6) FUS_DECL_DEGREE(7)
FUS_DECL_DEGREE(8) FUS_DECL_DEGREE(9) FUS_DECL_DEGREE(10)
const DegreeImpl* degree_impl(int dtype, int P)
{
  switch (P)
  {
    FUS_CASE_DEGREE(2) FUS_CASE_DEGREE(3) FUS_CASE_DEGREE(4) FUS_CASE_DEGREE(5) FUS_CASE_DEGREE(6) FUS_CASE_DEGREE(7)
    FUS_CASE_DEGREE(8) FUS_CASE_DEGREE(9) FUS_CASE_DEGREE(10)
  default: return nullptr;
  }
}
#endif

// by the operator's scalar type, for the wave and bioheat units (declared in core.hpp)
int d_apply_internal(fus_op* op, int kind, const void* coef, const void* x, void* b) { return FUS_BY_DTYPE(op->dtype, apply_internal, op, kind, coef, x, b); }
int d_halo_sum(fus_op* op, void* v) { return FUS_BY_DTYPE(op->dtype, halo_sum, op, v); }
int d_halo_pack(fus_op* op, const void* v) { return FUS_BY_DTYPE(op->dtype, halo_pack, op, v); }
int d_halo_unpack(fus_op* op, void* v) { return FUS_BY_DTYPE(op->dtype, halo_unpack, op, v); }

// (Re)build the block layout and the device-side operator data.  force_shared marks dofs held by
// other ranks too: they must never be finished inside a block's fused epilogue.
static int op_build(fus_op* op, const uint8_t* force_shared)
{
  fus_ctx* c = op->ctx;
  for (void* q : op->allocs)
    (void)hipFree(q);
  op->allocs.clear();
  // (the gradient kernel's arrays were among them: gradient.hip allocates them again for the new layout)
  op->d_grad_y = op->d_grad_part = op->d_grad_den = op->d_grad_coef = op->d_grad_in = nullptr, op->grad_in_bytes = 0;
  // centroids for the block partitioner
  std::vector<double> cen((size_t)op->ncells * 3, 0.0);
  const int nv = op->geom_nv;
  for (int64_t cidx = 0; cidx < op->ncells; ++cidx)
    for (int v = 0; v < nv; ++v)
      for (int j = 0; j < 3; ++j)
      {
        const size_t k = 3 * (size_t)op->h_geom_dm[cidx * nv + v] + j;
        cen[3 * cidx + j] +=
            (1.0 / nv) * (op->dtype == FUS_F64 ? reinterpret_cast<const double*>(op->h_geom_x.data())[k]
                                          : (double)reinterpret_cast<const float*>(op->h_geom_x.data())[k]);
      }
  // will the per-cell (affine) geometry path be taken?  (same test as k_geometry_affine, on the host
  // copy: every vertex of every cell on the parallelepiped spanned by vertices 0, 1, 2, 4)
  bool affine_mesh = c->geometry == 0 && op->geom_order == 1 && op->tdim == 3;
  bool ortho_mesh = affine_mesh;
  for (int64_t cidx = 0; cidx < op->ncells && affine_mesh; ++cidx)
  {
    double cd[8][3], h2 = 0, e2 = 0;
    for (int v = 0; v < 8; ++v)
      for (int j = 0; j < 3; ++j)
      {
        const size_t k = 3 * (size_t)op->h_geom_dm[cidx * 8 + v] + j;
        cd[v][j] = op->dtype == FUS_F64 ? reinterpret_cast<const double*>(op->h_geom_x.data())[k]
                                        : (double)reinterpret_cast<const float*>(op->h_geom_x.data())[k];
      }
    for (int v = 0; v < 8; ++v)
      for (int i = 0; i < 3; ++i)
      {
        const double e0 = cd[1][i] - cd[0][i], e1 = cd[2][i] - cd[0][i], e4 = cd[4][i] - cd[0][i];
        const double d = cd[v][i] - (cd[0][i] + (v & 1) * e0 + ((v >> 1) & 1) * e1 + (v >> 2) * e4);
        e2 = std::max(e2, d * d);
        if (v == 0)
          h2 += e0 * e0 + e1 * e1 + e4 * e4;
      }
    const double tol = op->dtype == FUS_F64 ? 1e-12 : 1e-6;
    if (std::sqrt(e2 / h2) > 0.5 * tol)
      affine_mesh = false;
    // mutually orthogonal edges: J^T J, and with it G = |det J| (J^T J)^-1, is diagonal
    double ed[3][3];
    for (int i = 0; i < 3; ++i)
      ed[0][i] = cd[1][i] - cd[0][i], ed[1][i] = cd[2][i] - cd[0][i], ed[2][i] = cd[4][i] - cd[0][i];
    for (int u = 0; u < 3; ++u)
      for (int v = u + 1; v < 3; ++v)
      {
        double dot = 0, nu = 0, nv2 = 0;
        for (int i = 0; i < 3; ++i)
          dot += ed[u][i] * ed[v][i], nu += ed[u][i] * ed[u][i], nv2 += ed[v][i] * ed[v][i];
        if (std::fabs(dot) > (op->dtype == FUS_F64 ? 1e-14 : 2e-7) * std::sqrt(nu * nv2))
          ortho_mesh = false;
      }
  }
  // first-order hexahedra that are not all affine: J and G recomputed per point from each cell's
  // trilinear map (GEOM_TRILINEAR) unless the streamed factors are asked for; else: per-point factors streamed
  const bool trilinear_mesh = !affine_mesh && c->geometry != 1 && op->geom_order == 1 && op->tdim == 3;
  // the traits of the predicted mode: whether the layout gets the packed kernel's two slots, and the LDS budget
  op->facts = op_facts(op, affine_mesh ? GEOM_AFFINE : (trilinear_mesh ? GEOM_TRILINEAR : GEOM_STREAM),
                       affine_mesh && ortho_mesh, c->deterministic);
  op->traits = op_traits(op->facts);
  const int gcs = op->traits.gcs;
  // auto block size: about 2-3 thousand local dofs per block when G is streamed (128 / 64 / 32
  // elements at P = 2 / 3 / >= 4; larger P shrink further to fit LDS), half of that on the affine
  // path (profiles/r01_block_sweep.txt)
  // quadrilaterals: N^2 nodes per element, so many more elements make a block of that size
  if (op->P >= 8)
  {
    // degrees 8-10 (two waves per element): 4-element blocks, an even number of waves
    int waves8 = c->waves > 0 ? std::min(4, (c->waves + 1) & ~1) : 4;
    // (fp64 distorted cells at degree 8: 8-element blocks, +8.5 % over 4 -- fewer shared dofs; profiles/r03_experiments.md 7)
    const int be_hi = op->tdim == 2 ? 32 : ((op->P == 8 && op->dtype == FUS_F64 && trilinear_mesh) ? 8 : 4);
    for (int be = c->block_elems > 0 ? c->block_elems : be_hi;; be = (be + 1) / 2)
    {
      std::string err = build_layout(op->L, op->P, op->ncells, op->ndofs, op->h_dofmap.data(), cen.data(), be, waves8,
                                     force_shared, op->tdim);
      const bool too_big = err.empty() ? op->L.lds_bytes(op->ts, op->nfields, gcs) + 64 > 160 * 1024
                                       : err.find("65535") != std::string::npos;
      if (too_big && be > 1)
        continue;
      if (!err.empty())
        return fail(FUS_ERR_ARG, "layout: " + err);
      if (too_big)
        return fail(FUS_ERR_LIMIT, "a one-element block does not fit the LDS budget at this degree");
      break;
    }
    int r8 = FUS_BY_DTYPE(op->dtype, op_setup_device, op);
    if (r8 != FUS_OK)
    {
      for (void* q : op->allocs)
        (void)hipFree(q);
      op->allocs.clear();
    }
    return r8;
  }
  static const int be_quad[8] = {0, 0, 512, 256, 256, 128, 128, 64};
  // fp32 halves the LDS per dof: there the best sizes keep two or three blocks per CU resident
  // (p=4: 48, p=5/6: 24, p=7: 16 -- +8 / +15 / +45 / +42 % over 32 elements, profiles/r01_block_sweep.txt)
  static const int be_hex_f32[8] = {0, 0, 128, 64, 48, 24, 24, 16};
  const int be_hex = op->dtype == FUS_F32 ? be_hex_f32[op->P] : (op->P == 2 ? 128 : (op->P == 3 ? 64 : 32));
  const int be_stream = op->tdim == 2 ? be_quad[op->P] : be_hex;
  // fp64, p >= 5, streamed geometry, LDS-atomic mode: the block kernel keeps ONE geometry register
  // set there (kernels.hpp, FUS_PF1) and fits two waves per SIMD, which pays only if two blocks per
  // CU are resident: blocks of at most 80 KB of LDS (20 / 12 / 8 elements at p = 5 / 6 / 7 with one
  // operator input, fewer with two).  +50 / +30 / +35 % over one 32->16-element block per CU.
  const bool two_per_cu = op->dtype == FUS_F64 && op->tdim == 3 && op->P >= 5 && !affine_mesh && !trilinear_mesh
                          && c->block_elems <= 0;
  static const int be_two[8] = {0, 0, 0, 0, 0, 20, 12, 8};
  // per-cell geometry paths (affine, trilinear): about half the streamed size; at p >= 5 blocks of 8
  // elements, small enough for four / three / two blocks per CU at the register budgets of those
  // kernels (p=5: +3-5 % over 12, p=6: +19-20 %; profiles/r01_block_sweep.txt)
  // (fp32, round 3: the fp64 block accumulator costs 4 more bytes of LDS per local dof; re-swept at 64^3,
  // profiles/r03_experiments.md section 4: affine 8 / 8 / 4 elements at p = 5 / 6 / 7)
  static const int be_aff_hi[8] = {0, 0, 0, 0, 0, 8, 8, 8};
  const int be_affine = (op->tdim == 3 && op->P >= 5) ? ((op->dtype == FUS_F32 && op->P == 7) ? 4 : be_aff_hi[op->P])
                                                      : be_stream / 2;
  // fp32 halves the LDS per block: the trilinear kernel takes 16 elements at p >= 5 (+9-12 %), the
  // affine one at p = 5 only (+5 %; 16 is 2-9 % slower at p = 6, 7)
  // (round 3, fp64 accumulator: 16 / 8 / 8 elements at p = 5 / 6 / 7)
  const bool hi32 = op->dtype == FUS_F32 && op->tdim == 3 && op->P >= 5;
  const int be_tri = hi32 ? (op->P == 5 ? 16 : 8) : be_affine;
  const int be0 = c->block_elems > 0
                      ? c->block_elems
                      : ((trilinear_mesh || affine_mesh) && op->P == 4 && op->nfields == 1 && c->waves <= 0) ? 32
                      : (two_per_cu ? be_two[op->P]
                                    : (trilinear_mesh ? be_tri : (affine_mesh ? be_affine : be_stream)));
  const size_t lds_cap = two_per_cu ? 80 * 1024 : 160 * 1024;
  int waves = c->waves > 0 ? c->waves : 4;
  if (op->P > 4 && waves > FUS_MID_THREADS / 64)
    waves = FUS_MID_THREADS / 64;  // launch bound of the block kernel for the higher degrees
  // per-cell geometry paths at p = 4 in fp64: 32 elements / 8 waves (two 8-wave blocks per CU) leave fewer
  // shared dofs than 16 / 4 -- the block kernel is 2-6 % slower, the step 1.5-3 % faster
  // (one operator input only: with two, such a block takes 92 KB of LDS and a CU holds one)
  // (fp32: the same 32 elements, +7-8 % over 24; eight waves on affine cells, four on the trilinear kernel)
  // (fp32 trilinear too since the fp64 accumulator: 1.58 -> 1.62e10 with eight waves)
  const bool tri_p4 = (trilinear_mesh || affine_mesh) && op->P == 4 && op->nfields == 1 && c->waves <= 0
                      && c->block_elems <= 0;
  if (tri_p4)
    waves = 8;
  // blocks must fit the LDS budget (the CU's 160 KB, or half of it): shrink the block until they do
  for (int be = be0;; be = two_per_cu && be > 4 ? be - std::max(1, be / 4) : (be + 1) / 2)
  {
    std::string err = build_layout(op->L, op->P, op->ncells, op->ndofs, op->h_dofmap.data(),
                                   cen.data(), be, waves, force_shared, op->tdim, op->traits.pk ? 2 : 1);
    const bool too_big = err.empty() ? op->L.lds_bytes(op->ts, op->nfields, gcs) + 64 > lds_cap
                                     : err.find("65535") != std::string::npos;
    if (too_big && be > 1)
      continue;
    if (!err.empty())
      return fail(FUS_ERR_ARG, "layout: " + err);
    if (too_big)
      return fail(FUS_ERR_LIMIT, "a one-element block does not fit the LDS budget at this degree");
    break;
  }
  int r = FUS_BY_DTYPE(op->dtype, op_setup_device, op);
  if (r != FUS_OK)
  {
    for (void* q : op->allocs)
      (void)hipFree(q);
    op->allocs.clear();
  }
  return r;
}

// -------------------------------------------------------------------------------------------------
// C ABI
// -------------------------------------------------------------------------------------------------
extern "C"
{

const char* fus_last_error(void) { return g_err.c_str(); }
int fus_version(void) { return 1; }

int fus_init(int device, fus_ctx** out)
{
  if (!out)
    return fail(FUS_ERR_ARG, "null ctx pointer");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(FUS_ERR_HIP, "no HIP device: libfusmi has no CPU fallback");
  if (device < 0 || device >= ndev)
    return fail(FUS_ERR_ARG, "device index out of range");
  HIPCHK(hipSetDevice(device));
  auto* c = new fus_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    c->num_cus = prop.multiProcessorCount;
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&c->ev_packed, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&c->ev_recv, hipEventDisableTiming));
  *out = c;
  return FUS_OK;
}

int fus_finalize(fus_ctx* c)
{
  if (!c)
    return FUS_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (auto& kv : c->profs)
    for (auto& ev : kv.second.ev)
      (void)hipEventDestroy(ev.first), (void)hipEventDestroy(ev.second);
  (void)hipStreamSynchronize(c->comm_stream);
  if (c->comm)
    g_rccl.CommDestroy(c->comm);
  (void)hipEventDestroy(c->ev_packed), (void)hipEventDestroy(c->ev_recv);
  (void)hipStreamDestroy(c->comm_stream);
  (void)hipStreamDestroy(c->stream);
  delete c;
  return FUS_OK;
}

int fus_synchronize(fus_ctx* c)
{
  HIPCHK(hipStreamSynchronize(c->stream));
  return FUS_OK;
}

int fus_set_option(fus_ctx* c, const char* key, int64_t value)
{
  if (!c || !key)
    return fail(FUS_ERR_ARG, "null argument");
  if (!strcmp(key, "block_elems"))
  {
    if (value < 0 || value > 4096)
      return fail(FUS_ERR_ARG, "block_elems out of range");
    c->block_elems = (int)value;
  }
  else if (!strcmp(key, "waves"))
  {
    if (value < 0 || value > 8)
      return fail(FUS_ERR_ARG, "waves must be 0 (auto) or 1..8");
    c->waves = (int)value;
  }
  else if (!strcmp(key, "deterministic"))
    c->deterministic = value != 0;
  else if (!strcmp(key, "graph"))
    c->graph = value != 0;
  else if (!strcmp(key, "geometry"))
  {
    if (value < 0 || value > 2)
      return fail(FUS_ERR_ARG, "geometry must be 0 (auto), 1 (stream) or 2 (trilinear)");
    c->geometry = (int)value;
  }
  else if (!strcmp(key, "halo_loopback"))
    c->loopback = value != 0;
  else if (!strcmp(key, "overlap_blocks"))
    c->overlap_blocks = value != 0;
  else if (!strcmp(key, "external_transport"))
    c->external_transport = value != 0;
  else if (!strcmp(key, "forms"))
  {
    if (value != 0 && value != 1)
      return fail(FUS_ERR_ARG, "forms must be 0 (C++ benchmark forms) or 1 (Python package forms)");
    c->forms = (int)value;
  }
  else if (!strcmp(key, "lean_rk4"))
    c->lean_rk4 = value != 0;
  else if (!strcmp(key, "pack32"))
  {
    if (value < -1 || value > 1)
      return fail(FUS_ERR_ARG, "pack32 must be -1 (auto), 0 or 1");
    c->pack32 = (int)value;
  }
  else if (!strcmp(key, "profile_sample"))
  {
    if (value < 1 || value > 1000)
      return fail(FUS_ERR_ARG, "profile_sample must be 1..1000");
    c->prof_sample = (int)value;
  }
  else if (!strcmp(key, "planes"))
  {
    if (value < 0 || value > 16)   // FUS_MAX_PLANES (wave_kernels.hpp; wave.hip asserts the 16)
      return fail(FUS_ERR_ARG, "planes must be 0 (CSR form), 1 (planes) or 2..16 (planes for meshes with at most so many sharers of a dof)");
    c->planes = (int)value;
  }
  else if (!strcmp(key, "diag_metric"))
    c->diag_metric = value != 0;
  else if (!strcmp(key, "walk"))
  {
    if (value < -1 || value > 8)
      return fail(FUS_ERR_ARG, "walk must be -1 (auto), 0 (one workgroup per block) or 1..8 workgroups per CU");
    c->walk = (int)value;
  }
  else if (!strcmp(key, "rayleigh_chunks"))
  {
    if (value < 0 || value > 1024)   // RAY_MAX_CHUNKS (rayleigh.hip)
      return fail(FUS_ERR_ARG, "rayleigh_chunks must be 0 (auto) or 1..1024");
    c->rayleigh_chunks = (int)value;
  }
  else if (!strcmp(key, "mfma"))
  {
    if (value < -1 || value > 1)
      return fail(FUS_ERR_ARG, "mfma must be -1 (auto), 0 or 1");
    c->mfma = (int)value;
  }
  else if (!strcmp(key, "fields"))
  {
    if (value != 1 && value != 2)
      return fail(FUS_ERR_ARG, "fields must be 1 or 2");
    c->fields = (int)value;
  }
  else
    return fail(FUS_ERR_ARG, std::string("unknown option ") + key);
  return FUS_OK;
}

int fus_comm_unique_id(void* id128)
{
  static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id is 128 bytes");
  FUSCHK(rccl_load());
  ncclUniqueId id;
  NCCLCHK(g_rccl.GetUniqueId(&id));
  memcpy(id128, &id, 128);
  return FUS_OK;
}

int fus_comm_init(fus_ctx* c, int rank, int nranks, const void* id128)
{
  if (!c || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(FUS_ERR_ARG, "bad rank/nranks");
  c->rank = rank, c->nranks = nranks;
  if (c->external_transport)
  {
    // the caller moves the packed interface values itself (fus_op_halo_buffers): no communicator, the
    // stage / setup halves are driven through fus_model_stage_begin/_end, fus_model_setup_*
    c->local_group = nranks > 1;
    return FUS_OK;
  }
  if (nranks == 1 && !id128)
    return FUS_OK;
  if (!id128)
    return fail(FUS_ERR_ARG, "fus_comm_init: RCCL id missing (or set option external_transport)");
  FUSCHK(rccl_load());
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  HIPCHK(hipSetDevice(c->device));
  if (c->loopback)
    NCCLCHK(g_rccl.CommInitRank(&c->comm, 1, id, 0));
  else
    NCCLCHK(g_rccl.CommInitRank(&c->comm, nranks, id, rank));
  return FUS_OK;
}

// Round trip of n doubles through ncclSend/ncclRecv to the own rank on the library's stream:
// checks the run-time RCCL binding and the grouped send/recv pattern the halo exchange uses.
int fus_comm_selftest(fus_ctx* c, int64_t n)
{
  if (!c || n < 2)
    return fail(FUS_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  FUSCHK(rccl_load());
  ncclComm_t comm = c->comm;
  bool own = false;
  if (!comm)
  {
    ncclUniqueId id;
    NCCLCHK(g_rccl.GetUniqueId(&id));
    NCCLCHK(g_rccl.CommInitRank(&comm, 1, id, 0));
    own = true;
  }
  std::vector<double> h(n), back(n, 0.0);
  for (int64_t i = 0; i < n; ++i)
    h[i] = 0.5 * (double)i - 3.0;
  double *a = nullptr, *b = nullptr;
  HIPCHK(hipMalloc((void**)&a, n * sizeof(double)));
  HIPCHK(hipMalloc((void**)&b, n * sizeof(double)));
  HIPCHK(hipMemcpyAsync(a, h.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(b, 0, n * sizeof(double), c->stream));
  const int self = own ? 0 : c->rank;
  NCCLCHK(g_rccl.GroupStart());
  NCCLCHK(g_rccl.Send(a, n, ncclDouble, self, comm, c->stream));
  NCCLCHK(g_rccl.Recv(b, n, ncclDouble, self, comm, c->stream));
  NCCLCHK(g_rccl.GroupEnd());
  HIPCHK(hipMemcpyAsync(back.data(), b, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  // and the all-reduce of fus_comm_allreduce (over this communicator's ranks; a 1-rank one returns its input)
  double red[2] = {0, 0};
  if (own || c->nranks == 1)
  {
    NCCLCHK(g_rccl.AllReduce(a, a, 2, ncclDouble, ncclMin, comm, c->stream));
    HIPCHK(hipMemcpyAsync(red, a, sizeof(red), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  (void)hipFree(a), (void)hipFree(b);
  if (own)
    g_rccl.CommDestroy(comm);
  for (int64_t i = 0; i < n; ++i)
    if (back[i] != h[i])
      return fail(FUS_ERR_RCCL, "RCCL self send/recv returned wrong data");
  if ((own || c->nranks == 1) && n >= 2 && (red[0] != h[0] || red[1] != h[1]))
    return fail(FUS_ERR_RCCL, "RCCL all-reduce over one rank changed the data");
  return FUS_OK;
}

// Scalars every rank needs: the global minimum cell size behind the time step
// (MPI_Reduce(MIN) + MPI_Bcast, fenicsx-sf-naive/examples/linear_planewave2d_1/main.cpp:67-68) and the
// sums behind norms (fem::assemble_scalar + MPI sum, :151-157), over the library's RCCL communicator.
int fus_comm_allreduce(fus_ctx* c, double* values, int n, int op)
{
  if (!c || !values || n < 1 || op < FUS_SUM || op > FUS_MAX)
    return fail(FUS_ERR_ARG, "bad argument");
  if (c->nranks <= 1 || c->loopback)
    return FUS_OK;
  if (c->local_group || !c->comm)
    return fail(FUS_ERR_STATE, "fus_comm_allreduce needs the RCCL communicator (in-process groups and the "
                               "external transport reduce on the caller's side)");
  HIPCHK(hipSetDevice(c->device));
  double* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, n * sizeof(double)));
  HIPCHK(hipMemcpyAsync(d, values, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const ncclRedOp_t rop = op == FUS_SUM ? ncclSum : (op == FUS_MIN ? ncclMin : ncclMax);
  ncclResult_t r = g_rccl.AllReduce(d, d, (size_t)n, ncclDouble, rop, c->comm, c->stream);
  if (r == ncclSuccess)
  {
    HIPCHK(hipMemcpyAsync(values, d, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  (void)hipFree(d);
  NCCLCHK(r);
  return FUS_OK;
}

// Smallest cell size of the local mesh, size = largest vertex-to-vertex distance of a cell
// (dolfinx::mesh::h as used by linear_planewave2d_1/main.cpp:60-64).
int fus_op_hmin(fus_op* op, double* hmin)
{
  if (!op || !hmin)
    return fail(FUS_ERR_ARG, "null argument");
  const int nv1 = op->tdim == 3 ? 8 : 4;
  const int nvg = op->geom_order == 1 ? nv1 : (op->tdim == 3 ? 27 : 9);
  int vert[8];
  for (int v = 0; v < nv1; ++v)  // second order: tensor nodes with every index in {0, 2}
    vert[v] = op->geom_order == 1 ? v : 2 * (v & 1) + 6 * ((v >> 1) & 1) + 18 * (v >> 2);
  auto coord = [&](int64_t node, int j) -> double
  {
    const size_t k = 3 * (size_t)node + j;
    return op->dtype == FUS_F64 ? reinterpret_cast<const double*>(op->h_geom_x.data())[k]
                                : (double)reinterpret_cast<const float*>(op->h_geom_x.data())[k];
  };
  double best = std::numeric_limits<double>::infinity();
  for (int64_t cidx = 0; cidx < op->ncells; ++cidx)
  {
    double h2 = 0;
    for (int a = 0; a < nv1; ++a)
      for (int b = a + 1; b < nv1; ++b)
      {
        double d2 = 0;
        for (int j = 0; j < 3; ++j)
        {
          const double d = coord(op->h_geom_dm[cidx * nvg + vert[a]], j) - coord(op->h_geom_dm[cidx * nvg + vert[b]], j);
          d2 += d * d;
        }
        h2 = std::max(h2, d2);
      }
    best = std::min(best, h2);
  }
  *hmin = std::sqrt(best);
  return FUS_OK;
}

int fus_op_create(fus_ctx* c, int tdim, int P, int dtype, int64_t ncells, int64_t ndofs,
                  const int32_t* tensor_dofmap, const double* nodes1d, const void* geom_x,
                  int64_t nnodes, const int32_t* geom_dofmap, int geom_order, fus_op** out)
{
  if (!c || !out || !tensor_dofmap || !nodes1d || !geom_x || !geom_dofmap)
    return fail(FUS_ERR_ARG, "null argument");
  if (tdim != 2 && tdim != 3)
    return fail(FUS_ERR_ARG, "tdim must be 3 (hexahedra) or 2 (quadrilaterals)");
  if (P < 2 || P > 10)
    return fail(FUS_ERR_ARG, "unsupported polynomial degree (2..10)");
  if (dtype != FUS_F64 && dtype != FUS_F32)
    return fail(FUS_ERR_ARG, "dtype must be FUS_F32 or FUS_F64");
  if (geom_order != 1 && geom_order != 2)
    return fail(FUS_ERR_ARG, "geometry order must be 1 (2^tdim vertices) or 2 (3^tdim nodes, tensor order)");
  if (ncells <= 0 || ndofs <= 0 || nnodes <= 0)
    return fail(FUS_ERR_ARG, "empty mesh");
  const int N = P + 1;
  if (!is_gll_node_set(N, nodes1d))
    return fail(FUS_ERR_ARG, "nodes1d are not the GLL points of [0,1]");
  HIPCHK(hipSetDevice(c->device));
  std::unique_ptr<fus_op> op(new fus_op());
  op->deterministic = c->deterministic;
  op->nfields = c->fields;
  op->ctx = c, op->P = P, op->N = N, op->tdim = tdim, op->dtype = dtype;
  op->Nd = tdim == 3 ? N * N * N : N * N;
  op->ts = dtype == FUS_F64 ? 8 : 4;
  op->ncells = ncells, op->ndofs = ndofs, op->nnodes = nnodes;
  op->nodes.assign(nodes1d, nodes1d + N);
  op->wts = gll_weights_at(N, nodes1d);
  op->D = dphi_table(N, nodes1d);
  op->h_geom_x.assign(static_cast<const char*>(geom_x),
                      static_cast<const char*>(geom_x) + (size_t)nnodes * 3 * op->ts);
  op->geom_order = geom_order;
  op->geom_nv = geom_order == 2 ? (tdim == 3 ? 27 : 9) : (tdim == 3 ? 8 : 4);
  op->h_geom_dm.assign(geom_dofmap, geom_dofmap + ncells * op->geom_nv);
  op->h_dofmap.assign(tensor_dofmap, tensor_dofmap + ncells * op->Nd);
  for (int64_t k = 0; k < ncells * op->geom_nv; ++k)
    if (geom_dofmap[k] < 0 || geom_dofmap[k] >= nnodes)
      return fail(FUS_ERR_ARG, "geometry dofmap entry out of range");
  int r = op_build(op.get(), nullptr);
  if (r != FUS_OK)
    return r;
  *out = op.release();
  return FUS_OK;
}

int fus_op_destroy(fus_op* op)
{
  if (!op)
    return FUS_OK;
  (void)hipSetDevice(op->ctx->device);
  (void)hipStreamSynchronize(op->ctx->stream);
  for (void* q : op->allocs)
    (void)hipFree(q);
  for (void* q : {(void*)op->d_pack_idx, (void*)op->d_uidx, (void*)op->d_uptr, (void*)op->d_usrc,
                  op->d_sendbuf, op->d_recvbuf})
    (void)hipFree(q);
  delete op;
  return FUS_OK;
}

int fus_stiffness_apply(fus_op* op, const void* x, const void* coeffs, void* y, int space)
{
  if (!op || !x || !coeffs || !y)
    return fail(FUS_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(op->ctx->device));
  return FUS_BY_DTYPE(op->dtype, op_apply, op, OP_STIFFNESS, x, coeffs, y, space);
}

int fus_mass_apply(fus_op* op, const void* x, const void* coeffs, void* y, int space)
{
  if (!op || !x || !coeffs || !y)
    return fail(FUS_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(op->ctx->device));
  return FUS_BY_DTYPE(op->dtype, op_apply, op, OP_MASS, x, coeffs, y, space);
}

// sum over the LOCAL cells of the GLL-quadrature integral of x^2 (= x . M(1) x with the local,
// un-exchanged mass action): summed over ranks (fus_comm_allreduce, FUS_SUM) it is the squared L2
// norm the examples print (fem::assemble_scalar of u*u*dx, linear_planewave2d_1/main.cpp:151-157).
int fus_op_norm2(fus_op* op, const void* x, int space, double* out)
{
  if (!op || !x || !out)
    return fail(FUS_ERR_ARG, "null argument");
  const size_t ts = op->ts;
  std::vector<char> xh(op->ndofs * ts), yh(op->ndofs * ts, 0), ones(op->ncells * ts);
  if (space == FUS_HOST)
    memcpy(xh.data(), x, xh.size());
  else
  {
    HIPCHK(hipSetDevice(op->ctx->device));
    HIPCHK(hipMemcpy(xh.data(), x, xh.size(), hipMemcpyDeviceToHost));
  }
  for (int64_t i = 0; i < op->ncells; ++i)
    if (ts == 8)
      reinterpret_cast<double*>(ones.data())[i] = 1.0;
    else
      reinterpret_cast<float*>(ones.data())[i] = 1.0f;
  FUSCHK(fus_mass_apply(op, xh.data(), ones.data(), yh.data(), FUS_HOST));
  long double acc = 0;
  for (int64_t i = 0; i < op->ndofs; ++i)
    acc += ts == 8 ? (long double)reinterpret_cast<double*>(xh.data())[i] * reinterpret_cast<double*>(yh.data())[i]
                   : (long double)reinterpret_cast<float*>(xh.data())[i] * reinterpret_cast<float*>(yh.data())[i];
  *out = (double)acc;
  return FUS_OK;
}

int fus_op_get_geometry(fus_op* op, void* G, void* detJ)
{
  if (!op)
    return fail(FUS_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(op->ctx->device));
  return FUS_BY_DTYPE(op->dtype, op_get_geometry, op, G, detJ);
}

int fus_op_get_tables(fus_op* op, double* weights, double* dphi)
{
  if (!op)
    return fail(FUS_ERR_ARG, "null argument");
  if (weights)
    memcpy(weights, op->wts.data(), sizeof(double) * op->N);
  if (dphi)
    memcpy(dphi, op->D.data(), sizeof(double) * op->N * op->N);
  return FUS_OK;
}

static void layout_info(const Layout& L, size_t ts, int64_t out[8])
{
  out[0] = L.nblocks, out[1] = L.n_interior, out[2] = L.n_shared, out[3] = L.npairs;
  out[4] = L.max_nloc, out[5] = (int64_t)L.shapes.size();
  out[6] = (int64_t)L.lds_bytes(ts);
  out[7] = L.n_internal;
}

// which block kernel the operator runs, answered the way a launch decides it: the variant of the plain stiffness action
static BlockVariant op_variant(const fus_op* op) { return block_variant(op->facts, op->traits, OP_STIFFNESS, STAGE_NONE); }
int fus_op_is_affine(fus_op* op) { return (op && op->facts.mode == GEOM_AFFINE) ? 1 : 0; }
int fus_op_geometry_mode(fus_op* op) { return !op ? 0 : op->facts.mode; }
int fus_op_uses_mfma(fus_op* op) { return (op && op_variant(op).mf) ? 1 : 0; }
int fus_op_uses_diag_metric(fus_op* op) { return (op && op_variant(op).geom == GEOM_DIAG) ? 1 : 0; }
int fus_op_uses_mfma4(fus_op* op)
{
  if (!op)
    return 0;
  const BlockVariant v = op_variant(op);
  return uses_mf4(op->N, (int)op->ts, v.geom, v.mf) ? 1 : 0;
}
int fus_op_uses_pack32(fus_op* op) { return (op && op_variant(op).pk) ? 1 : 0; }
int fus_op_uses_block_loop(fus_op* op)
{
  if (!op)
    return 0;
  // what a launch with one workgroup per block runs, with as many inputs as the operator was created for (option "walk"
  // decides per launch, from the launch's number of blocks, whether it has fewer workgroups: not part of this answer)
  return block_walk(op->facts, op->traits, op_variant(op), op->nfields == 2 ? 2 : 1, false);
}

int fus_op_info(fus_op* op, int64_t out[8])
{
  if (!op || !out)
    return fail(FUS_ERR_ARG, "null argument");
  layout_info(op->L, op->ts, out);
  out[6] = (int64_t)op->lds_bytes;  // what the block kernel is launched with (fields, geometry mode)
  return FUS_OK;
}

int fus_layout_check(int P, int64_t ncells, int64_t ndofs, const int32_t* tensor_dofmap,
                     const double* centroids, int block_elems, int waves, int64_t out[8])
{
  return fus_layout_check_ex(3, P, ncells, ndofs, tensor_dofmap, centroids, block_elems, waves, nullptr, out);
}

int fus_layout_check_ex(int tdim, int P, int64_t ncells, int64_t ndofs, const int32_t* tensor_dofmap,
                        const double* centroids, int block_elems, int waves,
                        const uint8_t* force_shared, int64_t out[8])
{
  if (!tensor_dofmap || !centroids || !out)
    return fail(FUS_ERR_ARG, "null argument");
  Layout L;
  std::string err = build_layout(L, P, ncells, ndofs, tensor_dofmap, centroids, block_elems, waves,
                                 force_shared, tdim);
  if (!err.empty())
    return fail(FUS_ERR_ARG, "layout: " + err);
  err = verify_layout(L, tensor_dofmap);
  if (!err.empty())
    return fail(FUS_ERR_STATE, "layout verification: " + err);
  layout_info(L, 8, out);
  return FUS_OK;
}

int fus_op_set_neighbours(fus_op* op, int nneigh, const int32_t* ranks, const int64_t* counts,
                          const int32_t* dof_idx)
{
  if (!op || nneigh < 0 || (nneigh > 0 && (!ranks || !counts || !dof_idx)))
    return fail(FUS_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(op->ctx->device));
  hipStream_t st = op->ctx->stream;
  if (!op->neigh.empty())
    return fail(FUS_ERR_STATE, "neighbours already set");
  {
    // dofs other ranks hold as well are classified shared: rebuild the layout with that mask
    int64_t total = 0;
    for (int k = 0; k < nneigh; ++k)
      total += counts[k];
    std::vector<uint8_t> mask(op->ndofs, 0);
    for (int64_t j = 0; j < total; ++j)
    {
      if (dof_idx[j] < 0 || dof_idx[j] >= op->ndofs)
        return fail(FUS_ERR_ARG, "shared dof index out of range");
      mask[dof_idx[j]] = 1;
    }
    HIPCHK(hipStreamSynchronize(st));
    FUSCHK(op_build(op, mask.data()));
  }
  std::vector<std::pair<int, int>> order;  // (rank, k)
  std::vector<int64_t> off(nneigh + 1, 0);
  for (int k = 0; k < nneigh; ++k)
    off[k + 1] = off[k] + counts[k], order.emplace_back(ranks[k], k);
  std::sort(order.begin(), order.end());
  if (off[nneigh] > 2000000000ll)
    return fail(FUS_ERR_LIMIT, "halo exceeds int32 indexing");
  // concatenated neighbour lists in ascending rank order
  std::vector<int32_t> pack_idx;
  for (auto& rk : order)
  {
    const int k = rk.second;
    if (rk.first == op->ctx->rank)
      return fail(FUS_ERR_ARG, "a rank cannot be its own neighbour");
    Neigh nb;
    nb.rank = rk.first, nb.count = counts[k], nb.off = (int64_t)pack_idx.size();
    for (int64_t j = 0; j < nb.count; ++j)
      pack_idx.push_back(op->L.dof_perm[dof_idx[off[k] + j]]);
    op->neigh.push_back(nb);
  }
  op->n_halo = (int64_t)pack_idx.size();
  // unique interface dofs and, per dof, its addends in ascending rank order (own = -1)
  std::vector<int32_t> uniq(pack_idx);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  op->n_uidx = (int64_t)uniq.size();
  std::vector<std::vector<int32_t>> addends(uniq.size());
  for (size_t n = 0; n < op->neigh.size(); ++n)
  {
    const Neigh& nb = op->neigh[n];
    // the own partial goes before the first neighbour of higher rank
    const bool first_higher = nb.rank > op->ctx->rank
                              && (n == 0 || op->neigh[n - 1].rank < op->ctx->rank);
    if (first_higher)
      for (auto& a : addends)
        a.push_back(-1);
    for (int64_t j = 0; j < nb.count; ++j)
    {
      const size_t u = std::lower_bound(uniq.begin(), uniq.end(), pack_idx[nb.off + j]) - uniq.begin();
      addends[u].push_back((int32_t)(nb.off + j));
    }
  }
  if (op->neigh.empty() || op->neigh.back().rank < op->ctx->rank)
    for (auto& a : addends)
      a.push_back(-1);
  std::vector<int32_t> uptr(uniq.size() + 1, 0), usrc;
  for (size_t u = 0; u < uniq.size(); ++u)
  {
    // a dof not shared with the lower ranks still has its own partial in rank position: the -1
    // was appended for every dof at the right place above, so the list is already ordered
    uptr[u] = (int32_t)usrc.size();
    usrc.insert(usrc.end(), addends[u].begin(), addends[u].end());
  }
  uptr[uniq.size()] = (int32_t)usrc.size();
  auto up = [&](int32_t** d, const std::vector<int32_t>& v) -> int
  {
    HIPCHK(hipMalloc((void**)d, std::max<size_t>(1, v.size()) * sizeof(int32_t)));
    HIPCHK(hipMemcpy(*d, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return FUS_OK;
  };
  FUSCHK(up(&op->d_pack_idx, pack_idx));
  FUSCHK(up(&op->d_uidx, uniq));
  FUSCHK(up(&op->d_uptr, uptr));
  FUSCHK(up(&op->d_usrc, usrc));
  HIPCHK(hipMalloc(&op->d_sendbuf, std::max<size_t>(1, pack_idx.size()) * op->ts));
  HIPCHK(hipMalloc(&op->d_recvbuf, std::max<size_t>(1, pack_idx.size()) * op->ts));
  return FUS_OK;
}

// ---- in-process transport (single-GPU rehearsal of the multi-rank path) -----------------------
int fus_comm_init_local(fus_ctx** ctxs, int n)
{
  if (!ctxs || n < 1)
    return fail(FUS_ERR_ARG, "bad group");
  for (int i = 0; i < n; ++i)
  {
    if (!ctxs[i])
      return fail(FUS_ERR_ARG, "null ctx in group");
    ctxs[i]->rank = i, ctxs[i]->nranks = n, ctxs[i]->local_group = n > 1;
  }
  return FUS_OK;
}

// ---- external transport: the exchange is the caller's (the stage / setup halves: fus_model_*, wave.hip) ----------
int fus_op_halo_layout(fus_op* op, int* nneigh, int32_t* ranks, int64_t* counts, int64_t* offsets)
{
  if (!op || !nneigh)
    return fail(FUS_ERR_ARG, "null argument");
  *nneigh = (int)op->neigh.size();
  for (size_t k = 0; k < op->neigh.size(); ++k)
  {
    if (ranks)
      ranks[k] = op->neigh[k].rank;
    if (counts)
      counts[k] = op->neigh[k].count;
    if (offsets)
      offsets[k] = op->neigh[k].off;
  }
  return FUS_OK;
}

int fus_op_halo_buffers(fus_op* op, void** send_dev, void** recv_dev, int64_t* nvalues)
{
  if (!op)
    return fail(FUS_ERR_ARG, "null op");
  if (send_dev)
    *send_dev = op->d_sendbuf;
  if (recv_dev)
    *recv_dev = op->d_recvbuf;
  if (nvalues)
    *nvalues = op->n_halo;
  return FUS_OK;
}

// Measured streaming bandwidth of this device: triad y = x + a z over three arrays of nbytes each
// (16-byte accesses, all CUs), best of `reps` launches; GB/s counts 3 * nbytes per launch.
int fus_measure_bandwidth(fus_ctx* c, int64_t nbytes, int reps, double* gbps)
{
  if (!c || !gbps || nbytes < (1 << 20) || reps < 1)
    return fail(FUS_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  typedef double D2 __attribute__((ext_vector_type(2)));
  const int64_t nvec = nbytes / 16;
  D2 *x = nullptr, *y = nullptr;
  HIPCHK(hipMalloc(&x, nvec * 16));
  HIPCHK(hipMalloc(&y, nvec * 16));
  HIPCHK(hipMemsetAsync(x, 0, nvec * 16, c->stream));
  HIPCHK(hipMemsetAsync(y, 0, nvec * 16, c->stream));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int r = 0; r < reps + 1; ++r)  // first launch is a warm-up
  {
    HIPCHK(hipEventRecord(e0, c->stream));
    hipLaunchKernelGGL((k_stream_copy<D2>), dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, c->stream, nvec,
                       static_cast<const D2*>(x), y);
    HIPCHK(hipEventRecord(e1, c->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    if (r > 0 && ms < best)
      best = ms;
  }
  (void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
  (void)hipFree(x), (void)hipFree(y);
  *gbps = 2.0 * (double)(nvec * 16) / (best * 1e-3) / 1e9;   // bytes read + bytes written
  return FUS_OK;
}

int fus_profile_enable(fus_ctx* c, int on)
{
  if (!c)
    return fail(FUS_ERR_ARG, "null ctx");
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto& kv : c->profs)
    for (auto& ev : kv.second.ev)
      (void)hipEventDestroy(ev.first), (void)hipEventDestroy(ev.second);
  c->profs.clear();
  c->prof = on < 0 ? 0 : (on > 2 ? 1 : on);
  return FUS_OK;
}

int fus_profile_get(fus_ctx* c, const char* name, double* total_ms, int64_t* count)
{
  if (!c || !name)
    return fail(FUS_ERR_ARG, "null argument");
  HIPCHK(hipStreamSynchronize(c->stream));
  auto it = c->profs.find(name);
  double ms = 0;
  int64_t n = 0;
  if (it != c->profs.end())
  {
    Prof& p = it->second;
    for (auto& ev : p.ev)
    {
      float f = 0;
      HIPCHK(hipEventElapsedTime(&f, ev.first, ev.second));
      p.done_ms += f, p.done_count += 1;
      (void)hipEventDestroy(ev.first), (void)hipEventDestroy(ev.second);
    }
    p.ev.clear();
    ms = p.done_ms, n = p.done_count;
  }
  if (total_ms)
    *total_ms = ms;
  if (count)
    *count = n;
  return FUS_OK;
}

} // extern "C"
