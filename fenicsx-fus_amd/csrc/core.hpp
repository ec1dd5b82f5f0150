// core.hpp -- what the units compiled once share beyond host.hpp: fusmi.hip (the operator and its C ABI), wave.hip (the
// wave models and their C ABI) and thermal.hip (the bioheat model and its C ABI).  degree_unit.hip does not include it.
// Everything wave.hip and thermal.hip take from fusmi.hip is declared here, and nothing else of fusmi.hip has external
// linkage: this header is the list.  (The bioheat unit takes nothing from wave.hip but the fus_model fields named below.)
#ifndef FUS_CORE_HPP
#define FUS_CORE_HPP

#include <algorithm>
#include <cmath>
#include <cstring>

#include "host.hpp"
#include "source_signal.hpp"

// -------------------------------------------------------------------------------------------------
// owners of device memory
// -------------------------------------------------------------------------------------------------
// (The types below are FUS_HIDDEN: their inline members stay out of the library's dynamic symbols.)
// One device allocation and its owner: move-only, the destructor frees.  The rule of the units stays the caller's: the
// device is current, and the model's stream synchronised, before a buffer that a kernel may still read is reset, replaced
// or destroyed.
struct FUS_HIDDEN DevBuf
{
  void* p = nullptr;
  size_t bytes = 0;   // as asked for (the allocation itself is never shorter than 16 bytes)
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    if (this != &o)
    {
      reset();
      p = o.p, bytes = o.bytes;
      o.p = nullptr, o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset()
  {
    if (p)
      (void)hipFree(p);
    p = nullptr, bytes = 0;
  }
  explicit operator bool() const { return p != nullptr; }
  template <typename U>
  U* as() const
  {
    return static_cast<U*>(p);
  }
  // replaces what the buffer held by n bytes, uninitialised; a failure leaves it empty and the runtime without a sticky error
  int alloc(size_t n, const char* what)
  {
    reset();
    const hipError_t e = hipMalloc(&p, std::max<size_t>(n, 16));
    if (e != hipSuccess)
    {
      (void)hipGetLastError();
      p = nullptr;
      return fail(FUS_ERR_HIP, "cannot allocate " + std::to_string(n) + " bytes of " + what + ": " + hipGetErrorString(e));
    }
    bytes = n;
    return FUS_OK;
  }
};
template <typename U>
static int upload(DevBuf& b, const std::vector<U>& v, hipStream_t st, const char* what)
{
  FUSCHK(b.alloc(v.size() * sizeof(U), what));
  if (!v.empty())
    HIPCHK(hipMemcpyAsync(b.p, v.data(), b.bytes, hipMemcpyHostToDevice, st));
  return FUS_OK;
}

// The arrays a model allocates once, at setup or on the first use of a feature: freed with the model (dalloc,
// dalloc_bytes and upload below take it like the std::vector<void*> of fus_op::allocs)
struct FUS_HIDDEN DevPool : std::vector<void*>
{
  DevPool() = default;
  DevPool(const DevPool&) = delete;
  DevPool& operator=(const DevPool&) = delete;
  ~DevPool()
  {
    for (void* q : *this)
      (void)hipFree(q);
  }
};

// -------------------------------------------------------------------------------------------------
// handles
// -------------------------------------------------------------------------------------------------
// The parts of fus_model that a call between runs replaces as a whole.  Every array in them is a DevBuf, so a part is
// rebuilt beside the one in force and move-assigned once nothing can fail any more.

// The boundary-entry lists (model_build_entries, wave.hip): the dofs with a diagonal source / absorbing weight, sorted
// by internal index: [0, nb_int) are block-interior (applied in the fused epilogue through d_blk_bnd_off), [nb_int, nb)
// are shared dofs (their terms ride in pseudo partial slots: boundary_next / k_boundary_partial)
struct FUS_HIDDEN ModelEntries
{
  int64_t nb = 0, nb_int = 0;
  DevBuf d_bidx, d_blk_bnd_off;    // int32
  DevBuf d_sh_ptr32, d_sh_pairs32; // int32: shared CSR incl. boundary pseudo pairs
  DevBuf d_bnd_mask;               // uint64, rank-local shared dofs: boundary dof bits ...
  DevBuf d_bnd_base;               // int32 ... and boundary dofs ahead of each 64-dof word (both empty without such dofs)
  DevBuf d_bsrc, d_babs;           // T: the weights the kernels read
  DevBuf d_bsrc2;                  // T, lossy: delta/(rho c^2) w_f on the source facets (dg term); empty otherwise
};

// phased / apodised source (fus_model_set_source).  mode 0: the default source, d_bsrc / d_bsrc2 hold the facet weights.
// 1: amplitude only -- the weights times the per-entry amplitude, folded in once; the scalar path stays.
// 2: delays or a burst -- k_source_entries writes d_bsrc / d_bsrc2 = weights x per-entry waveform for a stage time and
// the kernels get gval = dgval = 1.  d.base / d.base2 keep the unmodified weights, d.amp / d.tau the per-entry amplitude
// and delay, all in boundary-entry order.  tn_int / tn_sh: the stage time the block-interior entries [0, nb_int) and the
// shared entries [nb_int, nb) of d_bsrc hold (NaN: none).
// 3: sampled drive signals (fus_model_set_source_signals) -- as 2, with k_source_entries_signal: d.chan is the channel
// of every entry (-1: silent), renumbered in order of first use along the entry list, d.table the samples time-major,
// double[nsamp][sig.nchan].
struct FUS_HIDDEN ModelSource
{
  int mode = 0;
  double dur = 0.0;
  struct Arrays
  {
    DevBuf base, base2, amp, tau;   // T
    DevBuf chan;                    // int32
    DevBuf table;                   // double
  } d;
  fus::SourceSignal sig{};
  double tn_int = NAN, tn_sh = NAN;
  // The facet weights as the setup produced them, sparse, by ascending internal index (exact in double for both scalar
  // types): what the entry lists are built from, at setup and again by fus_model_set_source_weights, whose weights
  // only ever add to the src part.
  std::vector<int32_t> h_fidx;
  std::vector<double> h_fsrc, h_fabs, h_fsrc2;
};

// receivers (fus_model_set_receivers): per point the internal indices of its cell's dofs and the 1-D basis values at its
// reference coordinates; record buffer for sampling every k steps inside the RK loops
struct FUS_HIDDEN ModelReceivers
{
  int64_t n = 0;
  DevBuf d_idx;          // int32
  DevBuf d_bas, d_out;   // T
  DevBuf d_rec;          // T: it only grows, until new receivers drop it
  int rec_every = 0, rec_which = 0;
  int64_t rec_cap = 0, rec_n = 0, rec_step = 0;  // rec_cap: the records the last fus_model_record asked for
  std::vector<double> rec_times;
};

// field monitor (fus_model_monitor): per-DOF accumulator planes over the internal vector, one allocation --
// T[2][n_internal] (max, min) then double[2 + 2 nharm][n_internal] (sum, sum of squares, cos_k, sin_k)
struct FUS_HIDDEN ModelMonitor
{
  DevBuf d_mon;
  int every = 0, which = 0, nharm = 0;
  double freq = 0.0;
  int64_t skip = 0, count = 0, step = 0, n = 0;
  double t_first = 0.0, t_last = 0.0;
};

// relaxation absorption (fus_model_set_relaxation): nrelax processes, per process one memory variable z_nu and one
// per-DOF strength A_nu, planes of n_internal T in one allocation each.  den: the lumped M(1/(rho c^2)) 1 kept while the
// sums over the sharers of an in-process group are pending (fus_group_relaxation_finish divides by it and frees it).
struct FUS_HIDDEN ModelRelax
{
  int nrelax = 0;
  double omega[4] = {0, 0, 0, 0};   // angular relaxation frequencies, 1/s
  DevBuf z, A;                      // T[nrelax][n_internal]
  DevBuf den;                       // T[n_internal], only while pending
  bool pending = false;
};

// absorbing layers (fus_model_set_sponge): the damping rate sigma per DOF in internal numbering (padding slots 0) and the
// ascending list of the tiles -- 256 16-byte vectors of the internal vector each -- that hold a nonzero sigma; the
// sub-step kernel runs over that list.  Off: both buffers empty, ntiles == 0.
struct FUS_HIDDEN ModelSponge
{
  DevBuf sigma;   // T[n_internal]
  DevBuf tiles;   // int32[ntiles]
  int64_t ntiles = 0, ntiles_total = 0, ndofs_active = 0;
};

// Of the wave model the bioheat unit reads what its two heat-load calls need: op, d_rho0, d_c0 and the monitor's
// mon.d_mon, mon.n, mon.nharm, mon.every, mon.which.
struct fus_model
{
  fus_ctx* ctx;
  fus_op* op;
  int kind;
  hipGraphExec_t gexec = nullptr;  // option "graph": the RK step as one executable graph (see d_model_step)
  int64_t gsteps = 0;              // steps taken since init / set (the first one is launched directly)
  double freq, amp, speed;
  void *u0 = nullptr, *v0 = nullptr, *u_ = nullptr, *v_ = nullptr, *un = nullptr, *vn = nullptr,
       *b = nullptr, *minv = nullptr, *m = nullptr, *coef = nullptr, *coef2 = nullptr;
  void* mn1 = nullptr;      // Westervelt: diag of M(-2 beta/(rho^2 c^4)), internal numbering
  DevPool allocs;           // what the setup allocated: the vectors above and the coefficients
  bool initialised = false;
  bool setup_done = false;
  int rk_order = 4;  // explicit Runge-Kutta scheme, tables of python/src/fenicsxfus/_linear.py:286-311
  int forms = 0;     // fus_ctx::forms at creation
  int lean_rk4 = 1;  // fus_ctx::lean_rk4 at creation
  // The boundary term of the shared boundary dofs rides in pseudo partial slots.  With RK4 the
  // shared-dof stage kernels write the NEXT stage's values there (boundary_next, wave_kernels.hpp);
  // bnd_valid / bnd_tn say for which stage time the slots are current, and stage_begin launches
  // k_boundary_partial only when they are not (first stage after init / set, other RK orders).
  bool bnd_valid = false;
  double bnd_tn = 0.0;
  ModelEntries bnd;
  ModelSource src;
  ModelReceivers rc;
  ModelMonitor mon;
  ModelRelax rx;
  ModelSponge sp;
  void* mcoef = nullptr;   // the mass coefficient 1/(rho c^2), internal cell order (the setup's; in allocs)
  // c0 and rho0 as fus_model_create was given them, internal cell order: fus_thermal_set_heat_from_monitor forms
  // q_coef = 2 alpha / (rho c) from them
  void *d_c0 = nullptr, *d_rho0 = nullptr;
};

// -------------------------------------------------------------------------------------------------
// small helpers
// -------------------------------------------------------------------------------------------------
template <typename U>
static int dalloc(std::vector<void*>& pool, U** p, size_t n)
{
  void* q = nullptr;
  HIPCHK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(U)));
  pool.push_back(q);
  *p = static_cast<U*>(q);
  return FUS_OK;
}
static int dalloc_bytes(std::vector<void*>& pool, void** p, size_t bytes, bool zero, hipStream_t st)
{
  void* q = nullptr;
  HIPCHK(hipMalloc(&q, std::max<size_t>(bytes, 16)));
  pool.push_back(q);
  if (zero)
    HIPCHK(hipMemsetAsync(q, 0, std::max<size_t>(bytes, 16), st));
  *p = q;
  return FUS_OK;
}
template <typename U>
static int upload(std::vector<void*>& pool, U** p, const std::vector<U>& v, hipStream_t st)
{
  FUSCHK(dalloc(pool, p, v.size()));
  if (!v.empty())
    HIPCHK(hipMemcpyAsync(*p, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice, st));
  return FUS_OK;
}
// fn<double>(...) or fn<float>(...) by a FUS_F64 / FUS_F32 scalar type
#define FUS_BY_DTYPE(dtype, fn, ...) ((dtype) == FUS_F64 ? fn<double>(__VA_ARGS__) : fn<float>(__VA_ARGS__))

struct ProfScope
{
  fus_ctx* c;
  Prof* p = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ProfScope(fus_ctx* c_, const char* name) : c(c_)
  {
    // level 1: every scope; level 2: the dominant kernel only ("stiffness", "stiffness_if") -- each
    // event record drains the queue between two kernels, so a timed run keeps them to a minimum
    bool take = c->prof == 1;
    if (c->prof == 2 && !strncmp(name, "stiffness", 9))
      take = (c->profs[name].seen++ % c->prof_sample) == 0;
    if (take)
    {
      p = &c->profs[name];
      (void)hipEventCreate(&e0), (void)hipEventCreate(&e1);
      (void)hipEventRecord(e0, c->stream);
    }
  }
  ~ProfScope()
  {
    if (p)
    {
      (void)hipEventRecord(e1, c->stream);
      p->ev.emplace_back(e0, e1);
    }
  }
};

// ---- fusmi.hip's typed functions as the wave and bioheat units call them, by the operator's scalar type (defined in fusmi.hip) ----
// The degree unit (degree_unit.hip, DegreeImpl in host.hpp) of a scalar type and degree: the wave models' stage_begin
// launches the block kernel with its fused stage epilogue through it
FUS_HIDDEN const DegreeImpl* degree_impl(int dtype, int P);
// b_internal = A x_internal on device vectors in internal numbering, coef in internal cell order; kind = OP_STIFFNESS | OP_MASS
FUS_HIDDEN int d_apply_internal(fus_op* op, int kind, const void* coef, const void* x, void* b);
// the shared-DOF exchange of a vector in its three phases, and all three back to back over RCCL (d_halo_sum)
FUS_HIDDEN int d_halo_pack(fus_op* op, const void* v);
FUS_HIDDEN int d_halo_unpack(fus_op* op, void* v);
FUS_HIDDEN int d_halo_sum(fus_op* op, void* v);
FUS_HIDDEN int halo_exchange_rccl(fus_op* op);
FUS_HIDDEN int halo_exchange_local(fus_op** ops, int n);

#endif

