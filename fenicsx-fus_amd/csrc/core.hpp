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
// handles
// -------------------------------------------------------------------------------------------------
// Of the wave model the bioheat unit reads what its two heat-load calls need: op, d_rho0, d_c0 and the monitor's d_mon,
// mon_n, mon_nharm, mon_every, mon_which.
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
  void* d_bsrc2 = nullptr;  // lossy: delta/(rho c^2) w_f on the source facets (dg term)
  void* mn1 = nullptr;      // Westervelt: diag of M(-2 beta/(rho^2 c^4)), internal numbering
  // boundary dofs (diagonal source / absorbing weights), sorted by internal index:
  // [0, nb_int) are block-interior (applied in the fused epilogue through d_blk_bnd_off),
  // [nb_int, nb) are shared dofs (their terms ride in pseudo partial slots: boundary_next / k_boundary_partial)
  int64_t nb = 0, nb_int = 0;
  int32_t* d_bidx = nullptr;
  int32_t* d_blk_bnd_off = nullptr;
  int32_t *d_sh_ptr32 = nullptr, *d_sh_pairs32 = nullptr;  // shared CSR incl. boundary pseudo pairs
  uint64_t* d_bnd_mask = nullptr;                           // rank-local shared dofs: boundary dof bits ...
  int32_t* d_bnd_base = nullptr;                            // ... and boundary dofs ahead of each 64-dof word
  void *d_bsrc = nullptr, *d_babs = nullptr;
  std::vector<void*> allocs;
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
  // receivers (fus_model_set_receivers): per point the internal indices of its cell's dofs and the 1-D basis
  // values at its reference coordinates; record buffer for sampling every k steps inside the RK loops
  int64_t rc_n = 0;
  int32_t* d_rc_idx = nullptr;
  void *d_rc_bas = nullptr, *d_rc_out = nullptr, *d_rec = nullptr;
  int rec_every = 0, rec_which = 0;
  int64_t rec_cap = 0, rec_n = 0, rec_step = 0;  // rec_cap: the records the last fus_model_record asked for
  int64_t rec_alloc = 0;                         // records d_rec has room for (it only grows)
  std::vector<double> rec_times;
  // field monitor (fus_model_monitor): per-DOF accumulator planes over the internal vector, one allocation --
  // T[2][n_internal] (max, min) then double[2 + 2 nharm][n_internal] (sum, sum of squares, cos_k, sin_k)
  void* d_mon = nullptr;
  size_t mon_bytes = 0;
  int mon_every = 0, mon_which = 0, mon_nharm = 0;
  double mon_freq = 0.0;
  int64_t mon_skip = 0, mon_count = 0, mon_step = 0, mon_n = 0;
  double mon_t_first = 0.0, mon_t_last = 0.0;
  // phased / apodised source (fus_model_set_source).  src_mode 0: the default source, d_bsrc / d_bsrc2 hold the facet
  // weights.  1: amplitude only -- the weights times the per-entry amplitude, folded in once; the scalar path stays.
  // 2: delays or a burst -- k_source_entries writes d_bsrc / d_bsrc2 = weights x per-entry waveform for a stage time and
  // the kernels get gval = dgval = 1.  d_src_base / d_src_base2 keep the unmodified weights, d_src_amp / d_src_tau the
  // per-entry amplitude and delay, all in boundary-entry order.  src_tn_int / src_tn_sh: the stage time the block-interior
  // entries [0, nb_int) and the shared entries [nb_int, nb) of d_bsrc hold (NaN: none).
  // 3: sampled drive signals (fus_model_set_source_signals) -- as 2, with k_source_entries_signal: d_src_chan is the
  // channel of every entry (-1: silent), renumbered in order of first use along the entry list, d_src_table the samples
  // time-major, double[nsamp][src_sig.nchan].
  int src_mode = 0;
  void *d_src_base = nullptr, *d_src_base2 = nullptr, *d_src_amp = nullptr, *d_src_tau = nullptr;
  int32_t* d_src_chan = nullptr;
  double* d_src_table = nullptr;
  fus::SourceSignal src_sig{};
  double src_dur = 0.0;
  double src_tn_int = NAN, src_tn_sh = NAN;
  // The facet weights as the setup produced them, sparse, by ascending internal index (exact in double for both scalar
  // types): what the entry lists are built from, at setup and again by fus_model_set_source_weights, whose weights
  // only ever add to the src part.
  std::vector<int32_t> h_fidx;
  std::vector<double> h_fsrc, h_fabs, h_fsrc2;
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

