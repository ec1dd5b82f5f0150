// thermal.hip -- the Pennes bioheat model and CEM43 dose (fusmi.h "bioheat"): the fus_thermal handle, its typed
// implementation and its C entry points, fus_thermal_* and fus_group_thermal_*.  The kernels are in thermal_kernels.hpp;
// what this unit takes from fusmi.hip (the operator) is listed in core.hpp, with the fields it reads of wave.hip's fus_model.
#include <memory>

#include "core.hpp"
#include "sts_coef.hpp"
#include "thermal_bc.hpp"
#include "thermal_kernels.hpp"
#include "thermal_owner.hpp"
#include "thermal_response.hpp"

using namespace fus;

// The boundary in force (fus_thermal_set_boundary; lists: thermal_bc.hpp): replaced as a whole
struct FUS_HIDDEN ThermalBoundary
{
  int64_t nfix = 0, nconv = 0;
  DevBuf fix_idx, conv_idx;          // int32
  DevBuf fix_val, conv_hw, conv_r;   // T
};

// The operator action runs through d_apply_internal (STAGE_NONE block kernel + shared reduction) on the thermal object's
// own vectors; of the op's scratch it takes d_partial (rewritten by every operator pass of any model; the wave models'
// pseudo boundary slots behind n_partial are not touched), d_tmp_c and d_tmp_coef -- never d_tmp_x, whose padding
// therefore stays zero.
struct fus_thermal
{
  fus_ctx* ctx = nullptr;
  fus_op* op = nullptr;
  double t_base = 37.0;
  // n_internal vectors of T: rise theta_0, stage input, accumulator, operator result, 1 / m_C, m_C, m_W, heat load h
  void *th0 = nullptr, *ths = nullptr, *acc = nullptr, *b = nullptr, *minv = nullptr, *mc = nullptr, *mw = nullptr,
       *h = nullptr;
  void *f0 = nullptr;          // F_0 of the super-time-stepping scheme: allocated by the first fus_thermal_steps_sts call
  void *kneg = nullptr;        // -k per cell, internal cell order
  double* dose = nullptr;      // CEM43 minutes, n_internal doubles
  double* d_stage = nullptr;   // ndofs doubles in caller numbering (dose in / out)
  // minv_bc: the copy of minv with zeros at the fixed DOFs that the stage and power kernels read while bc.nfix > 0,
  // allocated by the first call that fixes a DOF
  void* minv_bc = nullptr;
  ThermalBoundary bc;
  DevPool allocs;   // the vectors above, each allocated once
  bool initialised = false;
  // several ranks (fusmi.h "bioheat", several ranks): m_C, m_W, the heat weight and the fixed flags of the DOFs that other
  // ranks hold too are ordered sums over the sharers.  Under RCCL the call that forms them exchanges at once; in an
  // in-process group it leaves them `pending` for fus_group_thermal_finish.
  enum { PEND_SETUP = 1, PEND_HEAT = 2, PEND_BC = 4 };
  int pending = 0;
  // pending heat load: this rank's part of M(q_coef) 1, and q -- a T vector, or the monitor's sum-of-squares plane in
  // double with its sample count (qp_monitor) -- both n_internal long, allocated by the first call that needs them
  void *mq = nullptr, *qp = nullptr;
  bool qp_monitor = false;
  double qp_nsamp = 1.0;
  // the pending mq is this rank's part of the per-harmonic load itself (fus_thermal_set_heat_from_harmonics): the sum over
  // the sharers is then the load, and qp was only the scratch plane of the sum over the harmonics
  bool pend_load = false;
  // the boundary as this rank's caller gave it last (caller numbering; an empty vector: NULL): the agreement over the
  // sharers starts from it whenever any member of the group sets a boundary
  std::vector<uint8_t> rq_fixed;
  std::vector<char> rq_rise, rq_diag, rq_crise;
  // perfusion response and damage (fusmi.h "bioheat", perfusion response and damage; laws: thermal_response.hpp).  While a
  // response is set the stage kernels read mweff = m_W .* phi(theta_n, D_n) in place of mw; k_thermal_response rewrites it
  // after every step, together with Omega and r_prev, the damage rate at the state it saw.  respond_dirty: the state, the
  // response or the boundary changed since that kernel ran last, so the next steps call (or a read of the perfusion plane)
  // starts with a launch of it that only primes mweff and r_prev.
  fus::ThermalResponse resp;
  fus::ThermalDamage dmg;
  void* mweff = nullptr;   // T, n_internal: allocated by the first fus_thermal_set_response that sets a law
  DevBuf omega, rprev;     // double, n_internal: held while the damage is on
  bool respond_dirty = true;
};

static bool thermal_multi(const fus_thermal* th) { return !th->op->neigh.empty(); }
static bool thermal_in_group(const fus_thermal* th) { return thermal_multi(th) && th->ctx->local_group; }

// vec(th) becomes the ordered sum over the sharers at the interface DOFs, the same bits on all of them: over RCCL for a
// single object (nothing without neighbours), across the members of an in-process group otherwise
static int thermal_sum(fus_thermal** ths, int n, void* (*vec)(fus_thermal*))
{
  if (n == 1 && !ths[0]->ctx->local_group)
    return d_halo_sum(ths[0]->op, vec(ths[0]));
  std::vector<fus_op*> ops(n);
  for (int i = 0; i < n; ++i)
  {
    ops[i] = ths[i]->op;
    FUSCHK(d_halo_pack(ops[i], vec(ths[i])));
  }
  FUSCHK(halo_exchange_local(ops.data(), n));
  for (int i = 0; i < n; ++i)
    FUSCHK(d_halo_unpack(ops[i], vec(ths[i])));
  return FUS_OK;
}

// 1 / m_C as the stage and power kernels take it: zero at the fixed DOFs while there are any
static const void* thermal_minv(const fus_thermal* th) { return th->bc.nfix > 0 ? th->minv_bc : th->minv; }

// the perfusion plane as the stage kernels take it: m_W itself while no response is set
static const void* thermal_mw(const fus_thermal* th) { return th->resp.active() ? th->mweff : th->mw; }

// b += r - m_H x at the convective DOFs (r_too = false: the homogeneous part); nothing is enqueued without such DOFs
template <typename T>
static int thermal_robin(fus_thermal* th, const T* x, bool r_too)
{
  const ThermalBoundary& B = th->bc;
  if (B.nconv == 0)
    return FUS_OK;
  ProfScope ps(th->ctx, "thermal_bc");
  hipLaunchKernelGGL((k_thermal_robin<T>), dim3(nblk(B.nconv)), dim3(256), 0, th->ctx->stream, B.nconv,
                     B.conv_idx.as<const int32_t>(), B.conv_hw.as<const T>(), r_too ? B.conv_r.as<const T>() : nullptr, x,
                     static_cast<T*>(th->b));
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

// vec = the fixed values (zero_values: 0) at the fixed DOFs; with_minv: minv_bc = 0 there as well.  Nothing is enqueued
// without fixed DOFs
template <typename T>
static int thermal_impose(fus_thermal* th, void* vec, bool zero_values = false, bool with_minv = false)
{
  const ThermalBoundary& B = th->bc;
  if (B.nfix == 0)
    return FUS_OK;
  ProfScope ps(th->ctx, "thermal_fix");
  hipLaunchKernelGGL((k_thermal_fix<T>), dim3(nblk(B.nfix)), dim3(256), 0, th->ctx->stream, B.nfix,
                     B.fix_idx.as<const int32_t>(), zero_values ? nullptr : B.fix_val.as<const T>(), static_cast<T*>(vec),
                     with_minv ? static_cast<T*>(th->minv_bc) : nullptr);
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

template <typename T>
static int thermal_cells_to_internal(fus_thermal* th, const void* host_cells, T* out_i)
{
  fus_op* op = th->op;
  hipStream_t st = th->ctx->stream;
  T* cc = static_cast<T*>(op->d_tmp_coef);
  HIPCHK(hipMemcpyAsync(cc, host_cells, op->ncells * sizeof(T), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL((k_cells_to_internal<T>), dim3(nblk(op->ncells)), dim3(256), 0, st, op->ncells, op->d_cell_perm,
                     static_cast<const T*>(cc), out_i);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));   // host_cells may be a temporary of the caller
  return FUS_OK;
}

// out = M(coef_i) 1 (coef_i in internal cell order); acc serves as the vector of ones and is zeroed again
template <typename T>
static int thermal_lumped(fus_thermal* th, const T* coef_i, T* out)
{
  fus_op* op = th->op;
  hipStream_t st = th->ctx->stream;
  const int64_t n = op->L.n_internal;
  hipLaunchKernelGGL((k_fill<T>), dim3(1024), dim3(256), 0, st, n, static_cast<T*>(th->acc), T(1));
  HIPCHK(hipMemsetAsync(out, 0, n * sizeof(T), st));
  FUSCHK(d_apply_internal(op, OP_MASS, coef_i, th->acc, out));
  HIPCHK(hipMemsetAsync(th->acc, 0, n * sizeof(T), st));
  return FUS_OK;
}

// minv = 1 / m_C (0 in the padding slots), once m_C is complete
template <typename T>
static int thermal_setup_finish(fus_thermal* th)
{
  const int64_t n = th->op->L.n_internal;
  hipLaunchKernelGGL((k_reciprocal<T>), dim3(nblk(n)), dim3(256), 0, th->ctx->stream, n, static_cast<const T*>(th->mc),
                     static_cast<T*>(th->minv));
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

template <typename T>
static int thermal_setup(fus_thermal* th, const void* k_, const void* rc_, const void* w_)
{
  fus_op* op = th->op;
  hipStream_t st = th->ctx->stream;
  const int64_t n = op->L.n_internal, nc = op->ncells;
  const T *kc = static_cast<const T*>(k_), *rc = static_cast<const T*>(rc_), *wc = static_cast<const T*>(w_);
  for (int64_t e = 0; e < nc; ++e)
  {
    if (!(rc[e] > T(0)) || !std::isfinite((double)rc[e]))
      return fail(FUS_ERR_ARG, "fus_thermal_create: rho_c must be positive and finite in every cell");
    if (!(kc[e] >= T(0)) || !std::isfinite((double)kc[e]))
      return fail(FUS_ERR_ARG, "fus_thermal_create: conductivity must be >= 0 and finite in every cell");
    if (wc && (!(wc[e] >= T(0)) || !std::isfinite((double)wc[e])))
      return fail(FUS_ERR_ARG, "fus_thermal_create: perfusion must be >= 0 and finite in every cell");
  }
  for (void** v : {&th->th0, &th->ths, &th->acc, &th->b, &th->minv, &th->mc, &th->mw, &th->h})
    FUSCHK(dalloc_bytes(th->allocs, v, n * sizeof(T), true, st));
  void* dz = nullptr;
  FUSCHK(dalloc_bytes(th->allocs, &dz, n * sizeof(double), true, st));
  th->dose = static_cast<double*>(dz);
  FUSCHK(dalloc_bytes(th->allocs, &dz, op->ndofs * sizeof(double), true, st));
  th->d_stage = static_cast<double*>(dz);
  FUSCHK(dalloc_bytes(th->allocs, &th->kneg, nc * sizeof(T), false, st));
  T* ci = static_cast<T*>(th->kneg);   // per-cell staging until -k takes it
  FUSCHK(thermal_cells_to_internal<T>(th, rc, ci));
  FUSCHK(thermal_lumped<T>(th, ci, static_cast<T*>(th->mc)));
  // several ranks: 1 / m_C is formed from the sum over the sharers -- here over RCCL, in a group by fus_group_thermal_finish
  const bool rccl = thermal_multi(th) && !th->ctx->local_group;
  if (rccl)
    FUSCHK(d_halo_sum(op, th->mc));
  if (!thermal_in_group(th))
    FUSCHK(thermal_setup_finish<T>(th));
  if (wc)
  {
    FUSCHK(thermal_cells_to_internal<T>(th, wc, ci));
    FUSCHK(thermal_lumped<T>(th, ci, static_cast<T*>(th->mw)));
  }
  if (rccl)   // collective: also where this rank has no perfusion
    FUSCHK(d_halo_sum(op, th->mw));
  if (thermal_in_group(th))
    th->pending |= fus_thermal::PEND_SETUP;
  std::vector<T> kn(nc);
  for (int64_t e = 0; e < nc; ++e)
    kn[e] = -kc[e];
  FUSCHK(thermal_cells_to_internal<T>(th, kn.data(), ci));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

// grid and 16-byte vector count of a streaming pass over the whole vectors, or (local) over the DOFs no other rank holds:
// [0, n_int_pad + n_if_start_pad), a multiple of 16 elements -- the interface DOFs behind it wait for the exchange
template <typename T>
static unsigned thermal_grid(const fus_thermal* th, int64_t* nvec, bool local = false)
{
  const Layout& L = th->op->L;
  *nvec = (local ? L.n_int_pad + L.n_if_start_pad : L.n_internal) / (16 / (int64_t)sizeof(T));
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((*nvec + 255) / 256, (int64_t)th->ctx->num_cus * 8));
}

// The launch behind the perfusion response and the damage (k_thermal_response), over all n_internal slots: after a step of
// size dt, or (prime) before the first step after something it reads from changed.  Nothing is enqueued while both are off.
template <typename T>
static int thermal_respond(fus_thermal* th, double dt, bool prime)
{
  const int mode = (th->resp.active() ? 1 : 0) | (th->dmg.on() ? 2 : 0);
  if (mode == 0)
    return FUS_OK;
  ThermalRespond<T> A;
  A.th = static_cast<const T*>(th->th0), A.dose = th->dose, A.mw = static_cast<const T*>(th->mw);
  A.mweff = static_cast<T*>(th->mweff), A.omega = th->omega.as<double>(), A.rprev = th->rprev.as<double>();
  A.R = th->resp, A.lnA = th->dmg.lnA, A.Ea = th->dmg.Ea, A.dt2 = dt / 2.0, A.t_base = th->t_base;
  A.prime = prime ? 1 : 0;
  int64_t nvec;
  const unsigned grid = thermal_grid<T>(th, &nvec);
  ProfScope ps(th->ctx, "thermal_response");
  return with_kind<1, 2, 3>(mode, [&](auto M) -> int
  {
    hipLaunchKernelGGL((k_thermal_response<T, decltype(M)::value>), dim3(grid), dim3(256), 0, th->ctx->stream, nvec, A);
    HIPCHK(hipGetLastError());
    return FUS_OK;
  });
}

template <typename T>
static int thermal_prime(fus_thermal* th)
{
  if (th->respond_dirty)
    FUSCHK(thermal_respond<T>(th, 0.0, true));
  th->respond_dirty = false;
  return FUS_OK;
}

// First half of a stage of either scheme: b = K(-k) x, the convective term, and on several ranks the pack of this rank's
// totals of the interface DOFs into the send buffer (the event hands it to the exchange)
template <typename T>
static int thermal_stage_begin(fus_thermal* th, const void* x)
{
  FUSCHK(d_apply_internal(th->op, OP_STIFFNESS, th->kneg, x, th->b));
  FUSCHK(thermal_robin<T>(th, static_cast<const T*>(x), true));
  if (thermal_multi(th))
  {
    ProfScope ps(th->ctx, "halo");
    FUSCHK(d_halo_pack(th->op, th->b));
  }
  return FUS_OK;
}

// the kernel families of the two schemes: stage kinds, profile scope of the streaming launch, and the two kernels by kind
struct ThermalRk4
{
  using Kinds = std::integer_sequence<int, STAGE_FIRST, STAGE_MID, STAGE_LAST>;
  static constexpr const char* scope = "thermal";
  template <typename T, int K> static constexpr auto stream = &k_thermal_stage<T, K>;
  template <typename T, int K> static constexpr auto iface = &k_thermal_if_stage<T, K>;
};
struct ThermalRkl2
{
  using Kinds = std::integer_sequence<int, 0, 1, 2>;   // first, middle, last stage of the step (k_thermal_sts_stage)
  static constexpr const char* scope = "thermal_sts";
  template <typename T, int K> static constexpr auto stream = &k_thermal_sts_stage<T, K>;
  template <typename T, int K> static constexpr auto iface = &k_thermal_if_sts_stage<T, K>;
};

// Second half of a stage of either scheme, from a kernel family F, a stage kind and the family's argument struct: the
// streaming kernel over the DOFs no other rank holds, and on several ranks, once the sharers' totals have arrived, the
// interface kernel with the same arguments
template <typename T, typename F, typename Args>
static int thermal_stage_end(fus_thermal* th, int kind, const Args& A)
{
  fus_op* op = th->op;
  fus_ctx* c = th->ctx;
  const bool multi = thermal_multi(th);
  int64_t nvec;
  const unsigned grid = thermal_grid<T>(th, &nvec, multi);
  return with_kind(kind, [&](auto K) -> int
  {
    {
      ProfScope ps(c, F::scope);
      hipLaunchKernelGGL((F::template stream<T, decltype(K)::value>), dim3(grid), dim3(256), 0, c->stream, nvec, A);
      HIPCHK(hipGetLastError());
    }
    if (multi)
    {
      if (!c->local_group)
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_recv, 0));
      ProfScope ps(c, "thermal_if");
      hipLaunchKernelGGL((F::template iface<T, decltype(K)::value>), dim3(nblk(op->n_uidx)), dim3(256), 0, c->stream, op->n_uidx,
                         op->d_uidx, op->d_uptr, op->d_usrc, static_cast<const T*>(op->d_recvbuf), A);
      HIPCHK(hipGetLastError());
    }
    return FUS_OK;
  }, typename F::Kinds{});
}

// classical RK4 (a = 0, 1/2, 1/2, 1; b = 1/6, 1/3, 1/3, 1/6), stage i: per stage the operator's two launches and
// k_thermal_stage; on several ranks that kernel covers the rank's own DOFs while the exchange is in flight, and
// k_thermal_if_stage finishes the interface DOFs from the received totals
static const void* thermal_rk4_input(const fus_thermal* th, int i) { return i == 0 ? th->th0 : th->ths; }

template <typename T>
static int thermal_rk4_end(fus_thermal* th, int i, double dt_, double sigma)
{
  const T dt = (T)dt_;
  const T a_next[4] = {T(0.5), T(0.5), T(1), T(0)};
  const T b_runge[4] = {(T)(1.0 / 6.0), (T)(1.0 / 3.0), (T)(1.0 / 3.0), (T)(1.0 / 6.0)};
  ThermalStage<T> A;
  A.b = static_cast<const T*>(th->b), A.th_in = static_cast<const T*>(thermal_rk4_input(th, i));
  A.th_out = static_cast<T*>(i == 3 ? th->th0 : th->ths);
  A.th0 = static_cast<const T*>(th->th0), A.acc = static_cast<T*>(th->acc);
  A.minv = static_cast<const T*>(thermal_minv(th)), A.mw = static_cast<const T*>(thermal_mw(th)), A.h = static_cast<const T*>(th->h);
  A.dose = th->dose;
  A.adt = dt * a_next[i], A.bdt = dt * b_runge[i], A.sigma = (T)sigma;
  A.dt60 = dt_ / 60.0, A.t_base = th->t_base;
  return thermal_stage_end<T, ThermalRk4>(th, i == 0 ? STAGE_FIRST : (i < 3 ? STAGE_MID : STAGE_LAST), A);
}

// RKL2 of c.s stages (sts_coef.hpp), stage j = 1..s: per stage the operator's two launches and k_thermal_sts_stage (on
// several ranks split like an RK4 stage, k_thermal_if_sts_stage on the interface DOFs).  Y_0 stays in th0 until the last
// stage overwrites it, F_0 sits in f0, and Y_1, Y_2, ... alternate between ths and acc: Y_j lands where Y_{j-2} was,
// except Y_2, whose Y_{j-2} is Y_0
static const void* thermal_sts_input(const fus_thermal* th, int j) { return j == 1 ? th->th0 : ((j - 2) & 1 ? th->acc : th->ths); }

template <typename T>
static int thermal_sts_end(fus_thermal* th, int j, double dt_, double sigma, const fus::StsCoef& c)
{
  T* rot[2] = {static_cast<T*>(th->ths), static_cast<T*>(th->acc)};
  T* th0 = static_cast<T*>(th->th0);
  ThermalSts<T> A;
  A.b = static_cast<const T*>(th->b), A.y1 = static_cast<const T*>(thermal_sts_input(th, j));
  A.y2 = j <= 2 ? th0 : rot[(j - 1) & 1];
  A.y0 = th0, A.f0 = static_cast<T*>(th->f0);
  A.out = j == c.s ? th0 : rot[(j - 1) & 1];
  A.minv = static_cast<const T*>(thermal_minv(th)), A.mw = static_cast<const T*>(thermal_mw(th)), A.h = static_cast<const T*>(th->h);
  A.dose = th->dose;
  A.mu = (T)c.mu[j], A.nu = (T)c.nu[j], A.om = (T)(1.0 - c.mu[j] - c.nu[j]);
  A.mdt = (T)(c.mut[j] * dt_), A.gdt = (T)(c.gat[j] * dt_), A.sigma = (T)sigma;
  A.dt120 = dt_ / 120.0, A.t_base = th->t_base;
  return thermal_stage_end<T, ThermalRkl2>(th, j == 1 ? 0 : (j < c.s ? 1 : 2), A);
}

// nsteps steps of RK4 (stages == 0) or of RKL2 with `stages` stages (which the caller has checked), on a single object --
// one rank, or several over RCCL -- or on the n members of an in-process group.  Per stage: the first halves of all members
// (they end with the pack), the exchange, the second halves.
template <typename T>
static int thermal_run(fus_thermal** ths, int n, double dt, int64_t nsteps, double sigma, int stages)
{
  fus::StsCoef coef;
  if (stages != 0 && !fus::sts_coefficients(stages, &coef))
    return fail(FUS_ERR_ARG, "thermal_run: stages must be 0 (RK4) or lie in 2..32");
  const bool rccl = n == 1 && !ths[0]->ctx->local_group;   // as thermal_sum decides
  std::vector<fus_op*> ops(n);
  for (int i = 0; i < n; ++i)
    ops[i] = ths[i]->op;
  for (int i = 0; i < n; ++i)
    FUSCHK(thermal_prime<T>(ths[i]));
  for (int64_t s = 0; s < nsteps; ++s)
  {
    for (int st = 0; st < (stages == 0 ? 4 : stages); ++st)
    {
      for (int i = 0; i < n; ++i)
        FUSCHK(thermal_stage_begin<T>(ths[i], stages == 0 ? thermal_rk4_input(ths[i], st) : thermal_sts_input(ths[i], st + 1)));
      if (!rccl)
        FUSCHK(halo_exchange_local(ops.data(), n));
      else if (thermal_multi(ths[0]))   // the RCCL exchange on the comm stream (nothing without neighbours)
      {
        ProfScope ps(ths[0]->ctx, "halo");
        FUSCHK(halo_exchange_rccl(ops[0]));
      }
      for (int i = 0; i < n; ++i)
        FUSCHK(stages == 0 ? thermal_rk4_end<T>(ths[i], st, dt, sigma) : thermal_sts_end<T>(ths[i], st + 1, dt, sigma, coef));
    }
    // RKL2: a fixed DOF passes through mu Y + nu Y + om Y in every stage, which returns Y only up to rounding (RK4's stages
    // add an exact zero instead): one sparse launch per step puts the values back, so that they hold exactly here too
    if (stages != 0)
      for (int i = 0; i < n; ++i)
        FUSCHK(thermal_impose<T>(ths[i], ths[i]->th0));
    // phi of the next step from (theta_{n+1}, D_{n+1}), and the damage of this one
    for (int i = 0; i < n; ++i)
      FUSCHK(thermal_respond<T>(ths[i], dt, false));
  }
  for (int i = 0; i < n; ++i)
    HIPCHK(hipStreamSynchronize(ths[i]->ctx->stream));
  return FUS_OK;
}

// h = M(qcoef_i) 1 .* q: q a T vector in internal numbering (q_i), or Q / nsamp from the monitor's plane (Q)
template <typename T>
static int thermal_heat(fus_thermal* th, const T* qcoef_i, const T* q_i, const double* Q, double nsamp)
{
  fus_op* op = th->op;
  hipStream_t st = th->ctx->stream;
  const int64_t n = op->L.n_internal;
  T* mq = static_cast<T*>(th->b);
  FUSCHK(thermal_lumped<T>(th, qcoef_i, mq));
  if (thermal_in_group(th))
  {
    // the weight waits for the sharers' parts: keep it and q until fus_group_thermal_finish; h stays as it was
    if (!th->mq)
      FUSCHK(dalloc_bytes(th->allocs, &th->mq, n * sizeof(T), true, st));
    if (!th->qp)
      FUSCHK(dalloc_bytes(th->allocs, &th->qp, n * sizeof(double), true, st));
    HIPCHK(hipMemcpyAsync(th->mq, mq, n * sizeof(T), hipMemcpyDeviceToDevice, st));
    if (q_i)
      HIPCHK(hipMemcpyAsync(th->qp, q_i, n * sizeof(T), hipMemcpyDeviceToDevice, st));
    else
      HIPCHK(hipMemcpyAsync(th->qp, Q, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    th->qp_monitor = q_i == nullptr, th->qp_nsamp = nsamp, th->pend_load = false;
    th->pending |= fus_thermal::PEND_HEAT;
  }
  else
  {
    if (thermal_multi(th))
      FUSCHK(d_halo_sum(op, mq));
    int64_t nvec;
    const unsigned grid = thermal_grid<T>(th, &nvec);
    hipLaunchKernelGGL((k_thermal_heat<T>), dim3(grid), dim3(256), 0, st, nvec, static_cast<const T*>(mq), q_i, Q, nsamp,
                       static_cast<T*>(th->h));
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemsetAsync(th->b, 0, n * sizeof(T), st));
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

// the pending heat load of a group member, once its weight holds the sharers' parts
template <typename T>
static int thermal_heat_finish(fus_thermal* th)
{
  if (th->pend_load)   // per-harmonic load: the sharers' parts of h itself have been summed
  {
    HIPCHK(hipMemcpyAsync(th->h, th->mq, th->op->L.n_internal * sizeof(T), hipMemcpyDeviceToDevice, th->ctx->stream));
    return FUS_OK;
  }
  int64_t nvec;
  const unsigned grid = thermal_grid<T>(th, &nvec);
  hipLaunchKernelGGL((k_thermal_heat<T>), dim3(grid), dim3(256), 0, th->ctx->stream, nvec, static_cast<const T*>(th->mq),
                     th->qp_monitor ? nullptr : static_cast<const T*>(th->qp),
                     th->qp_monitor ? static_cast<const double*>(th->qp) : nullptr, th->qp_nsamp, static_cast<T*>(th->h));
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

template <typename T>
static int thermal_set_heat(fus_thermal* th, const void* q, const void* q_coef, int space)
{
  fus_op* op = th->op;
  hipStream_t st = th->ctx->stream;
  const int64_t n = op->L.n_internal, nc = op->ncells;
  if (!q)
  {
    HIPCHK(hipMemsetAsync(th->h, 0, n * sizeof(T), st));
    HIPCHK(hipStreamSynchronize(st));
    th->pending &= ~fus_thermal::PEND_HEAT;   // a load that waited for the sharers is dropped with it
    return FUS_OK;
  }
  T* cc = static_cast<T*>(op->d_tmp_coef);
  T* ci = cc + nc;
  if (!q_coef)
    hipLaunchKernelGGL((k_fill<T>), dim3(nblk(nc)), dim3(256), 0, st, nc, ci, T(1));
  else
  {
    const T* src = static_cast<const T*>(q_coef);
    if (space == FUS_HOST)
    {
      HIPCHK(hipMemcpyAsync(cc, q_coef, nc * sizeof(T), hipMemcpyHostToDevice, st));
      src = cc;
    }
    hipLaunchKernelGGL((k_cells_to_internal<T>), dim3(nblk(nc)), dim3(256), 0, st, nc, op->d_cell_perm, src, ci);
  }
  // q in internal numbering: the stage input's place is free between steps (its padding stays zero)
  const T* qs = static_cast<const T*>(q);
  T* tc = static_cast<T*>(op->d_tmp_c);
  if (space == FUS_HOST)
  {
    HIPCHK(hipMemcpyAsync(tc, q, op->ndofs * sizeof(T), hipMemcpyHostToDevice, st));
    qs = tc;
  }
  T* qi = static_cast<T*>(th->ths);
  hipLaunchKernelGGL((k_to_internal<T>), dim3(nblk(op->ndofs)), dim3(256), 0, st, op->ndofs, op->d_dof_perm, qs, qi);
  HIPCHK(hipGetLastError());
  FUSCHK(thermal_heat<T>(th, ci, qi, nullptr, 1.0));
  HIPCHK(hipMemsetAsync(th->ths, 0, n * sizeof(T), st));
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

template <typename T>
static int thermal_heat_from_monitor(fus_thermal* th, fus_model* m, const void* absorption)
{
  fus_op* op = th->op;
  hipStream_t st = th->ctx->stream;
  const int64_t n = op->L.n_internal, nc = op->ncells;
  const T* al = static_cast<const T*>(absorption);
  for (int64_t e = 0; e < nc; ++e)
    if (!(al[e] >= T(0)) || !std::isfinite((double)al[e]))
      return fail(FUS_ERR_ARG, "fus_thermal_set_heat_from_monitor: absorption must be >= 0 and finite in every cell");
  T* cc = static_cast<T*>(op->d_tmp_coef);
  T* ci = cc + nc;
  HIPCHK(hipMemcpyAsync(cc, al, nc * sizeof(T), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL((k_cells_to_internal<T>), dim3(nblk(nc)), dim3(256), 0, st, nc, op->d_cell_perm,
                     static_cast<const T*>(cc), ci);
  hipLaunchKernelGGL((k_thermal_qcoef<T>), dim3(nblk(nc)), dim3(256), 0, st, nc, static_cast<const T*>(ci),
                     static_cast<const T*>(m->d_rho0), static_cast<const T*>(m->d_c0), cc);
  HIPCHK(hipGetLastError());
  const double* Q = reinterpret_cast<const double*>(m->mon.d_mon.as<const T>() + 2 * n) + n;   // acc plane 1
  return thermal_heat<T>(th, cc, nullptr, Q, (double)m->mon.n);
}

// h = sum_k M(2 alpha_k / (rho c)) 1 .* (2 / n^2) (C_k^2 + S_k^2) over the harmonics 1..nharm of the model's monitor
// (fusmi.h "bioheat", per-harmonic heat load): per harmonic the lumped weight into b and one launch of
// k_thermal_heat_harmonic, which carries the sum in the double plane qp.  Several ranks: the sharers' parts of h are
// summed -- at once over RCCL, by fus_group_thermal_finish in a group, where the part waits in mq.
template <typename T>
static int thermal_heat_from_harmonics(fus_thermal* th, fus_model* m, int nharm, const void* absorption)
{
  fus_op* op = th->op;
  hipStream_t st = th->ctx->stream;
  const int64_t n = op->L.n_internal, nc = op->ncells;
  const T* al = static_cast<const T*>(absorption);
  for (int64_t e = 0; e < (int64_t)nharm * nc; ++e)
    if (!(al[e] >= T(0)) || !std::isfinite((double)al[e]))
      return fail(FUS_ERR_ARG, "fus_thermal_set_heat_from_harmonics: absorption must be >= 0 and finite in every cell and row");
  const bool group = thermal_in_group(th);
  if (nharm > 1 && !th->qp)
    FUSCHK(dalloc_bytes(th->allocs, &th->qp, n * sizeof(double), true, st));
  if (group && !th->mq)
    FUSCHK(dalloc_bytes(th->allocs, &th->mq, n * sizeof(T), true, st));
  T* cc = static_cast<T*>(op->d_tmp_coef);
  T* ci = cc + nc;
  T* mk = static_cast<T*>(th->b);
  T* out = static_cast<T*>(group ? th->mq : th->h);   // in a group h stays as it was until the finish
  const double* acc = reinterpret_cast<const double*>(m->mon.d_mon.as<const T>() + 2 * n);
  const double ns = (double)m->mon.n;
  int64_t nvec;
  const unsigned grid = thermal_grid<T>(th, &nvec);
  for (int k = 1; k <= nharm; ++k)
  {
    HIPCHK(hipMemcpyAsync(cc, al + (int64_t)(k - 1) * nc, nc * sizeof(T), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_cells_to_internal<T>), dim3(nblk(nc)), dim3(256), 0, st, nc, op->d_cell_perm,
                       static_cast<const T*>(cc), ci);
    hipLaunchKernelGGL((k_thermal_qcoef<T>), dim3(nblk(nc)), dim3(256), 0, st, nc, static_cast<const T*>(ci),
                       static_cast<const T*>(m->d_rho0), static_cast<const T*>(m->d_c0), cc);
    HIPCHK(hipGetLastError());
    FUSCHK(thermal_lumped<T>(th, cc, mk));
    hipLaunchKernelGGL((k_thermal_heat_harmonic<T>), dim3(grid), dim3(256), 0, st, nvec, static_cast<const T*>(mk),
                       acc + (size_t)(1 + k) * n, acc + (size_t)(1 + m->mon.nharm + k) * n, static_cast<double*>(th->qp),
                       k == 1 ? 1 : 0, k == nharm ? 2.0 / (ns * ns) : 0.0, out);
    HIPCHK(hipGetLastError());
  }
  if (group)
  {
    th->pend_load = true;
    th->pending |= fus_thermal::PEND_HEAT;
  }
  else if (thermal_multi(th))
    FUSCHK(d_halo_sum(op, out));
  HIPCHK(hipMemsetAsync(th->b, 0, n * sizeof(T), st));
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

template <typename T>
static int thermal_vec(fus_thermal* th, int which, void* host_or_dev, int space, bool set)
{
  fus_op* op = th->op;
  hipStream_t st = th->ctx->stream;
  const int64_t nd = op->ndofs;
  if (which == FUS_TH_DOSE || which == FUS_TH_DAMAGE)
  {
    double* plane = which == FUS_TH_DOSE ? th->dose : th->omega.as<double>();
    double* stg = th->d_stage;
    if (set)
    {
      const double* src = static_cast<const double*>(host_or_dev);
      if (space == FUS_HOST)
      {
        HIPCHK(hipMemcpyAsync(stg, host_or_dev, nd * sizeof(double), hipMemcpyHostToDevice, st));
        src = stg;
      }
      hipLaunchKernelGGL((k_to_internal<double>), dim3(nblk(nd)), dim3(256), 0, st, nd, op->d_dof_perm, src, plane);
    }
    else
    {
      double* dst = space == FUS_HOST ? stg : static_cast<double*>(host_or_dev);
      hipLaunchKernelGGL((k_from_internal<double, 0>), dim3(nblk(nd)), dim3(256), 0, st, nd, op->d_dof_perm,
                         static_cast<const double*>(plane), dst);
      if (space == FUS_HOST)
        HIPCHK(hipMemcpyAsync(host_or_dev, stg, nd * sizeof(double), hipMemcpyDeviceToHost, st));
    }
  }
  else
  {
    // (the perfusion plane is only read)
    T* vec = static_cast<T*>(which == FUS_TH_RISE ? th->th0 : (which == FUS_TH_HEAT ? th->h : const_cast<void*>(thermal_mw(th))));
    T* tc = static_cast<T*>(op->d_tmp_c);
    if (set)
    {
      const T* src = static_cast<const T*>(host_or_dev);
      if (space == FUS_HOST)
      {
        HIPCHK(hipMemcpyAsync(tc, host_or_dev, nd * sizeof(T), hipMemcpyHostToDevice, st));
        src = tc;
      }
      hipLaunchKernelGGL((k_to_internal<T>), dim3(nblk(nd)), dim3(256), 0, st, nd, op->d_dof_perm, src, vec);
      HIPCHK(hipGetLastError());
      FUSCHK(thermal_impose<T>(th, vec));   // the rise: fus_thermal_set refuses FUS_TH_HEAT
    }
    else
    {
      T* dst = space == FUS_HOST ? tc : static_cast<T*>(host_or_dev);
      hipLaunchKernelGGL((k_from_internal<T, 0>), dim3(nblk(nd)), dim3(256), 0, st, nd, op->d_dof_perm,
                         static_cast<const T*>(vec), dst);
      if (space == FUS_HOST)
        HIPCHK(hipMemcpyAsync(host_or_dev, tc, nd * sizeof(T), hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

// Power iteration for lambda_max of m_C^-1 (K(k) + diag(phi_max m_W + m_H)) (phi_max: the largest factor of the perfusion
// response, 1 without one) with the rows and columns of the fixed DOFs removed
// (the start vector is zero there, and so is every iterate: minv_bc).  Setup-time work: the operator and the quotient
// y = (K(k) x + m_W x + m_H x) / m_C run on the device, y is pulled, the three m_C-weighted dot products and the normalisation
// are done on the host in double, and the next x is pushed back.
// Several ranks -- one object under RCCL, or the n members of an in-process group: every rank starts from its own
// 1 + 0.5 sin(37 d + 1) over its own DOF numbers, one ordered sum makes the start the same on all sharers of a DOF, every
// operator result is summed over the sharers, the dot products count a DOF on the rank that owns it (thermal_owner.hpp)
// and their three sums are added over the ranks before the quotient is formed: every rank gets the same double.
template <typename T>
static int thermal_lambda_max(fus_thermal** ths, int n, int iters, double* lambda)
{
  struct Member
  {
    std::vector<T> x, y, mc;
    std::vector<uint8_t> own;   // empty: every DOF is this rank's
  };
  std::vector<Member> M(n);
  for (int i = 0; i < n; ++i)
  {
    fus_thermal* th = ths[i];
    fus_op* op = th->op;
    hipStream_t st = th->ctx->stream;
    const int64_t ni = op->L.n_internal, nd = op->ndofs;
    std::vector<T> xc(nd);
    for (int64_t d = 0; d < nd; ++d)
      xc[d] = (T)(1.0 + 0.5 * std::sin(37.0 * (double)d + 1.0));
    T* tc = static_cast<T*>(op->d_tmp_c);
    T* xd = static_cast<T*>(th->ths);   // the stage input's place is free between steps
    HIPCHK(hipMemsetAsync(xd, 0, ni * sizeof(T), st));
    HIPCHK(hipMemcpyAsync(tc, xc.data(), nd * sizeof(T), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_to_internal<T>), dim3(nblk(nd)), dim3(256), 0, st, nd, op->d_dof_perm, static_cast<const T*>(tc), xd);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // xc leaves scope
    if (thermal_multi(th))
    {
      std::vector<int32_t> uidx(op->n_uidx), uptr(op->n_uidx + 1), usrc;
      HIPCHK(hipMemcpy(uidx.data(), op->d_uidx, uidx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(uptr.data(), op->d_uptr, uptr.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      usrc.resize((size_t)uptr.back());
      HIPCHK(hipMemcpy(usrc.data(), op->d_usrc, usrc.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (fus::thermal_owner_mask(ni, op->n_uidx, uidx.data(), uptr.data(), usrc.data(), &M[i].own) != fus::TOWN_OK)
        return fail(FUS_ERR_STATE, "fus_thermal_lambda_max: malformed halo lists");
    }
  }
  FUSCHK(thermal_sum(ths, n, [](fus_thermal* t) -> void* { return t->ths; }));
  for (int i = 0; i < n; ++i)
  {
    fus_thermal* th = ths[i];
    hipStream_t st = th->ctx->stream;
    const int64_t ni = th->op->L.n_internal;
    FUSCHK(thermal_impose<T>(th, th->ths, true));
    M[i].x.resize(ni), M[i].y.resize(ni), M[i].mc.resize(ni);
    HIPCHK(hipMemcpyAsync(M[i].x.data(), th->ths, ni * sizeof(T), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(M[i].mc.data(), th->mc, ni * sizeof(T), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  double rho = 0.0;
  for (int it = 0; it < iters; ++it)
  {
    for (int i = 0; i < n; ++i)
    {
      fus_thermal* th = ths[i];
      FUSCHK(d_apply_internal(th->op, OP_STIFFNESS, th->kneg, th->ths, th->b));
      FUSCHK(thermal_robin<T>(th, static_cast<const T*>(th->ths), false));
    }
    FUSCHK(thermal_sum(ths, n, [](fus_thermal* t) -> void* { return t->b; }));
    double dots[3] = {0.0, 0.0, 0.0};   // x . m y, x . m x, y . m y
    for (int i = 0; i < n; ++i)
    {
      fus_thermal* th = ths[i];
      hipStream_t st = th->ctx->stream;
      const int64_t ni = th->op->L.n_internal;
      Member& m = M[i];
      hipLaunchKernelGGL((k_thermal_power<T>), dim3(1024), dim3(256), 0, st, ni, static_cast<const T*>(th->b),
                         static_cast<const T*>(th->ths), static_cast<const T*>(th->mw),
                         (T)th->resp.phi_max, static_cast<const T*>(thermal_minv(th)), static_cast<T*>(th->acc));
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(m.y.data(), th->acc, ni * sizeof(T), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      double xy = 0.0, xx = 0.0, yy = 0.0;
      for (int64_t k = 0; k < ni; ++k)
      {
        if (!m.own.empty() && !m.own[k])
          continue;
        const double w = (double)m.mc[k], xi = (double)m.x[k], yi = (double)m.y[k];
        xy += xi * (w * yi), xx += xi * (w * xi), yy += yi * (w * yi);
      }
      dots[0] += xy, dots[1] += xx, dots[2] += yy;
    }
    if (n == 1 && thermal_multi(ths[0]) && !ths[0]->ctx->local_group)
      FUSCHK(fus_comm_allreduce(ths[0]->ctx, dots, 3, FUS_SUM));
    const double xy = dots[0], xx = dots[1], yy = dots[2];
    if (!(xx > 0.0) || !std::isfinite(xy) || !std::isfinite(yy))
      return fail(FUS_ERR_STATE, "fus_thermal_lambda_max: the iteration broke down (zero or non-finite vector)");
    rho = xy / xx;
    if (!(yy > 0.0))   // k = 0 and W = 0 everywhere: the operator is zero
      break;
    const double nrm = std::sqrt(yy);
    for (int i = 0; i < n; ++i)
    {
      fus_thermal* th = ths[i];
      Member& m = M[i];
      for (size_t k = 0; k < m.x.size(); ++k)
        m.x[k] = (T)((double)m.y[k] / nrm);
      HIPCHK(hipMemcpyAsync(th->ths, m.x.data(), m.x.size() * sizeof(T), hipMemcpyHostToDevice, th->ctx->stream));
      HIPCHK(hipStreamSynchronize(th->ctx->stream));
    }
  }
  for (int i = 0; i < n; ++i)
  {
    fus_thermal* th = ths[i];
    const int64_t ni = th->op->L.n_internal;
    HIPCHK(hipMemsetAsync(th->ths, 0, ni * sizeof(T), th->ctx->stream));
    HIPCHK(hipMemsetAsync(th->acc, 0, ni * sizeof(T), th->ctx->stream));
    HIPCHK(hipStreamSynchronize(th->ctx->stream));
  }
  *lambda = rho;
  return FUS_OK;
}

// Replaces the boundary: the lists are built and validated on the host (thermal_bc.hpp), uploaded into buffers of their own
// and only then put in force, so that an error leaves the previous boundary as it was.
template <typename T>
static int thermal_install_boundary(fus_thermal* th, const uint8_t* fixed, const void* fixed_rise, const void* conv_diag,
                                    const void* conv_rise)
{
  fus_op* op = th->op;
  hipStream_t st = th->ctx->stream;
  const int64_t n = op->L.n_internal;
  fus::ThermalBcLists<T> L;
  const int err = fus::thermal_bc_lists<T>(op->ndofs, op->L.dof_perm.data(), fixed, static_cast<const T*>(fixed_rise),
                                           static_cast<const T*>(conv_diag), static_cast<const T*>(conv_rise), &L);
  if (err != fus::TBC_OK)
    return fail(FUS_ERR_ARG, std::string("fus_thermal_set_boundary: ") + fus::thermal_bc_message(err));
  ThermalBoundary B;
  const char* what = "boundary lists (fus_thermal_set_boundary)";
  B.nfix = (int64_t)L.fix_idx.size(), B.nconv = (int64_t)L.conv_idx.size();
  if (B.nfix > 0)
  {
    FUSCHK(upload(B.fix_idx, L.fix_idx, st, what));
    FUSCHK(upload(B.fix_val, L.fix_val, st, what));
    if (!th->minv_bc)
      FUSCHK(dalloc_bytes(th->allocs, &th->minv_bc, n * sizeof(T), false, st));
  }
  if (B.nconv > 0)
  {
    FUSCHK(upload(B.conv_idx, L.conv_idx, st, what));
    FUSCHK(upload(B.conv_hw, L.hw, st, what));
    FUSCHK(upload(B.conv_r, L.r, st, what));
  }
  HIPCHK(hipStreamSynchronize(st));   // the uploads read L
  th->bc = std::move(B);   // every step that read the previous lists has finished: the step calls synchronise
  if (th->bc.nfix > 0)
  {
    HIPCHK(hipMemcpyAsync(th->minv_bc, th->minv, n * sizeof(T), hipMemcpyDeviceToDevice, st));
    // the rise of an object not yet initialised is rewritten by fus_thermal_init / fus_thermal_set, which impose again
    FUSCHK(thermal_impose<T>(th, th->th0, false, true));
    HIPCHK(hipStreamSynchronize(st));
  }
  return FUS_OK;
}

// Several ranks: a DOF is fixed if any sharer fixes it, at the mean of the values the fixing sharers gave (callers are
// expected to give the same one).  Ordered sums of the 0/1 flags and of flag * value make every sharer see the same
// flags and values; the lists are then built from them, so a sharer drops its convective entry on a DOF another rank
// fixed.  The convective diagonal is NOT summed: like the wave models' boundary weights each rank's part rides in its
// partial b.  Every member starts from the boundary its caller gave last (rq_*), and installs the agreed one.
template <typename T>
static int thermal_agree_boundary(fus_thermal** ths, int n)
{
  for (int i = 0; i < n; ++i)
  {
    fus_thermal* th = ths[i];
    fus_op* op = th->op;
    hipStream_t st = th->ctx->stream;
    const int64_t nd = op->ndofs;
    const T* rise = th->rq_rise.empty() ? nullptr : reinterpret_cast<const T*>(th->rq_rise.data());
    std::vector<T> flag(nd, T(0)), val(nd, T(0));
    for (int64_t d = 0; d < nd; ++d)
      if (!th->rq_fixed.empty() && th->rq_fixed[d])
        flag[d] = T(1), val[d] = rise ? rise[d] : T(0);
    T* tc = static_cast<T*>(op->d_tmp_c);
    // flags and values in internal numbering: the stage input's and the accumulator's places are free between steps
    for (int pass = 0; pass < 2; ++pass)
    {
      HIPCHK(hipMemcpyAsync(tc, (pass ? val : flag).data(), nd * sizeof(T), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL((k_to_internal<T>), dim3(nblk(nd)), dim3(256), 0, st, nd, op->d_dof_perm, static_cast<const T*>(tc),
                         static_cast<T*>(pass ? th->acc : th->ths));
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(st));
    }
  }
  FUSCHK(thermal_sum(ths, n, [](fus_thermal* t) -> void* { return t->ths; }));
  FUSCHK(thermal_sum(ths, n, [](fus_thermal* t) -> void* { return t->acc; }));
  int rc = FUS_OK;
  for (int i = 0; i < n; ++i)
  {
    fus_thermal* th = ths[i];
    fus_op* op = th->op;
    hipStream_t st = th->ctx->stream;
    const int64_t nd = op->ndofs, ni = op->L.n_internal;
    std::vector<T> cnt(nd), sum(nd);
    T* tc = static_cast<T*>(op->d_tmp_c);
    for (int pass = 0; pass < 2; ++pass)
    {
      hipLaunchKernelGGL((k_from_internal<T, 0>), dim3(nblk(nd)), dim3(256), 0, st, nd, op->d_dof_perm,
                         static_cast<const T*>(pass ? th->acc : th->ths), tc);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync((pass ? sum : cnt).data(), tc, nd * sizeof(T), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipMemsetAsync(th->ths, 0, ni * sizeof(T), st));
    HIPCHK(hipMemsetAsync(th->acc, 0, ni * sizeof(T), st));
    std::vector<uint8_t> fixed(nd);
    std::vector<T> rise(nd, T(0));
    for (int64_t d = 0; d < nd; ++d)
      if ((fixed[d] = cnt[d] > T(0.5)))
        rise[d] = (T)((double)sum[d] / (double)cnt[d]);
    const int r = thermal_install_boundary<T>(th, fixed.data(), rise.data(), th->rq_diag.empty() ? nullptr : th->rq_diag.data(),
                                              th->rq_crise.empty() ? nullptr : th->rq_crise.data());
    if (r == FUS_OK)
      th->pending &= ~fus_thermal::PEND_BC;
    else if (rc == FUS_OK)   // every member still takes part in what follows; the first error is reported
      rc = r;
  }
  return rc;
}

template <typename T>
static int thermal_set_boundary(fus_thermal* th, const uint8_t* fixed, const void* fixed_rise, const void* conv_diag,
                                const void* conv_rise)
{
  if (!thermal_multi(th))
    return thermal_install_boundary<T>(th, fixed, fixed_rise, conv_diag, conv_rise);
  // validated before anything is kept: an error leaves the previous boundary, and the previous request, as they were
  fus::ThermalBcLists<T> L;
  const int err = fus::thermal_bc_lists<T>(th->op->ndofs, th->op->L.dof_perm.data(), fixed, static_cast<const T*>(fixed_rise),
                                           static_cast<const T*>(conv_diag), static_cast<const T*>(conv_rise), &L);
  if (err != fus::TBC_OK)
    return fail(FUS_ERR_ARG, std::string("fus_thermal_set_boundary: ") + fus::thermal_bc_message(err));
  const size_t nd = (size_t)th->op->ndofs;
  auto keep = [nd](std::vector<char>& v, const void* a)
  {
    const char* q = static_cast<const char*>(a);
    v.assign(q, q + (a ? nd * sizeof(T) : 0));
  };
  th->rq_fixed.assign(fixed, fixed + (fixed ? nd : 0));
  keep(th->rq_rise, fixed_rise), keep(th->rq_diag, conv_diag), keep(th->rq_crise, conv_rise);
  if (thermal_in_group(th))
  {
    th->pending |= fus_thermal::PEND_BC;
    return FUS_OK;
  }
  return thermal_agree_boundary<T>(&th, 1);
}

// ---- C ABI (fusmi.h "bioheat") ----

// FUS_ERR_STATE while sums over the sharers wait for fus_group_thermal_finish
static int thermal_ready(const fus_thermal* th, const char* fn)
{
  if (th->pending)
    return fail(FUS_ERR_STATE, std::string(fn) + ": sums over the sharers of the interface DOFs are pending; "
                                                 "fus_group_thermal_finish must be called first");
  return FUS_OK;
}

// the single-object calls that exchange: not on a member of an in-process group
static int thermal_single(const fus_thermal* th, const char* fn, const char* group_fn)
{
  FUSCHK(thermal_ready(th, fn));
  if (thermal_in_group(th))
    return fail(FUS_ERR_STATE, std::string(fn) + ": in-process transport: use " + group_fn);
  return FUS_OK;
}

// the members of a group call: objects of one scalar type on one device, in in-process contexts of distinct ranks, every
// neighbour of every member among them
static int thermal_group(fus_thermal** ths, int n, const char* fn)
{
  if (!ths || n < 1)
    return fail(FUS_ERR_ARG, std::string(fn) + ": bad group");
  for (int i = 0; i < n; ++i)
  {
    if (!ths[i])
      return fail(FUS_ERR_ARG, std::string(fn) + ": null member");
    if (ths[i]->op->dtype != ths[0]->op->dtype || ths[i]->ctx->device != ths[0]->ctx->device)
      return fail(FUS_ERR_ARG, std::string(fn) + ": the members differ in scalar type or device");
    if (thermal_multi(ths[i]) && !ths[i]->ctx->local_group)
      return fail(FUS_ERR_ARG, std::string(fn) + ": a member's context is not part of an in-process group (fus_comm_init_local)");
    for (int j = 0; j < i; ++j)
      if (ths[j] == ths[i] || ths[j]->ctx->rank == ths[i]->ctx->rank)
        return fail(FUS_ERR_ARG, std::string(fn) + ": two members of one rank");
  }
  for (int i = 0; i < n; ++i)
    for (const Neigh& nb : ths[i]->op->neigh)
    {
      bool found = false;
      for (int j = 0; j < n; ++j)
        found = found || ths[j]->ctx->rank == nb.rank;
      if (!found)
        return fail(FUS_ERR_ARG, std::string(fn) + ": the group lacks rank " + std::to_string(nb.rank) + ", a neighbour of rank "
                                     + std::to_string(ths[i]->ctx->rank));
    }
  return FUS_OK;
}

// the members of a group call carry the same response and damage laws
static int thermal_same_laws(fus_thermal** ths, int n, const char* fn)
{
  for (int i = 1; i < n; ++i)
    if (!ths[i]->resp.same(ths[0]->resp) || !ths[i]->dmg.same(ths[0]->dmg))
      return fail(FUS_ERR_STATE, std::string(fn) + ": the members differ in their perfusion response or damage parameters; "
                                                   "call fus_thermal_set_response / fus_thermal_set_damage alike on all of them");
  return FUS_OK;
}

static int thermal_step_args(const char* fn, double dt, int64_t nsteps, double heat_scale)
{
  if (!(dt > 0) || !std::isfinite(dt))
    return fail(FUS_ERR_ARG, std::string(fn) + ": dt must be positive and finite");
  if (nsteps < 0 || !std::isfinite(heat_scale))
    return fail(FUS_ERR_ARG, std::string(fn) + ": nsteps must be >= 0 and heat_scale finite");
  return FUS_OK;
}

int fus_thermal_create(fus_ctx* c, fus_op* op, const void* conductivity, const void* rho_c, const void* perfusion,
                       double t_base, fus_thermal** out)
{
  if (!c || !op || !conductivity || !rho_c || !out)
    return fail(FUS_ERR_ARG, "fus_thermal_create: null argument");
  if (op->ctx != c)
    return fail(FUS_ERR_ARG, "fus_thermal_create: the operator data belongs to another context");
  if (!std::isfinite(t_base))
    return fail(FUS_ERR_ARG, "fus_thermal_create: t_base must be finite");
  if ((!op->neigh.empty() || c->nranks > 1) && !(c->comm || (c->local_group && !c->external_transport)))
    return fail(FUS_ERR_STATE, "fus_thermal_create: several ranks need a transport of the library's own: an RCCL communicator "
                               "(fus_comm_init) or an in-process group (fus_comm_init_local); the external-transport entry "
                               "points do not cover the thermal model");
  HIPCHK(hipSetDevice(c->device));
  std::unique_ptr<fus_thermal> th(new fus_thermal());
  th->ctx = c, th->op = op, th->t_base = t_base;
  const int r = FUS_BY_DTYPE(th->op->dtype, thermal_setup, th.get(), conductivity, rho_c, perfusion);
  if (r != FUS_OK)
    return r;   // (th frees what the setup had allocated)
  *out = th.release();
  return FUS_OK;
}

int fus_thermal_destroy(fus_thermal* th)
{
  if (!th)
    return FUS_OK;
  (void)hipSetDevice(th->ctx->device);
  (void)hipStreamSynchronize(th->ctx->stream);
  delete th;   // frees its arrays: nothing on the stream reads them any more
  return FUS_OK;
}

int fus_thermal_init(fus_thermal* th)
{
  if (!th)
    return fail(FUS_ERR_ARG, "fus_thermal_init: null argument");
  FUSCHK(thermal_ready(th, "fus_thermal_init"));
  HIPCHK(hipSetDevice(th->ctx->device));
  const int64_t n = th->op->L.n_internal;
  for (void* v : {th->th0, th->ths, th->acc})
    HIPCHK(hipMemsetAsync(v, 0, n * th->op->ts, th->ctx->stream));
  HIPCHK(hipMemsetAsync(th->dose, 0, n * sizeof(double), th->ctx->stream));
  if (th->dmg.on())
    HIPCHK(hipMemsetAsync(th->omega.p, 0, n * sizeof(double), th->ctx->stream));
  FUSCHK(FUS_BY_DTYPE(th->op->dtype, thermal_impose, th, th->th0));
  HIPCHK(hipStreamSynchronize(th->ctx->stream));
  th->initialised = th->respond_dirty = true;
  return FUS_OK;
}

int fus_thermal_set(fus_thermal* th, int which, const void* in, int space)
{
  if (!th || !in || (which != FUS_TH_RISE && which != FUS_TH_DOSE && which != FUS_TH_DAMAGE)
      || (space != FUS_HOST && space != FUS_DEVICE))
    return fail(FUS_ERR_ARG, "fus_thermal_set: null argument, which not FUS_TH_RISE | FUS_TH_DOSE | FUS_TH_DAMAGE, or bad space");
  if (which == FUS_TH_DAMAGE && !th->dmg.on())
    return fail(FUS_ERR_STATE, "fus_thermal_set: FUS_TH_DAMAGE while the damage is off (fus_thermal_set_damage)");
  FUSCHK(thermal_ready(th, "fus_thermal_set"));
  HIPCHK(hipSetDevice(th->ctx->device));
  FUSCHK(FUS_BY_DTYPE(th->op->dtype, thermal_vec, th, which, const_cast<void*>(in), space, true));
  th->initialised = th->respond_dirty = true;
  return FUS_OK;
}

int fus_thermal_get(fus_thermal* th, int which, void* out, int space)
{
  if (!th || !out || which < FUS_TH_RISE || which > FUS_TH_PERFUSION || (space != FUS_HOST && space != FUS_DEVICE))
    return fail(FUS_ERR_ARG, "fus_thermal_get: null argument, which not FUS_TH_RISE | FUS_TH_DOSE | FUS_TH_HEAT | FUS_TH_DAMAGE | "
                             "FUS_TH_PERFUSION, or bad space");
  if (which == FUS_TH_DAMAGE && !th->dmg.on())
    return fail(FUS_ERR_STATE, "fus_thermal_get: FUS_TH_DAMAGE while the damage is off (fus_thermal_set_damage)");
  HIPCHK(hipSetDevice(th->ctx->device));
  if (which == FUS_TH_PERFUSION)   // the plane the next step will use: formed now if the state changed since the last step
  {
    FUSCHK(thermal_ready(th, "fus_thermal_get"));
    FUSCHK(FUS_BY_DTYPE(th->op->dtype, thermal_prime, th));
  }
  return FUS_BY_DTYPE(th->op->dtype, thermal_vec, th, which, out, space, false);
}

int fus_thermal_set_heat(fus_thermal* th, const void* q, const void* q_coef, int space)
{
  if (!th || (space != FUS_HOST && space != FUS_DEVICE))
    return fail(FUS_ERR_ARG, "fus_thermal_set_heat: null argument or bad space");
  HIPCHK(hipSetDevice(th->ctx->device));
  return FUS_BY_DTYPE(th->op->dtype, thermal_set_heat, th, q, q_coef, space);
}

int fus_thermal_set_heat_from_monitor(fus_thermal* th, fus_model* m, const void* absorption)
{
  if (!th || !m || !absorption)
    return fail(FUS_ERR_ARG, "fus_thermal_set_heat_from_monitor: null argument");
  if (m->op != th->op)
    return fail(FUS_ERR_ARG, "fus_thermal_set_heat_from_monitor: the model runs on another fus_op than the thermal object");
  if (m->mon.every <= 0 || !m->mon.d_mon)
    return fail(FUS_ERR_STATE, "fus_thermal_set_heat_from_monitor: the model's monitor is off (fus_model_monitor)");
  if (m->mon.which != FUS_U)
    return fail(FUS_ERR_STATE, "fus_thermal_set_heat_from_monitor: the monitor watches FUS_V; the heat needs the pressure, FUS_U");
  if (m->mon.n == 0)
    return fail(FUS_ERR_STATE, "fus_thermal_set_heat_from_monitor: the monitor has taken no sample yet");
  HIPCHK(hipSetDevice(th->ctx->device));
  return FUS_BY_DTYPE(th->op->dtype, thermal_heat_from_monitor, th, m, absorption);
}

int fus_thermal_set_heat_from_harmonics(fus_thermal* th, fus_model* m, int nharm, const void* absorption)
{
  if (!th || !m || !absorption)
    return fail(FUS_ERR_ARG, "fus_thermal_set_heat_from_harmonics: null argument");
  if (m->op != th->op)
    return fail(FUS_ERR_ARG, "fus_thermal_set_heat_from_harmonics: the model runs on another fus_op than the thermal object");
  if (nharm < 1 || nharm > 8)
    return fail(FUS_ERR_ARG, "fus_thermal_set_heat_from_harmonics: nharm must lie in 1..8");
  if (m->mon.every <= 0 || !m->mon.d_mon)
    return fail(FUS_ERR_STATE, "fus_thermal_set_heat_from_harmonics: the model's monitor is off (fus_model_monitor)");
  if (m->mon.which != FUS_U)
    return fail(FUS_ERR_STATE, "fus_thermal_set_heat_from_harmonics: the monitor watches FUS_V; the heat needs the pressure, FUS_U");
  if (m->mon.n == 0)
    return fail(FUS_ERR_STATE, "fus_thermal_set_heat_from_harmonics: the monitor has taken no sample yet");
  if (nharm > m->mon.nharm)
    return fail(FUS_ERR_STATE, "fus_thermal_set_heat_from_harmonics: the monitor holds fewer harmonics than nharm asks for");
  HIPCHK(hipSetDevice(th->ctx->device));
  return FUS_BY_DTYPE(th->op->dtype, thermal_heat_from_harmonics, th, m, nharm, absorption);
}

int fus_thermal_lambda_max(fus_thermal* th, int iters, double* lambda)
{
  if (!th || !lambda)
    return fail(FUS_ERR_ARG, "fus_thermal_lambda_max: null argument");
  if (iters < 1)
    return fail(FUS_ERR_ARG, "fus_thermal_lambda_max: iters must be at least 1");
  FUSCHK(thermal_single(th, "fus_thermal_lambda_max", "fus_group_thermal_lambda_max"));
  HIPCHK(hipSetDevice(th->ctx->device));
  return FUS_BY_DTYPE(th->op->dtype, thermal_lambda_max, &th, 1, iters, lambda);
}

int fus_thermal_steps(fus_thermal* th, double dt, int64_t nsteps, double heat_scale)
{
  if (!th)
    return fail(FUS_ERR_ARG, "fus_thermal_steps: null argument");
  FUSCHK(thermal_step_args("fus_thermal_steps", dt, nsteps, heat_scale));
  FUSCHK(thermal_single(th, "fus_thermal_steps", "fus_group_thermal_steps"));
  if (!th->initialised)
    return fail(FUS_ERR_STATE, "fus_thermal_init (or fus_thermal_set) must be called before fus_thermal_steps");
  HIPCHK(hipSetDevice(th->ctx->device));
  return FUS_BY_DTYPE(th->op->dtype, thermal_run, &th, 1, dt, nsteps, heat_scale, 0);
}

int fus_thermal_steps_sts(fus_thermal* th, double dt, int64_t nsteps, double heat_scale, int stages)
{
  if (!th)
    return fail(FUS_ERR_ARG, "fus_thermal_steps_sts: null argument");
  if (!fus::sts_stages_ok(stages))
    return fail(FUS_ERR_ARG, "fus_thermal_steps_sts: stages must lie in 2..32");
  FUSCHK(thermal_step_args("fus_thermal_steps_sts", dt, nsteps, heat_scale));
  FUSCHK(thermal_single(th, "fus_thermal_steps_sts", "fus_group_thermal_steps"));
  if (!th->initialised)
    return fail(FUS_ERR_STATE, "fus_thermal_init (or fus_thermal_set) must be called before fus_thermal_steps_sts");
  HIPCHK(hipSetDevice(th->ctx->device));
  if (!th->f0)   // objects that never use the scheme keep their footprint
    FUSCHK(dalloc_bytes(th->allocs, &th->f0, th->op->L.n_internal * th->op->ts, true, th->ctx->stream));
  return FUS_BY_DTYPE(th->op->dtype, thermal_run, &th, 1, dt, nsteps, heat_scale, stages);
}

// ---- bioheat on the members of an in-process group (fusmi.h "bioheat", several ranks) ----
int fus_group_thermal_finish(fus_thermal** ths, int n)
{
  FUSCHK(thermal_group(ths, n, "fus_group_thermal_finish"));
  int any = 0, all = ~0;
  for (int i = 0; i < n; ++i)
    any |= ths[i]->pending, all &= ths[i]->pending;
  if ((any & ~all) & fus_thermal::PEND_SETUP)
    return fail(FUS_ERR_STATE, "fus_group_thermal_finish: some members have been finished before and some have not; create the "
                               "thermal objects of all ranks, then finish them together");
  if ((any & ~all) & fus_thermal::PEND_HEAT)
    return fail(FUS_ERR_STATE, "fus_group_thermal_finish: a heat load waits on some members only; fus_thermal_set_heat / "
                               "fus_thermal_set_heat_from_monitor must be called on every member");
  if (all & fus_thermal::PEND_HEAT)
    for (int i = 1; i < n; ++i)
      if (ths[i]->pend_load != ths[0]->pend_load)
        return fail(FUS_ERR_STATE, "fus_group_thermal_finish: the heat loads that wait on the members are of different kinds; "
                                   "call fus_thermal_set_heat_from_harmonics on every member or on none");
  HIPCHK(hipSetDevice(ths[0]->ctx->device));
  if (any & fus_thermal::PEND_SETUP)
  {
    FUSCHK(thermal_sum(ths, n, [](fus_thermal* t) -> void* { return t->mc; }));
    FUSCHK(thermal_sum(ths, n, [](fus_thermal* t) -> void* { return t->mw; }));
    for (int i = 0; i < n; ++i)
    {
      FUSCHK(FUS_BY_DTYPE(ths[i]->op->dtype, thermal_setup_finish, ths[i]));
      ths[i]->pending &= ~fus_thermal::PEND_SETUP;
    }
  }
  if (any & fus_thermal::PEND_BC)   // one member's new boundary may fix DOFs of the others: all agree again
    FUSCHK(FUS_BY_DTYPE(ths[0]->op->dtype, thermal_agree_boundary, ths, n));
  if (any & fus_thermal::PEND_HEAT)
  {
    FUSCHK(thermal_sum(ths, n, [](fus_thermal* t) -> void* { return t->mq; }));
    for (int i = 0; i < n; ++i)
    {
      FUSCHK(FUS_BY_DTYPE(ths[i]->op->dtype, thermal_heat_finish, ths[i]));
      ths[i]->pending &= ~fus_thermal::PEND_HEAT;
    }
  }
  for (int i = 0; i < n; ++i)
  {
    HIPCHK(hipStreamSynchronize(ths[i]->ctx->stream));
    ths[i]->respond_dirty = ths[i]->respond_dirty || any != 0;   // m_W or the fixed values may be new
  }
  return FUS_OK;
}

int fus_group_thermal_steps(fus_thermal** ths, int n, double dt, int64_t nsteps, double heat_scale, int stages)
{
  FUSCHK(thermal_group(ths, n, "fus_group_thermal_steps"));
  if (stages != 0 && !fus::sts_stages_ok(stages))
    return fail(FUS_ERR_ARG, "fus_group_thermal_steps: stages must be 0 (RK4) or lie in 2..32");
  FUSCHK(thermal_step_args("fus_group_thermal_steps", dt, nsteps, heat_scale));
  FUSCHK(thermal_same_laws(ths, n, "fus_group_thermal_steps"));
  for (int i = 0; i < n; ++i)
  {
    FUSCHK(thermal_ready(ths[i], "fus_group_thermal_steps"));
    if (!ths[i]->initialised)
      return fail(FUS_ERR_STATE, "fus_thermal_init (or fus_thermal_set) must be called on every member before fus_group_thermal_steps");
  }
  HIPCHK(hipSetDevice(ths[0]->ctx->device));
  for (int i = 0; i < n; ++i)
    if (stages != 0 && !ths[i]->f0)
      FUSCHK(dalloc_bytes(ths[i]->allocs, &ths[i]->f0, ths[i]->op->L.n_internal * ths[i]->op->ts, true, ths[i]->ctx->stream));
  return FUS_BY_DTYPE(ths[0]->op->dtype, thermal_run, ths, n, dt, nsteps, heat_scale, stages);
}

static int thermal_group_lambda(fus_thermal** ths, int n, int iters, const char* fn, double* lambda)
{
  FUSCHK(thermal_group(ths, n, fn));
  if (!lambda)
    return fail(FUS_ERR_ARG, std::string(fn) + ": null argument");
  if (iters < 1)
    return fail(FUS_ERR_ARG, std::string(fn) + ": iters must be at least 1");
  FUSCHK(thermal_same_laws(ths, n, fn));
  for (int i = 0; i < n; ++i)
    FUSCHK(thermal_ready(ths[i], fn));
  HIPCHK(hipSetDevice(ths[0]->ctx->device));
  return FUS_BY_DTYPE(ths[0]->op->dtype, thermal_lambda_max, ths, n, iters, lambda);
}

int fus_group_thermal_lambda_max(fus_thermal** ths, int n, int iters, double* lambda)
{
  return thermal_group_lambda(ths, n, iters, "fus_group_thermal_lambda_max", lambda);
}

// lambda_max turned into a step: 2 / rho for RK4 (stages = 0), 0.72 beta_s / rho for RKL2
static int thermal_dt_from(const char* fn, double rho, int stages, double* dt)
{
  if (!(rho > 0.0))
    return fail(FUS_ERR_STATE, std::string(fn) + ": the operator is zero (k = 0 and W = 0 everywhere): any step is stable");
  *dt = stages == 0 ? 2.0 / rho : 0.72 * fus::sts_beta(stages) / rho;
  return FUS_OK;
}

int fus_group_thermal_stable_dt(fus_thermal** ths, int n, int iters, int stages, double* dt)
{
  if (stages != 0 && !fus::sts_stages_ok(stages))
    return fail(FUS_ERR_ARG, "fus_group_thermal_stable_dt: stages must be 0 (RK4) or lie in 2..32");
  double rho = 0.0;
  FUSCHK(thermal_group_lambda(ths, n, iters, "fus_group_thermal_stable_dt", dt ? &rho : nullptr));
  return thermal_dt_from("fus_group_thermal_stable_dt", rho, stages, dt);
}

int fus_thermal_set_boundary(fus_thermal* th, const uint8_t* fixed, const void* fixed_rise, const void* conv_diag,
                             const void* conv_rise)
{
  if (!th)
    return fail(FUS_ERR_ARG, "fus_thermal_set_boundary: null argument");
  HIPCHK(hipSetDevice(th->ctx->device));
  th->respond_dirty = true;   // theta at the fixed DOFs may be new
  return FUS_BY_DTYPE(th->op->dtype, thermal_set_boundary, th, fixed, fixed_rise, conv_diag, conv_rise);
}

int fus_thermal_set_response(fus_thermal* th, int nknots, const double* temp, const double* factor, double dose_lo,
                             double dose_hi)
{
  if (!th)
    return fail(FUS_ERR_ARG, "fus_thermal_set_response: null argument");
  fus::ThermalResponse R;
  const int err = fus::thermal_response_check(nknots, temp, factor, dose_lo, dose_hi, &R);
  if (err != fus::TRS_OK)
    return fail(FUS_ERR_ARG, std::string("fus_thermal_set_response: ") + fus::thermal_response_message(err));
  HIPCHK(hipSetDevice(th->ctx->device));
  if (R.active() && !th->mweff)
  {
    FUSCHK(dalloc_bytes(th->allocs, &th->mweff, th->op->L.n_internal * th->op->ts, true, th->ctx->stream));
    HIPCHK(hipStreamSynchronize(th->ctx->stream));
  }
  th->resp = R;   // every step that read the previous law has finished: the step calls synchronise
  th->respond_dirty = true;
  return FUS_OK;
}

int fus_thermal_set_damage(fus_thermal* th, double A, double Ea)
{
  if (!th)
    return fail(FUS_ERR_ARG, "fus_thermal_set_damage: null argument");
  fus::ThermalDamage D;
  const int err = fus::thermal_damage_check(A, Ea, &D);
  if (err != fus::TRS_OK)
    return fail(FUS_ERR_ARG, std::string("fus_thermal_set_damage: ") + fus::thermal_response_message(err));
  HIPCHK(hipSetDevice(th->ctx->device));
  if (!D.on())
    th->omega.reset(), th->rprev.reset();
  else if (!th->dmg.on())   // switched on: Omega = 0; a change of the constants keeps what has accumulated
  {
    const size_t bytes = (size_t)th->op->L.n_internal * sizeof(double);
    DevBuf om, rp;
    FUSCHK(om.alloc(bytes, "the damage plane (fus_thermal_set_damage)"));
    FUSCHK(rp.alloc(bytes, "the damage rate plane (fus_thermal_set_damage)"));
    HIPCHK(hipMemsetAsync(om.p, 0, bytes, th->ctx->stream));
    HIPCHK(hipMemsetAsync(rp.p, 0, bytes, th->ctx->stream));
    HIPCHK(hipStreamSynchronize(th->ctx->stream));
    th->omega = std::move(om), th->rprev = std::move(rp);
  }
  th->dmg = D;
  th->respond_dirty = true;
  return FUS_OK;
}

int fus_thermal_boundary_info(fus_thermal* th, int64_t* nfixed, int64_t* nconvective)
{
  if (!th)
    return fail(FUS_ERR_ARG, "fus_thermal_boundary_info: null argument");
  if (nfixed)
    *nfixed = th->bc.nfix;
  if (nconvective)
    *nconvective = th->bc.nconv;
  return FUS_OK;
}

int fus_thermal_stable_dt(fus_thermal* th, int iters, int stages, double* dt)
{
  if (!th || !dt)
    return fail(FUS_ERR_ARG, "fus_thermal_stable_dt: null argument");
  if (iters < 1)
    return fail(FUS_ERR_ARG, "fus_thermal_stable_dt: iters must be at least 1");
  if (stages != 0 && !fus::sts_stages_ok(stages))
    return fail(FUS_ERR_ARG, "fus_thermal_stable_dt: stages must be 0 (RK4) or lie in 2..32");
  FUSCHK(thermal_single(th, "fus_thermal_stable_dt", "fus_group_thermal_stable_dt"));
  HIPCHK(hipSetDevice(th->ctx->device));
  double rho = 0.0;
  FUSCHK(FUS_BY_DTYPE(th->op->dtype, thermal_lambda_max, &th, 1, iters, &rho));
  return thermal_dt_from("fus_thermal_stable_dt", rho, stages, dt);
}

