// fusmi.hpp -- C++ host side above the C ABI (fusmi.h): the reference's operator and model classes
// with the same names, template parameters and call semantics, minus the DOLFINx types.
//
//   reference (cpp/fenicsx-sf/common)                     here (namespace fusmi)
//   StiffnessSpectral3D<T,P>(V); op(x, coeffs, y)         StiffnessSpectral3D<T,P>(data); op(x, coeffs, y)
//     spectral_op.hpp:132-243  (y += K(coeffs) x)
//   MassSpectral3D<T,P>(V); op(x, coeffs, y)              MassSpectral3D<T,P>(data); op(x, coeffs, y)
//     spectral_op.hpp:29-86
//   StiffnessSpectral2D / MassSpectral2D                  same classes, SpaceView::tdim = 2
//     cpp/fenicsx-sf-naive/common/spectral_op.hpp:29-359
//   LinearSpectral3D<T,P>(element, mesh, facet_tags,      LinearSpectral3D<T,P>(data, facets, c0, rho0,
//       c0, rho0, freq, amp, speed)                            freq, amp, speed)
//     init(); rk4(t0, tf, dt); u_sol(); number_of_dofs()    init(); rk4(t0, tf, dt); u_sol(); number_of_dofs()
//     Linear.hpp:52-347
//   LossySpectral3D (Lossy.hpp:56-342), WesterveltSpectral3D (Westervelt.hpp:58-373): + delta0 (, beta0)
//   (none: the reference has no thermal model)          BioheatSpectral3D<T,P>(data, conductivity, rho_c, perfusion)
//
// Where the reference takes a dolfinx::fem::FunctionSpace / Mesh / MeshTags and derives arrays from
// them (spectral_op.hpp:135-171, Linear.hpp:113-118), these classes take those arrays directly
// (SpaceView, FacetView): INTEGRATION.md shows how a DOLFINx build fills them.  Vectors are plain
// pointers to caller-owned host memory (la::Vector::array() in the reference).  Errors become
// fusmi::Error (the C ABI's code and message); nothing else is added on top of the C ABI.
// Header-only, C++17, no dependency beyond fusmi.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "fusmi.h"

namespace fusmi
{

struct Error : std::runtime_error
{
  int code;
  Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

inline void check(int rc)
{
  if (rc != FUS_OK)
    throw Error(rc, fus_last_error());
}

template <typename T>
constexpr int dtype_code()
{
  static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "T is float or double");
  return std::is_same<T, double>::value ? FUS_F64 : FUS_F32;
}

// One GPU = one context (the reference: one MPI rank).
class Context
{
public:
  explicit Context(int device = 0) { check(fus_init(device, &h_)); }
  ~Context() { fus_finalize(h_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  void set_option(const char* key, std::int64_t value) { check(fus_set_option(h_, key, value)); }
  void synchronize() { check(fus_synchronize(h_)); }
  // multi-GPU: id from comm_unique_id() on rank 0, broadcast by the caller (MPI_Bcast in the reference's setting)
  static std::vector<char> comm_unique_id()
  {
    std::vector<char> id(128);
    check(fus_comm_unique_id(id.data()));
    return id;
  }
  void comm_init(int rank, int nranks, const std::vector<char>& id) { check(fus_comm_init(h_, rank, nranks, id.data())); }
  // MPI_Reduce + MPI_Bcast of the examples' mains (linear_planewave2d_1/main.cpp:67-68): op = FUS_SUM | FUS_MIN | FUS_MAX
  double allreduce(double v, int op)
  {
    check(fus_comm_allreduce(h_, &v, 1, op));
    return v;
  }
  fus_ctx* handle() const { return h_; }

private:
  fus_ctx* h_ = nullptr;
};

// The Rayleigh integral of a radiating surface outside the mesh (fusmi.h "transducers"): src_xyz [nsrc][3], src_q [nsrc][2]
// (re, im of the volume velocity), tgt_xyz [ntgt][3] on the host; returns double[planes][ntgt], plane-major: P_re, P_im; with
// FUS_RAY_GRAD the six gradient planes; with FUS_RAY_RMIN the distance to the nearest source point.
struct RayleighPlan
{
  std::int64_t chunks, targets_per_workgroup, launches, workspace_bytes;
};
inline RayleighPlan rayleigh_plan(const Context& ctx, std::int64_t nsrc, std::int64_t ntgt, int what = FUS_RAY_P)
{
  std::int64_t o[4];
  check(fus_rayleigh_plan(ctx.handle(), nsrc, ntgt, what, o));
  return {o[0], o[1], o[2], o[3]};
}
inline std::vector<double> rayleigh(const Context& ctx, const std::vector<double>& src_xyz, const std::vector<double>& src_q,
                                    const std::vector<double>& tgt_xyz, double freq, double c, double rho, double alpha = 0.0,
                                    int what = FUS_RAY_P, int precision = FUS_RAY_F64)
{
  const std::int64_t nsrc = (std::int64_t)(src_xyz.size() / 3), ntgt = (std::int64_t)(tgt_xyz.size() / 3);
  if (src_xyz.size() != (std::size_t)nsrc * 3 || src_q.size() != (std::size_t)nsrc * 2 || tgt_xyz.size() != (std::size_t)ntgt * 3)
    throw Error(FUS_ERR_ARG, "rayleigh: src_xyz [nsrc][3], src_q [nsrc][2] and tgt_xyz [ntgt][3] are expected");
  const int planes = 2 + ((what & FUS_RAY_GRAD) ? 6 : 0) + ((what & FUS_RAY_RMIN) ? 1 : 0);
  std::vector<double> out((std::size_t)planes * (std::size_t)ntgt);
  check(fus_rayleigh(ctx.handle(), nsrc, src_xyz.data(), src_q.data(), ntgt, tgt_xyz.data(), freq, c, rho, alpha, what,
                     precision, out.data(), FUS_HOST));
  return out;
}

// What the reference's operator constructor derives from the function space (spectral_op.hpp:135-171):
// tensor-ordered cell dofmap (reorder_dofmap, permute.hpp:15-42), 1-D GLL node coordinates in the
// element's local order, mesh geometry.
template <typename T>
struct SpaceView
{
  int tdim = 3;                        // 3: hexahedra, 2: quadrilaterals
  std::int64_t ncells = 0, ndofs = 0, nnodes = 0;
  const std::int32_t* tensor_dofmap = nullptr;  // [ncells * (P+1)^tdim]
  const double* nodes1d = nullptr;              // [P+1]
  const T* geom_x = nullptr;                    // [nnodes * 3]
  const std::int32_t* geom_dofmap = nullptr;    // [ncells * 2^tdim] (order 1) or [ncells * 27] (order 2, tensor order)
  int geom_order = 1;
  // shared dofs per neighbour rank (IndexMap data behind scatter_fwd/rev, Linear.hpp:196-206); empty on one rank
  std::vector<std::int32_t> neighbour_ranks;
  std::vector<std::int64_t> neighbour_counts;
  std::vector<std::int32_t> neighbour_dofs;
};

// Boundary facets as (cell, local facet) pairs with their tag: what fem::compute_integration_domains
// returns per tag (Linear.hpp:113-118); tag 1 = source, tag 2 = absorbing (forms.py:36-39).
struct FacetView
{
  std::int64_t nfacets = 0;
  const std::int32_t* cells = nullptr;
  const std::int32_t* local_facets = nullptr;
  const std::int32_t* tags = nullptr;
};

// Device-resident operator data shared by the mass and stiffness operators and the models (the
// reference builds one copy per operator object, Lossy.hpp:152-153).
template <typename T, int P>
class SpectralOperatorData
{
public:
  // fields = 2 for the lossy / Westervelt models (two operator inputs per block pass)
  SpectralOperatorData(std::shared_ptr<Context> ctx, const SpaceView<T>& V, int fields = 1) : ctx_(std::move(ctx))
  {
    ctx_->set_option("fields", fields);
    int rc = fus_op_create(ctx_->handle(), V.tdim, P, dtype_code<T>(), V.ncells, V.ndofs, V.tensor_dofmap,
                           V.nodes1d, V.geom_x, V.nnodes, V.geom_dofmap, V.geom_order, &h_);
    fus_set_option(ctx_->handle(), "fields", 1);
    check(rc);
    ncells_ = V.ncells, ndofs_ = V.ndofs, tdim_ = V.tdim;
    if (!V.neighbour_ranks.empty())
      check(fus_op_set_neighbours(h_, (int)V.neighbour_ranks.size(), V.neighbour_ranks.data(),
                                  V.neighbour_counts.data(), V.neighbour_dofs.data()));
  }
  ~SpectralOperatorData() { fus_op_destroy(h_); }
  SpectralOperatorData(const SpectralOperatorData&) = delete;
  SpectralOperatorData& operator=(const SpectralOperatorData&) = delete;
  fus_op* handle() const { return h_; }
  const std::shared_ptr<Context>& context() const { return ctx_; }
  std::int64_t ncells() const { return ncells_; }
  std::int64_t ndofs() const { return ndofs_; }
  int tdim() const { return tdim_; }
  bool is_affine() const { return fus_op_is_affine(h_) != 0; }
  int geometry_mode() const { return fus_op_geometry_mode(h_); }  // 0 streamed, 1 affine, 2 trilinear
  // smallest local cell size, mesh::h of linear_planewave2d_1/main.cpp:60-64 (global: Context::allreduce(h, FUS_MIN))
  double hmin() const
  {
    double h = 0;
    check(fus_op_hmin(h_, &h));
    return h;
  }
  // local part of the squared L2 norm (assemble_scalar(u*u*dx), main.cpp:151-157); sum over ranks
  double norm2(const T* x, int loc = FUS_HOST) const
  {
    double v = 0;
    check(fus_op_norm2(h_, x, loc, &v));
    return v;
  }
  // gradient of the nodal field x, T[tdim][ndofs] component-major (fusmi.h "gradient"): nodal = the recovered nodal gradient;
  // else the weighted sums, no sum over the ranks.  coeffs: T[ncells] or nullptr (= 1)
  std::vector<T> gradient(const T* x, const T* coeffs = nullptr, bool nodal = true) const
  {
    std::vector<T> out((size_t)tdim_ * ndofs_, T(0));
    check(fus_op_gradient(h_, x, coeffs, out.data(), nodal ? FUS_GRAD_NODAL : FUS_GRAD_WEIGHTED, FUS_HOST));
    return out;
  }
  // sum_k coeffs[k] (a[k] grad b[k] - b[k] grad a[k]): a, b T[npairs][ndofs], coeffs T[npairs][ncells], npairs in 1..8
  std::vector<T> gradient_pairs(int npairs, const T* a, const T* b, const T* coeffs, bool nodal = true) const
  {
    std::vector<T> out((size_t)tdim_ * ndofs_, T(0));
    check(fus_op_gradient_pairs(h_, npairs, a, b, coeffs, out.data(), nodal ? FUS_GRAD_NODAL : FUS_GRAD_WEIGHTED, FUS_HOST));
    return out;
  }

private:
  std::shared_ptr<Context> ctx_;
  fus_op* h_ = nullptr;
  std::int64_t ncells_ = 0, ndofs_ = 0;
  int tdim_ = 3;
};

// y += K(coeffs) x ; x [ndofs], coeffs [ncells] (one scalar per cell), y [ndofs] accumulated
// (spectral_op.hpp:173-243; the caller zeroes y, Linear.hpp:203).
template <typename T, int P>
class StiffnessSpectral3D
{
public:
  explicit StiffnessSpectral3D(std::shared_ptr<SpectralOperatorData<T, P>> data) : d_(std::move(data)) {}
  void operator()(const T* x, const T* coeffs, T* y) const
  {
    check(fus_stiffness_apply(d_->handle(), x, coeffs, y, FUS_HOST));
  }

private:
  std::shared_ptr<SpectralOperatorData<T, P>> d_;
};

// y += M(coeffs) x (spectral_op.hpp:69-86)
template <typename T, int P>
class MassSpectral3D
{
public:
  explicit MassSpectral3D(std::shared_ptr<SpectralOperatorData<T, P>> data) : d_(std::move(data)) {}
  void operator()(const T* x, const T* coeffs, T* y) const
  {
    check(fus_mass_apply(d_->handle(), x, coeffs, y, FUS_HOST));
  }

private:
  std::shared_ptr<SpectralOperatorData<T, P>> d_;
};

template <typename T, int P>
using StiffnessSpectral2D = StiffnessSpectral3D<T, P>;  // SpaceView::tdim = 2
template <typename T, int P>
using MassSpectral2D = MassSpectral3D<T, P>;

namespace detail
{
template <typename T, int P, int KIND>
class SpectralModel
{
public:
  void init() { check(fus_model_init(h_)); }  // Linear.hpp:161-164: u = v = 0
  // classical RK4 from t0 until t >= tf (Linear.hpp:228-314); returns the number of steps taken
  std::int64_t rk4(const T& t0, const T& tf, const T& dt)
  {
    std::int64_t nsteps = 0;
    check(fus_model_rk4(h_, (double)t0, (double)tf, (double)dt, &nsteps));
    return nsteps;
  }
  // exactly nsteps steps (no last shortened step)
  void rk4_steps(const T& t0, const T& dt, std::int64_t nsteps) { check(fus_model_rk4_steps(h_, (double)t0, (double)dt, nsteps)); }
  // explicit RK order 1..4 of the Python reference (python/src/fenicsxfus/_linear.py:286-311)
  void set_rk_order(int order) { check(fus_model_set_rk_order(h_, order)); }
  std::vector<T> u_sol() const { return get(FUS_U); }  // Linear.hpp:316
  std::vector<T> v_sol() const { return get(FUS_V); }
  void set_state(const T* u, const T* v)
  {
    if (u)
      check(fus_model_set(h_, FUS_U, u, FUS_HOST));
    if (v)
      check(fus_model_set(h_, FUS_V, v, FUS_HOST));
  }
  std::vector<T> mass_vector() const
  {
    std::vector<T> m((size_t)d_->ndofs());
    check(fus_model_get_mass(h_, m.data()));
    return m;
  }
  std::int64_t number_of_dofs() const { return fus_model_ndofs(h_); }  // Linear.hpp:318
  // receivers: u->eval(points_on_proc, shape, cells, u_eval, ...) of cpp/mwe/parallel_eval_line/main.cpp:49-84 on the
  // resident solution -- cells / reference coordinates located by the caller (points outside the rank dropped)
  void set_receivers(const std::vector<std::int32_t>& cells, const std::vector<double>& refcoords)
  {
    nrecv_ = (std::int64_t)cells.size();
    check(fus_model_set_receivers(h_, nrecv_, cells.data(), refcoords.data()));
  }
  std::vector<T> eval(int which = FUS_U) const
  {
    std::vector<T> out((size_t)nrecv_);
    check(fus_model_sample(h_, which, out.data(), FUS_HOST));
    return out;
  }
  // sample after every `every`-th step of rk4 / rk4_steps -- or of fus_group_rk4_steps, or at the last fus_model_stage_end of
  // a step under the external transport -- into a device buffer of `capacity` records
  void record(int every, std::int64_t capacity, int which = FUS_U) { check(fus_model_record(h_, which, every, capacity)); }
  std::vector<T> records(std::vector<double>* times = nullptr) const
  {
    std::int64_t n = 0;
    check(fus_model_get_records(h_, nullptr, nullptr, &n));
    std::vector<T> out((size_t)(n * nrecv_));
    std::vector<double> t((size_t)n);
    check(fus_model_get_records(h_, out.data(), t.data(), &n));
    if (times)
      *times = t;
    return out;
  }
  // field monitor (fusmi.h): after every `every`-th step past the first `skip` steps fold u (or v) into per-DOF
  // running max / min, sum, sum of squares and the cosine / sine sums of the harmonics 1..nharm of freq
  // (0: the source frequency); every = 0 switches it off
  void monitor(int which = FUS_U, int nharm = 0, double freq = 0.0, std::int64_t skip = 0, int every = 1,
               std::int64_t count = 0)
  {
    check(fus_model_monitor(h_, which, nharm, freq, skip, every, count));
  }
  // quantity = FUS_MON_MAX | MIN | MEAN | RMS | COS | SIN (k = 1..nharm for the last two), caller numbering
  std::vector<T> monitor_get(int quantity, int k = 0) const
  {
    std::vector<T> out((size_t)d_->ndofs());
    check(fus_model_monitor_get(h_, quantity, k, out.data(), FUS_HOST));
    return out;
  }
  struct MonitorInfo
  {
    std::int64_t nsamples;
    double t_first, t_last;
  };
  MonitorInfo monitor_info() const
  {
    MonitorInfo i{0, 0.0, 0.0};
    check(fus_model_monitor_info(h_, &i.nsamples, &i.t_first, &i.t_last));
    return i;
  }
  // time-averaged intensity vector from the monitor's harmonic maps, on the device (fusmi.h "intensity"): T[tdim][ndofs],
  // component-major.  coef empty: 1 / (2 rho w_k), W/m^2; else T[nharm][ncells], e.g. alpha_k / (rho c w_k) for the
  // radiation force density in N/m^3
  std::vector<T> intensity(int nharm, const std::vector<T>& coef = {}) const
  {
    if (!coef.empty() && coef.size() != (std::size_t)nharm * (std::size_t)d_->ncells())
      throw Error(FUS_ERR_ARG, "intensity: coef must hold nharm rows of one value per cell");
    std::vector<T> out((size_t)d_->tdim() * d_->ndofs());
    check(fus_model_intensity(h_, nharm, coef.empty() ? nullptr : coef.data(), out.data(), FUS_HOST));
    return out;
  }
  // phased / apodised source (fusmi.h): amplitude factor and delay per DOF (T[ndofs], caller numbering; nullptr = 1 / 0)
  // and the burst duration (0: continuous); all defaults restore the uniform source
  void set_source(const T* amp, const T* delay, double duration = 0.0)
  {
    check(fus_model_set_source(h_, amp, delay, duration, FUS_HOST));
  }
  // source weight at any DOF (fusmi.h): w (T[ndofs], caller numbering) adds w_d g_d(t) to DOF d's right-hand side;
  // replaces earlier weights and restores the default source function, nullptr removes them
  void set_source_weights(const T* w) { check(fus_model_set_source_weights(h_, w, FUS_HOST)); }
  // sampled drive signals (fusmi.h): signals [nchan][nsamp] at the times t_first + j ds, cubic interpolation; channel
  // (int32[ndofs], -1 = silent; nullptr with nchan == 1: channel 0 everywhere); amplitude and delay as in set_source
  void set_source_signals(std::int64_t nchan, std::int64_t nsamp, double t_first, double ds, const double* signals,
                          const std::int32_t* channel = nullptr, const T* amp = nullptr, const T* delay = nullptr)
  {
    check(fus_model_set_source_signals(h_, nchan, nsamp, t_first, ds, signals, channel, amp, delay, FUS_HOST));
  }
  // relaxation absorption (fusmi.h): freqs.size() <= 4 processes with the relaxation frequencies freqs (Hz) and the
  // strengths strength[nu * ncells + cell] (1/s), or one strength per process for a homogeneous medium; the speed of
  // sound given to the constructor is then the high-frequency one.  The memory variables start from 0.
  void set_relaxation(const std::vector<double>& freqs, const std::vector<T>& strength)
  {
    const std::size_t R = freqs.size(), nc = (std::size_t)d_->ncells();
    std::vector<double> omega(R);
    for (std::size_t k = 0; k < R; ++k)
      omega[k] = 2.0 * 3.14159265358979323846 * freqs[k];
    std::vector<T> a(R * nc);
    if (strength.size() == R)
      for (std::size_t k = 0; k < R; ++k)
        std::fill(a.begin() + k * nc, a.begin() + (k + 1) * nc, strength[k]);
    else if (strength.size() == R * nc)
      a = strength;
    else
      throw Error(FUS_ERR_ARG, "set_relaxation: one strength per process, or one per process and cell");
    check(fus_model_set_relaxation(h_, (int)R, omega.data(), a.data()));
  }
  void clear_relaxation() { check(fus_model_set_relaxation(h_, 0, nullptr, nullptr)); }
  std::vector<T> relaxation_state(int nu) const   // z_nu, caller numbering
  {
    std::vector<T> z((size_t)d_->ndofs());
    check(fus_model_relaxation_get(h_, nu, z.data(), FUS_HOST));
    return z;
  }
  // absorbing layers (fusmi.h): the damping rate sigma (1/s) per DOF in caller numbering, zero outside the layers; the
  // sharers of a DOF on several ranks pass the same value.  u, v and the memory variables are kept.
  void set_sponge(const std::vector<T>& sigma)
  {
    if (sigma.size() != (std::size_t)d_->ndofs())
      throw Error(FUS_ERR_ARG, "set_sponge: one damping rate per DOF");
    check(fus_model_set_sponge(h_, sigma.data(), FUS_HOST));
  }
  void clear_sponge() { check(fus_model_set_sponge(h_, nullptr, FUS_HOST)); }
  void sponge_apply(double h) { check(fus_model_sponge_apply(h_, h)); }   // one sub-step on the current state
  fus_model* handle() const { return h_; }
  ~SpectralModel() { fus_model_destroy(h_); }
  SpectralModel(const SpectralModel&) = delete;
  SpectralModel& operator=(const SpectralModel&) = delete;

protected:
  SpectralModel(std::shared_ptr<SpectralOperatorData<T, P>> data, const FacetView& f, const T* c0, const T* rho0,
                const T* delta0, const T* beta0, const T& freq, const T& amp, const T& speed)
      : d_(std::move(data))
  {
    check(fus_model_create(d_->context()->handle(), KIND, d_->handle(), c0, rho0, delta0, beta0, f.nfacets, f.cells,
                           f.local_facets, f.tags, (double)freq, (double)amp, (double)speed, &h_));
  }

private:
  std::vector<T> get(int which) const
  {
    std::vector<T> out((size_t)d_->ndofs());
    check(fus_model_get(h_, which, out.data(), FUS_HOST));
    return out;
  }
  std::shared_ptr<SpectralOperatorData<T, P>> d_;
  fus_model* h_ = nullptr;
  std::int64_t nrecv_ = 0;
};
} // namespace detail

// c0, rho0 (, delta0, beta0): one value per cell (the reference's DG0 functions); freq, amp, speed:
// sourceFrequency, sourceAmplitude, sourceSpeed of Linear.hpp:55-62.
template <typename T, int P>
class LinearSpectral3D : public detail::SpectralModel<T, P, FUS_LINEAR>
{
public:
  LinearSpectral3D(std::shared_ptr<SpectralOperatorData<T, P>> data, const FacetView& facets, const T* c0,
                   const T* rho0, const T& freq, const T& amp, const T& speed)
      : detail::SpectralModel<T, P, FUS_LINEAR>(std::move(data), facets, c0, rho0, nullptr, nullptr, freq, amp, speed)
  {
  }
};
template <typename T, int P>
using LinearSpectral2D = LinearSpectral3D<T, P>;  // cpp/fenicsx-sf-naive/common/Linear.hpp:52-350

// data must have been created with fields = 2.  Boundary forms: Context::set_option("forms", 0 | 1)
// before construction (fusmi.h).
template <typename T, int P>
class LossySpectral3D : public detail::SpectralModel<T, P, FUS_LOSSY>
{
public:
  LossySpectral3D(std::shared_ptr<SpectralOperatorData<T, P>> data, const FacetView& facets, const T* c0,
                  const T* rho0, const T* delta0, const T& freq, const T& amp, const T& speed)
      : detail::SpectralModel<T, P, FUS_LOSSY>(std::move(data), facets, c0, rho0, delta0, nullptr, freq, amp, speed)
  {
  }
};

template <typename T, int P>
class WesterveltSpectral3D : public detail::SpectralModel<T, P, FUS_WESTERVELT>
{
public:
  WesterveltSpectral3D(std::shared_ptr<SpectralOperatorData<T, P>> data, const FacetView& facets, const T* c0,
                       const T* rho0, const T* delta0, const T* beta0, const T& freq, const T& amp,
                       const T& speed)
      : detail::SpectralModel<T, P, FUS_WESTERVELT>(std::move(data), facets, c0, rho0, delta0, beta0, freq, amp,
                                                    speed)
  {
  }
};

// Pennes bioheat model and CEM43 dose on the operator's mesh (fusmi.h "bioheat"; the reference has no thermal model):
//   rho C dtheta/dt = div(k grad theta) - W theta + Q for the temperature RISE theta over t_base, classical RK4 or,
//   with stages = s in 2..32, the super-time-stepping scheme RKL2 (s operator applications per step, trapezoid dose).
// conductivity, rho_c, perfusion (nullptr = 0): one value per cell.  On operator data with neighbours the context needs an
// RCCL communicator (comm_init), and the constructor, set_heat, set_heat_from, set_boundary, steps, lambda_max and stable_dt
// are collective calls; the members of an in-process group are driven through the C calls fus_group_thermal_* instead.
template <typename T, int P>
class BioheatSpectral3D
{
public:
  BioheatSpectral3D(std::shared_ptr<SpectralOperatorData<T, P>> data, const T* conductivity, const T* rho_c,
                    const T* perfusion = nullptr, double t_base = 37.0)
      : d_(std::move(data))
  {
    check(fus_thermal_create(d_->context()->handle(), d_->handle(), conductivity, rho_c, perfusion, t_base, &h_));
  }
  ~BioheatSpectral3D() { fus_thermal_destroy(h_); }
  BioheatSpectral3D(const BioheatSpectral3D&) = delete;
  BioheatSpectral3D& operator=(const BioheatSpectral3D&) = delete;
  void init() { check(fus_thermal_init(h_)); }  // rise = 0, dose = 0
  void set_state(const T* rise, const double* dose = nullptr)
  {
    if (rise)
      check(fus_thermal_set(h_, FUS_TH_RISE, rise, FUS_HOST));
    if (dose)
      check(fus_thermal_set(h_, FUS_TH_DOSE, dose, FUS_HOST));
  }
  // h = (M(q_coef) 1) .* q: q [ndofs], q_coef [ncells] or nullptr (= 1); q == nullptr: no heat
  void set_heat(const T* q, const T* q_coef = nullptr) { check(fus_thermal_set_heat(h_, q, q_coef, FUS_HOST)); }
  // acoustic heating 2 alpha p_rms^2 / (rho c) from the field monitor of a wave model on the same operator data
  template <typename Model>
  void set_heat_from(const Model& model, const T* absorption)
  {
    check(fus_thermal_set_heat_from_monitor(h_, model.handle(), absorption));
  }
  // per-harmonic heating sum_k 2 alpha_k |p_k|^2 / (2 rho c) from the monitor's harmonics 1..nharm (at most the monitor's
  // own): absorption [nharm][ncells], row k - 1 = alpha at k times the source frequency (fusmi.h, per-harmonic heat load)
  template <typename Model>
  void set_heat_from(const Model& model, const T* absorption, int nharm)
  {
    check(fus_thermal_set_heat_from_harmonics(h_, model.handle(), nharm, absorption));
  }
  // of m_C^-1 (K(k) + diag(phi_max m_W + m_H)) with the fixed DOFs removed (the boundary and the response in force)
  double lambda_max(int iters = 20) const
  {
    double l = 0;
    check(fus_thermal_lambda_max(h_, iters, &l));
    return l;
  }
  // stages = 0: 2 / lambda_max(20), the RK4 step; stages = s: 0.72 (s^2 + s - 2) / (2 lambda_max(20)), the RKL2 step
  double stable_dt(int stages = 0) const
  {
    double dt = 0;
    check(fus_thermal_stable_dt(h_, 20, stages, &dt));
    return dt;
  }
  void steps(double dt, std::int64_t nsteps, double heat_scale = 1.0, int stages = 0)
  {
    check(stages == 0 ? fus_thermal_steps(h_, dt, nsteps, heat_scale)
                      : fus_thermal_steps_sts(h_, dt, nsteps, heat_scale, stages));
  }
  // Boundary conditions, per-DOF arrays in caller numbering, any of them nullptr (fusmi.h "bioheat"): fixed[d] != 0 holds
  // the DOF at the rise fixed_rise[d]; conv_diag = m_H, the facet diagonal of the heat-transfer coefficient h_c
  // (fus_facet_diag on the operator's handle with cellcoef = h_c, summed over the convective faces), conv_rise the coolant's rise
  // over t_base.  Replaces any boundary set before; every other face stays insulating.
  void set_boundary(const std::uint8_t* fixed, const T* fixed_rise, const T* conv_diag, const T* conv_rise)
  {
    check(fus_thermal_set_boundary(h_, fixed, fixed_rise, conv_diag, conv_rise));
  }
  void clear_boundary() { check(fus_thermal_set_boundary(h_, nullptr, nullptr, nullptr, nullptr)); }
  // (number of fixed DOFs, number of convective DOFs) in force
  std::pair<std::int64_t, std::int64_t> boundary_info() const
  {
    std::int64_t nf = 0, nc = 0;
    check(fus_thermal_boundary_info(h_, &nf, &nc));
    return {nf, nc};
  }
  // Perfusion response (fusmi.h "bioheat", perfusion response and damage): each step runs with m_W phi of the state it
  // starts from, phi = P(T) S(D) -- P piecewise linear through up to 8 knots (temp strictly ascending, degrees C;
  // factor >= 0), S falling from 1 at dose_lo to 0 at dose_hi CEM43 minutes (dose_hi <= 0: no shutdown).  Call it before
  // stable_dt, which then takes the largest factor.  clear_response: the passive perfusion again.
  void set_response(const std::vector<double>& temp, const std::vector<double>& factor, double dose_lo = 0.0,
                    double dose_hi = 0.0)
  {
    if (temp.size() != factor.size())
      throw Error(FUS_ERR_ARG, "set_response: temp and factor differ in length");
    check(fus_thermal_set_response(h_, (int)temp.size(), temp.data(), factor.data(), dose_lo, dose_hi));
  }
  void clear_response() { check(fus_thermal_set_response(h_, 0, nullptr, nullptr, 0.0, 0.0)); }
  // Arrhenius damage integral beside the dose, trapezoid rule per step: A in 1/s, Ea in J/mol; A = 0 switches it off
  void set_damage(double A, double Ea) { check(fus_thermal_set_damage(h_, A, Ea)); }
  std::vector<T> rise() const { return get<T>(FUS_TH_RISE); }
  std::vector<T> heat() const { return get<T>(FUS_TH_HEAT); }
  std::vector<double> dose() const { return get<double>(FUS_TH_DOSE); }  // CEM43, minutes
  std::vector<double> damage() const { return get<double>(FUS_TH_DAMAGE); }   // Omega; set_damage must be on
  std::vector<T> perfusion() const { return get<T>(FUS_TH_PERFUSION); }       // m_W phi as the next step will use it
  fus_thermal* handle() const { return h_; }

private:
  template <typename U>
  std::vector<U> get(int which) const
  {
    std::vector<U> out((size_t)d_->ndofs());
    check(fus_thermal_get(h_, which, out.data(), FUS_HOST));
    return out;
  }
  std::shared_ptr<SpectralOperatorData<T, P>> d_;
  fus_thermal* h_ = nullptr;
};
template <typename T, int P>
using BioheatSpectral2D = BioheatSpectral3D<T, P>;  // SpaceView::tdim = 2

// delta = 2 alpha c0^3 / w0^2, alpha in Np/m (Lossy.hpp:375-379)
template <typename T>
T compute_diffusivity_of_sound(const T w0, const T c0, const T alpha)
{
  return 2 * alpha * c0 * c0 * c0 / w0 / w0;
}

} // namespace fusmi
