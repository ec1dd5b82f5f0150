// wave.hip -- the wave models (Linear, Lossy, Westervelt; fusmi.h): setup, the Runge-Kutta stage halves and the one step
// function behind every stepping entry, the graph replay, the field monitor, the receivers, the phased source and the
// C entry points fus_model_*, fus_group_finish_setup / fus_group_rk4_steps and fus_facet_diag.  The kernels only this unit
// launches are in wave_kernels.hpp; what it takes from fusmi.hip (the operator action, the shared-DOF exchange, the
// degree units) is listed in core.hpp.
//
// Reference counterpart: LinearSpectral3D (Linear.hpp:52-347) and its Lossy / Westervelt siblings.
#include <memory>

#include "core.hpp"
#include "wave_kernels.hpp"

using namespace fus;

static_assert(FUS_MAX_PLANES == 16, "fus_set_option (fusmi.hip) accepts \"planes\" up to 16");

// Host builder of the diagonal facet weights (setup)
template <typename T>
static void facet_diag_host(const fus_op* op, int64_t nfacets, const int32_t* fc, const int32_t* fl,
                            const T* cellcoef, T* out)
{
  static const int axis3[6] = {2, 1, 0, 0, 1, 2}, side3[6] = {0, 0, 0, 1, 1, 1};
  const int N = op->N, Nd = op->Nd;
  const T* xg = reinterpret_cast<const T*>(op->h_geom_x.data());
  int i_lo = 0, i_hi = 0;
  for (int i = 0; i < N; ++i)
  {
    if (op->nodes[i] < op->nodes[i_lo])
      i_lo = i;
    if (op->nodes[i] > op->nodes[i_hi])
      i_hi = i;
  }
  if (op->tdim == 2)
  {
    // edges of quadrilaterals (local facet 0: y=0, 1: x=0, 2: x=1, 3: y=1): weight = edge-length
    // element |dx/dX_t| times the 1-D quadrature weight
    static const int axis2[4] = {1, 0, 0, 1}, side2[4] = {0, 0, 1, 1};
    for (int64_t f = 0; f < nfacets; ++f)
    {
      const int64_t cell = fc[f];
      const int ax = axis2[fl[f]], sd = side2[fl[f]], d1 = 1 - ax;
      T cd[9][3];
      const int nv2 = op->geom_nv;
      for (int v = 0; v < nv2; ++v)
        for (int j = 0; j < 3; ++j)
          cd[v][j] = xg[3 * (int64_t)op->h_geom_dm[cell * nv2 + v] + j];
      for (int a = 0; a < N; ++a)
      {
        int idx[2];
        idx[ax] = sd ? i_hi : i_lo, idx[d1] = a;
        T J[2][2];
        if (op->geom_order == 1)
          jacobian2<T>(reinterpret_cast<const T(*)[3]>(cd), op->nodes[idx[0]], op->nodes[idx[1]], J);
        else
          jacobian2_q2<T>(cd, op->nodes[idx[0]], op->nodes[idx[1]], J);
        const T len = (T)std::sqrt((double)(J[0][d1] * J[0][d1] + J[1][d1] * J[1][d1]));
        out[op->h_dofmap[cell * Nd + idx[0] * N + idx[1]]] += cellcoef[cell] * len * (T)op->wts[a];
      }
    }
    return;
  }
  for (int64_t f = 0; f < nfacets; ++f)
  {
    const int64_t cell = fc[f];
    const int ax = axis3[fl[f]], sd = side3[fl[f]];
    const int d1 = (ax + 1) % 3, d2 = (ax + 2) % 3;
    T cd[27][3];
    const int nv = op->geom_nv;
    for (int v = 0; v < nv; ++v)
      for (int j = 0; j < 3; ++j)
        cd[v][j] = xg[3 * (int64_t)op->h_geom_dm[cell * nv + v] + j];
    for (int a = 0; a < N; ++a)
      for (int b = 0; b < N; ++b)
      {
        int idx[3];
        idx[ax] = sd ? i_hi : i_lo, idx[d1] = a, idx[d2] = b;
        T J[3][3];
        if (op->geom_order == 1)
          jacobian3<T>(reinterpret_cast<const T(*)[3]>(cd), op->nodes[idx[0]], op->nodes[idx[1]],
                       op->nodes[idx[2]], J);
        else
          jacobian3_q2<T>(cd, op->nodes[idx[0]], op->nodes[idx[1]], op->nodes[idx[2]], J);
        const T t1[3] = {J[0][d1], J[1][d1], J[2][d1]}, t2[3] = {J[0][d2], J[1][d2], J[2][d2]};
        const T n0 = t1[1] * t2[2] - t1[2] * t2[1], n1 = t1[2] * t2[0] - t1[0] * t2[2],
                n2 = t1[0] * t2[1] - t1[1] * t2[0];
        const T area = (T)std::sqrt((double)(n0 * n0 + n1 * n1 + n2 * n2));
        const int li = (idx[0] * N + idx[1]) * N + idx[2];
        out[op->h_dofmap[cell * Nd + li]] += cellcoef[cell] * area * (T)(op->wts[a] * op->wts[b]);
      }
  }
}

template <typename T>
static int model_setup(fus_model* m, const void* c0_, const void* rho0_, const void* delta0_,
                       const void* beta0_, int64_t nfacets, const int32_t* fc, const int32_t* fl,
                       const int32_t* ft)
{
  fus_op* op = m->op;
  fus_ctx* c = m->ctx;
  hipStream_t st = c->stream;
  const Layout& L = op->L;
  const int64_t n = L.n_internal;
  const T* c0 = static_cast<const T*>(c0_);
  const T* rho0 = static_cast<const T*>(rho0_);
  const T* delta0 = static_cast<const T*>(delta0_);
  const bool lossy = m->kind == FUS_LOSSY || m->kind == FUS_WESTERVELT;
  const T* beta0 = static_cast<const T*>(beta0_);
  auto& pool = m->allocs;
  for (void** v : {&m->u0, &m->v0, &m->u_, &m->v_, &m->un, &m->vn, &m->b, &m->minv, &m->m})
    FUSCHK(dalloc_bytes(pool, v, n * sizeof(T), true, st));

  // operator coefficients -1/rho (Linear.hpp:154-155) [and -delta/(rho c^2), Lossy.hpp:166-169]
  // and the mass coefficient 1/(rho c^2) (forms.py:36), internal element order
  std::vector<T> coef(op->ncells), coef2(lossy ? op->ncells : 0), mcoef(op->ncells), c0i(op->ncells), rho0i(op->ncells);
  for (int64_t e = 0; e < op->ncells; ++e)
  {
    const int64_t cell = L.cell_perm[e];
    c0i[e] = c0[cell], rho0i[e] = rho0[cell];
    coef[e] = T(-1.0) / rho0[cell];
    if (lossy)
      coef2[e] = -delta0[cell] / rho0[cell] / c0[cell] / c0[cell];
    mcoef[e] = T(1.0) / rho0[cell] / c0[cell] / c0[cell];
  }
  T *d_coef, *d_coef2 = nullptr, *d_mcoef;
  FUSCHK(upload(pool, &d_coef, coef, st));
  if (lossy)
    FUSCHK(upload(pool, &d_coef2, coef2, st));
  FUSCHK(upload(pool, &d_mcoef, mcoef, st));
  m->coef = d_coef, m->coef2 = d_coef2, m->mcoef = d_mcoef;
  T *d_c0i, *d_rho0i;
  FUSCHK(upload(pool, &d_c0i, c0i, st));
  FUSCHK(upload(pool, &d_rho0i, rho0i, st));
  m->d_c0 = d_c0i, m->d_rho0 = d_rho0i;

  // lumped mass, this rank's cells only: m = M(1/(rho c^2)) 1  (Linear.hpp:127-133)
  T* ones = static_cast<T*>(m->un);
  hipLaunchKernelGGL((k_fill<T>), dim3(1024), dim3(256), 0, st, n, ones, T(1));
  FUSCHK(d_apply_internal(op, OP_MASS, d_mcoef, ones, m->m));
  if (m->kind == FUS_WESTERVELT)
  {
    // diagonal of the nonlinear mass action: mn1 = M(-2 beta/(rho^2 c^4)) 1  (Westervelt.hpp:185,
    // 249-254); nlin2 = -nlin1 (:186), so the RHS term is -mn1 .* v_n^2
    std::vector<T> n1(op->ncells);
    for (int64_t e = 0; e < op->ncells; ++e)
    {
      const int64_t cell = L.cell_perm[e];
      const T cc = c0[cell], rr = rho0[cell];
      n1[e] = T(-2.0) * beta0[cell] / rr / rr / cc / cc / cc / cc;
    }
    T* d_n1;
    FUSCHK(upload(pool, &d_n1, n1, st));
    FUSCHK(dalloc_bytes(pool, &m->mn1, n * sizeof(T), true, st));
    FUSCHK(d_apply_internal(op, OP_MASS, d_n1, ones, m->mn1));
  }
  HIPCHK(hipMemsetAsync(m->un, 0, n * sizeof(T), st));

  // boundary weights of this rank's facets (diagonal: GLL collocation)
  //   Linear (SC1-BM1/forms.py:38-39): src = (1/rho) w_f on tag 1, abs = (1/(rho c)) w_f on tag 2
  //   Lossy  (BM7-SC1/forms.py:37-42): abs on EVERY boundary facet, src2 = (delta/(rho c^2)) w_f on
  //   tag 1 (dg term) and the mass gains (delta/(rho c^3)) w_f on every boundary facet
  std::vector<T> src(op->ndofs, T(0)), absb(op->ndofs, T(0)), src2, mb;
  std::vector<T> cs(op->ncells), ca(op->ncells), cs2, cm;
  for (int64_t k = 0; k < op->ncells; ++k)
    cs[k] = T(1.0) / rho0[k], ca[k] = T(1.0) / rho0[k] / c0[k];
  if (lossy)
  {
    src2.assign(op->ndofs, T(0)), mb.assign(op->ndofs, T(0));
    cs2.resize(op->ncells), cm.resize(op->ncells);
    for (int64_t k = 0; k < op->ncells; ++k)
    {
      cs2[k] = delta0[k] / rho0[k] / c0[k] / c0[k];
      cm[k] = delta0[k] / rho0[k] / c0[k] / c0[k] / c0[k];
    }
  }
  std::vector<int32_t> c1, l1, c2, l2;
  for (int64_t f = 0; f < nfacets; ++f)
  {
    if (fc[f] < 0 || fc[f] >= op->ncells || fl[f] < 0 || fl[f] > 5)
      return fail(FUS_ERR_ARG, "facet (cell, local facet) out of range");
    if (ft[f] == 1)
      c1.push_back(fc[f]), l1.push_back(fl[f]);
    if ((lossy && m->forms == 0) || ft[f] == 2)
      c2.push_back(fc[f]), l2.push_back(fl[f]);   // lossy, C++ forms: plain ds = every listed facet
  }
  facet_diag_host<T>(op, (int64_t)c1.size(), c1.data(), l1.data(), cs.data(), src.data());
  facet_diag_host<T>(op, (int64_t)c2.size(), c2.data(), l2.data(), ca.data(), absb.data());
  if (lossy)
  {
    facet_diag_host<T>(op, (int64_t)c1.size(), c1.data(), l1.data(), cs2.data(), src2.data());
    facet_diag_host<T>(op, (int64_t)c2.size(), c2.data(), l2.data(), cm.data(), mb.data());
  }
  T* tmpc = static_cast<T*>(op->d_tmp_c);
  // scratch until fus_model_init: full-length src / abs / src2 weights; b holds the mass term
  void* dst[4] = {m->u_, m->v_, m->vn, m->b};
  std::vector<T>* hv[4] = {&src, &absb, &src2, &mb};
  for (int k = 0; k < (lossy ? 4 : 2); ++k)
  {
    HIPCHK(hipMemcpyAsync(tmpc, hv[k]->data(), op->ndofs * sizeof(T), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_to_internal<T>), dim3(nblk(op->ndofs)), dim3(256), 0, st, op->ndofs,
                       op->d_dof_perm, tmpc, static_cast<T*>(dst[k]));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (lossy)
  {
    hipLaunchKernelGGL((k_add_vec<T>), dim3(1024), dim3(256), 0, st, n, static_cast<const T*>(m->b),
                       static_cast<T*>(m->m));
    HIPCHK(hipMemsetAsync(m->b, 0, n * sizeof(T), st));
  }
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

// Setup vectors: m (needs the sharers' contributions, m.scatter_rev(+), Linear.hpp:134), src
// weights (parked in u_) and abs weights (parked in v_) of this rank's own facets
static void* setup_halo_vector(fus_model* m, int k) { return k == 0 ? m->m : (k == 1 ? m->mn1 : m->v_); }

// The boundary-entry lists: every internal dof with a non-zero source or absorbing weight, sorted by internal index --
// bidx, nb, nb_int, d_blk_bnd_off, the pseudo pairs appended to d_sh_ptr32 / d_sh_pairs32, d_bnd_mask / d_bnd_base and
// the weights d_bsrc, d_babs (and d_bsrc2).  Built from the facet weights the setup left (ModelSource::h_f*) plus `vol`,
// the caller's source weights in internal numbering (n_internal long; nullptr: none), which add to the src part only.
// The lists are built beside those in force and replace them at the end: an error leaves the model as it was.  The setup
// and fus_model_set_source_weights both end here.
template <typename T>
static int model_build_entries(fus_model* m, const T* vol)
{
  fus_op* op = m->op;
  hipStream_t st = m->ctx->stream;
  const Layout& L = op->L;
  const int64_t n = L.n_internal;
  const bool lossy = m->kind == FUS_LOSSY || m->kind == FUS_WESTERVELT;
  HIPCHK(hipStreamSynchronize(st));
  std::vector<int32_t> bidx;
  std::vector<T> bsrc, babs, bsrc2;
  {
    size_t f = 0;
    const size_t nf = m->src.h_fidx.size();
    auto entry = [&](int64_t i, T s, T a, T s2)
    {
      bidx.push_back((int32_t)i), bsrc.push_back(s), babs.push_back(a);
      if (lossy)
        bsrc2.push_back(s2);
    };
    if (!vol)
      for (; f < nf; ++f)
        entry(m->src.h_fidx[f], (T)m->src.h_fsrc[f], (T)m->src.h_fabs[f], lossy ? (T)m->src.h_fsrc2[f] : T(0));
    else
      for (int64_t i = 0; i < n; ++i)
      {
        const bool facet = f < nf && m->src.h_fidx[f] == i;
        if (facet)
          entry(i, (T)m->src.h_fsrc[f] + vol[i], (T)m->src.h_fabs[f], lossy ? (T)m->src.h_fsrc2[f] : T(0)), ++f;
        else if (vol[i] != T(0))
          entry(i, vol[i], T(0), T(0));
      }
  }
  ModelEntries F;
  const char* what = "boundary-entry lists";
  F.nb = (int64_t)bidx.size();
  {
    F.nb_int = std::lower_bound(bidx.begin(), bidx.end(), (int32_t)L.n_int_pad) - bidx.begin();
    std::vector<int32_t> off(L.nblocks + 1);
    for (int32_t b = 0; b < L.nblocks; ++b)
      off[b] = (int32_t)(std::lower_bound(bidx.begin(), bidx.begin() + F.nb_int, L.blk_int_off[b])
                         - bidx.begin());
    off[L.nblocks] = (int32_t)F.nb_int;
    FUSCHK(upload(F.d_blk_bnd_off, off, st, what));
    // shared CSR of this model: where the op's pairs keep their partial sums + one trailing pseudo pair (slot
    // n_partial + k) for the k-th shared boundary dof, so the boundary term is the last addend like
    // Linear.hpp:204-205
    if (L.n_partial + L.n_shared > 2000000000ll)
      return fail(FUS_ERR_LIMIT, "partial slab exceeds int32 indexing");
    std::vector<int32_t> extra(L.n_shared, -1);
    for (int64_t k = F.nb_int; k < F.nb; ++k)
      extra[bidx[k] - L.n_int_pad] = (int32_t)(L.n_partial + (k - F.nb_int));
    std::vector<int32_t> ptr(L.n_shared + 1), prs;
    prs.reserve(L.npairs + (F.nb - F.nb_int));
    for (int64_t sidx = 0; sidx < L.n_shared; ++sidx)
    {
      ptr[sidx] = (int32_t)prs.size();
      for (int64_t k = L.sh_ptr[sidx]; k < L.sh_ptr[sidx + 1]; ++k)
        prs.push_back(L.pair_pos[L.sh_pairs[k]]);
      if (extra[sidx] >= 0)
        prs.push_back(extra[sidx]);
    }
    ptr[L.n_shared] = (int32_t)prs.size();
    FUSCHK(upload(F.d_sh_ptr32, ptr, st, what));
    FUSCHK(upload(F.d_sh_pairs32, prs, st, what));
    // the same for the plane form of the rank-local shared dofs (k_shared_stage_planes): one bit per dof and the
    // number of boundary dofs ahead of each 64-dof word (bidx ascends, so the k-th set bit is the k-th term)
    if (F.nb > F.nb_int && L.n_shared_local > 0)
    {
      const int64_t nw = (L.n_shared_local + 63) / 64;
      std::vector<uint64_t> mask(nw, 0);
      std::vector<int32_t> base(nw, 0);
      for (int64_t sidx = 0; sidx < L.n_shared_local; ++sidx)
        if (extra[sidx] >= 0)
          mask[sidx >> 6] |= 1ull << (sidx & 63);
      // boundary dofs of the interface range come after every local one in bidx, so the local ranks start at 0
      for (int64_t w = 1; w < nw; ++w)
        base[w] = base[w - 1] + __builtin_popcountll(mask[w - 1]);
      FUSCHK(upload(F.d_bnd_mask, mask, st, what));
      FUSCHK(upload(F.d_bnd_base, base, st, what));
    }
  }
  FUSCHK(upload(F.d_bidx, bidx, st, what));
  FUSCHK(upload(F.d_bsrc, bsrc, st, what));
  FUSCHK(upload(F.d_babs, babs, st, what));
  if (lossy)
    FUSCHK(upload(F.d_bsrc2, bsrc2, st, what));
  HIPCHK(hipStreamSynchronize(st));   // the host vectors leave scope; no kernel reads the previous lists (synchronised above)
  m->bnd = std::move(F);
  return FUS_OK;
}

template <typename T>
static int model_setup_finish(fus_model* m)
{
  fus_op* op = m->op;
  hipStream_t st = m->ctx->stream;
  const int64_t n = op->L.n_internal;
  hipLaunchKernelGGL((k_reciprocal<T>), dim3(nblk(n)), dim3(256), 0, st, n,
                     static_cast<const T*>(m->m), static_cast<T*>(m->minv));
  const bool lossy = m->kind == FUS_LOSSY || m->kind == FUS_WESTERVELT;
  std::vector<T> src(n), absb(n), src2(lossy ? n : 0);
  HIPCHK(hipMemcpyAsync(src.data(), m->u_, n * sizeof(T), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(absb.data(), m->v_, n * sizeof(T), hipMemcpyDeviceToHost, st));
  if (lossy)
    HIPCHK(hipMemcpyAsync(src2.data(), m->vn, n * sizeof(T), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  m->src.h_fidx.clear(), m->src.h_fsrc.clear(), m->src.h_fabs.clear(), m->src.h_fsrc2.clear();
  for (int64_t i = 0; i < n; ++i)
    if (src[i] != T(0) || absb[i] != T(0) || (lossy && src2[i] != T(0)))
    {
      m->src.h_fidx.push_back((int32_t)i);
      m->src.h_fsrc.push_back((double)src[i]);
      m->src.h_fabs.push_back((double)absb[i]);
      if (lossy)
        m->src.h_fsrc2.push_back((double)src2[i]);
    }
  FUSCHK(model_build_entries<T>(m, nullptr));
  HIPCHK(hipMemsetAsync(m->u_, 0, n * sizeof(T), st));
  HIPCHK(hipMemsetAsync(m->v_, 0, n * sizeof(T), st));
  HIPCHK(hipMemsetAsync(m->vn, 0, n * sizeof(T), st));
  HIPCHK(hipStreamSynchronize(st));
  m->setup_done = true;
  return FUS_OK;
}

struct StageScalars
{
  double gval, dgval, adt, bdt;
  double b0dt, pdt;    // dt b_0 and dt a_i (lean RK4 stage kinds: the stage's input is u0 + pdt V_{i-1})
  double tn;  // the stage's time t + c_i dt as the scalars above saw it (in T)
};

// source scalar g(t_n) (Linear.hpp:185-192) and the stage's axpy factors (:282-294), in T
template <typename T>
static StageScalars stage_scalars(const fus_model* m, int i, double t_, double dt_)
{
  const T t = (T)t_, dt = (T)dt_;
  // Runge-Kutta tables (_linear.py:286-311): forward Euler, Ralston 2nd / 3rd order, classical RK4
  // (Linear.hpp:263-265); a_runge carries one trailing 0 for "the stage after the last"
  T a_runge[5] = {0.0, 0.5, 0.5, 1.0, 0.0};
  T b_runge[4] = {(T)(1.0 / 6.0), (T)(1.0 / 3.0), (T)(1.0 / 3.0), (T)(1.0 / 6.0)};
  T c_runge[4] = {0.0, 0.5, 0.5, 1.0};
  if (m->rk_order == 1)
  {
    a_runge[0] = 0, a_runge[1] = 0, b_runge[0] = 1, c_runge[0] = 0;
  }
  else if (m->rk_order == 2)
  {
    a_runge[0] = 0, a_runge[1] = (T)(2.0 / 3.0), a_runge[2] = 0;
    b_runge[0] = (T)(1.0 / 4.0), b_runge[1] = (T)(3.0 / 4.0);
    c_runge[0] = 0, c_runge[1] = (T)(2.0 / 3.0);
  }
  else if (m->rk_order == 3)
  {
    a_runge[0] = 0, a_runge[1] = (T)(1.0 / 2.0), a_runge[2] = (T)(3.0 / 4.0), a_runge[3] = 0;
    b_runge[0] = (T)(2.0 / 9.0), b_runge[1] = (T)(1.0 / 3.0), b_runge[2] = (T)(4.0 / 9.0);
    c_runge[0] = 0, c_runge[1] = (T)(1.0 / 2.0), c_runge[2] = (T)(3.0 / 4.0);
  }
  const T freq = (T)m->freq, p0 = (T)m->amp, s0 = (T)m->speed;
  const T w0 = (T)(2 * M_PI * m->freq);
  const T period = (T)(1.0 / m->freq), window_length = (T)4.0;
  const T tn = t + c_runge[i] * dt;
  T window, dwindow;
  if (tn < period * window_length)
  {
    window = (T)(0.5 * (1.0 - std::cos((double)(freq * (T)M_PI * tn / window_length))));
    dwindow = (T)(0.5 * M_PI) * freq / window_length
              * (T)std::sin((double)(freq * (T)M_PI * tn / window_length));
  }
  else
    window = 1.0, dwindow = 0.0;
  StageScalars sc;
  if (m->kind == FUS_LOSSY || m->kind == FUS_WESTERVELT)
  {
    // heterogeneous-domain scaling, live in Lossy.hpp:216-220 (factor 2) and its derivative dg
    const T two = m->forms == 0 ? (T)2.0 : (T)1.0;  // "heterogenous domain" doubling, Lossy.hpp:216-220
    sc.gval = (double)(window * two * p0 * w0 / s0 * (T)std::cos((double)(w0 * tn)));
    sc.dgval = (double)(dwindow * two * p0 * w0 / s0 * (T)std::cos((double)(w0 * tn))
                        - window * two * p0 * w0 * w0 / s0 * (T)std::sin((double)(w0 * tn)));
  }
  else
  {
    sc.gval = (double)(window * p0 * w0 / s0 * (T)std::cos((double)(w0 * tn)));  // Linear.hpp:192
    sc.dgval = 0.0;
  }
  sc.adt = (double)(dt * a_runge[i + 1]);
  sc.bdt = (double)(dt * b_runge[i]);
  sc.b0dt = (double)(dt * b_runge[0]);
  sc.pdt = (double)(dt * a_runge[i]);
  sc.tn = (double)tn;
  return sc;
}

// Which fused-update variant stage i uses: STAGE_FIRST (reads u0, v0 only), STAGE_MID, STAGE_LAST = last stage of RK4
// (writes the new u0, v0 directly).  The lower-order schemes end on a middle stage and swap (u_, v_) with (u0, v0) afterwards.
static int stage_kind(const fus_model* m, int i)
{
  if (m->rk_order == 4 && m->lean_rk4)   // classical RK4 without accumulator streams (kernels.hpp, stage kinds 4-7)
    return STAGE_LEAN0 + i;
  if (i == 0)
    return STAGE_FIRST;
  return (m->rk_order == 4 && i == 3) ? STAGE_LAST : STAGE_MID;
}
// (every kind stage_kind returns is in FUS_STAGE_KINDS, host.hpp: the instantiations of the stage kernels)

// The stage's velocity buffers as the fused updates name them.  Stage kinds 0, 1, 3: the model's own vn, v_, u_.
// Lean RK4 (kinds 4-7): the three stage velocities V_1, V_2, V_3 rotate through those three buffers (A = vn, B = v_,
// C = u_): `vn` is the velocity this stage starts from (read; stage 0 starts from v0), `v_` the one it leaves for the
// next stage (written; at stage 3: V_2, read) and `u_` is V_1 (read at stages 2 and 3).
template <typename T>
struct StageVel
{
  T *vn, *v_, *u_;
};
template <typename T>
static StageVel<T> stage_vel(const fus_model* m, int i)
{
  T *A = static_cast<T*>(m->vn), *B = static_cast<T*>(m->v_), *C = static_cast<T*>(m->u_);
  if (!(m->rk_order == 4 && m->lean_rk4))
    return {A, B, C};
  switch (i)
  {
  case 0: return {A, A, C};   // writes V_1 -> A
  case 1: return {A, B, C};   // reads V_1, writes V_2 -> B
  case 2: return {B, C, A};   // reads V_2 and V_1, writes V_3 -> C
  default: return {C, B, A};  // reads V_3, V_2 and V_1
  }
}

template <typename T>
static StageArgs<T> stage_args(fus_model* m, int i, const StageScalars& sc)
{
  StageArgs<T> S;
  const StageVel<T> V = stage_vel<T>(m, i);
  S.minv = static_cast<const T*>(m->minv);
  S.vn = V.vn, S.un = static_cast<T*>(m->un);
  S.u0 = static_cast<T*>(m->u0), S.v0 = static_cast<T*>(m->v0);
  S.u_ = V.u_, S.v_ = V.v_;
  S.adt = (T)sc.adt, S.bdt = (T)sc.bdt, S.gval = (T)sc.gval;
  S.b0dt = (T)sc.b0dt, S.pdt = (T)sc.pdt, S.third = T(1) / T(3);
  S.blk_bnd_off = m->bnd.d_blk_bnd_off.as<int32_t>(), S.bnd_idx = m->bnd.d_bidx.as<int32_t>();
  S.bnd_src = m->bnd.d_bsrc.as<const T>(), S.bnd_abs = m->bnd.d_babs.as<const T>();
  S.x2 = nullptr, S.coef2 = static_cast<const T*>(m->coef2);
  S.bnd_src2 = m->bnd.d_bsrc2.as<const T>(), S.dgval = (T)sc.dgval;
  S.m0 = static_cast<const T*>(m->m), S.mn1 = static_cast<const T*>(m->mn1);
  return S;
}

// Per-entry source (src.mode 2, and 3 with the sampled signals): the weight arrays of the entries [k0, k1) for the stage
// time tn.  The rule of the callers: before a kernel reads a range of d_bsrc / d_bsrc2, the range holds the values for the
// time whose scalar that kernel would have carried -- the block kernel and k_boundary_partial the stage's own time, the
// shared-dof and interface stage kernels (BndNext) the next stage's.
template <typename T>
static int source_entries(fus_model* m, int64_t k0, int64_t k1, double tn)
{
  if (k1 <= k0)
    return FUS_OK;
  const bool lossy = m->kind == FUS_LOSSY || m->kind == FUS_WESTERVELT;
  const ModelSource::Arrays& A = m->src.d;
  T *out = m->bnd.d_bsrc.as<T>(), *out2 = m->bnd.d_bsrc2.as<T>();
  if (m->src.mode == 3)
  {
    ProfScope ps(m->ctx, "source_signal");
    hipLaunchKernelGGL((k_source_entries_signal<T>), dim3(nblk(k1 - k0)), dim3(256), 0, m->ctx->stream, k0, k1,
                       A.base.as<const T>(), A.base2.as<const T>(), A.amp.as<const T>(), A.tau.as<const T>(),
                       A.chan.as<int32_t>(), A.table.as<double>(), m->src.sig, tn, out, out2);
  }
  else
  {
    const SourceWave W = source_wave_make(m->freq, m->amp, m->speed, (lossy && m->forms == 0) ? 2.0 : 1.0, m->src.dur);
    ProfScope ps(m->ctx, "source");
    hipLaunchKernelGGL((k_source_entries<T>), dim3(nblk(k1 - k0)), dim3(256), 0, m->ctx->stream, k0, k1,
                       A.base.as<const T>(), A.base2.as<const T>(), A.amp.as<const T>(), A.tau.as<const T>(), W, tn, out, out2);
  }
  HIPCHK(hipGetLastError());
  if (k0 == 0)
    m->src.tn_int = tn;
  if (k1 == m->bnd.nb)
    m->src.tn_sh = tn;
  return FUS_OK;
}

// Stage i, first half: the block kernel applies K(-1/rho) to u_stage and, for every block-interior
// dof, finishes the stage right away (boundary terms, kv = b/m, axpys); shared dofs leave as partial
// sums, are reduced into b's shared range, and the interface entries are packed for the exchange.
template <typename T>
static int stage_begin(fus_model* m, int i, double t, double dt)
{
  fus_op* op = m->op;
  const T* ustage = static_cast<const T*>(i == 0 ? m->u0 : m->un);  // a_0 = 0: un == u0
  T* b = static_cast<T*>(m->b);
  const StageScalars sc_now = stage_scalars<T>(m, i, t, dt);
  StageArgs<T> S = stage_args<T>(m, i, sc_now);
  const T* vstage = i == 0 ? static_cast<const T*>(m->v0) : S.vn;   // the velocity this stage starts from
  S.x2 = vstage;   // lossy: second operator input v_n
  const int kind = stage_kind(m, i);
  const bool two_fields = m->kind == FUS_LOSSY || m->kind == FUS_WESTERVELT;
  const DegreeImpl* deg = degree_impl(op->dtype, op->P);
  auto launch = [&](int b0, int nb) -> int
  { return deg->block_op(op, OP_STIFFNESS, kind, two_fields ? 2 : 1, op->d_G, m->coef, ustage, b, &S, b0, nb); };
  // Multi-rank, option "overlap_blocks": the blocks that touch interface dofs (first in the layout)
  // run ahead, their partials are reduced, packed and handed to the exchange, and the remaining
  // blocks (the bulk of the stage) run while the planes are in flight.  Off by default: the exchange
  // already overlaps k_shared_stage, and on one GPU with the exchange looped back the extra small
  // launch costs more (2.47 vs 2.41 ms per step at 64^3 p=4) than it hides.  A block's epilogue only writes that block's interior dofs,
  // which no other block and none of the small kernels below reads.
  // boundary terms of the shared boundary dofs: a launch of their own unless the previous stage left them (below)
  const int64_t nbs = m->bnd.nb - m->bnd.nb_int;
  const bool bnd_launch = nbs > 0 && !(m->bnd_valid && op->bnd_owner == m && m->bnd_tn == sc_now.tn);
  if (m->src.mode >= 2)   // 2: the analytic waveform per entry, 3: sampled signals
  {
    // the source rides in the weights: the block-interior entries for this stage's time, the shared ones too when
    // k_boundary_partial reads them; in the steady RK4 state the previous stage_end has left both
    S.gval = T(1), S.dgval = T(1);
    const bool need_int = !(m->src.tn_int == sc_now.tn), need_sh = bnd_launch && !(m->src.tn_sh == sc_now.tn);
    if (need_int || need_sh)
      FUSCHK(source_entries<T>(m, need_int ? 0 : m->bnd.nb_int, need_sh ? m->bnd.nb : m->bnd.nb_int, sc_now.tn));
  }
  const int nb_if = op->L.nblocks_if;
  const bool split = m->ctx->overlap_blocks && !op->neigh.empty() && nb_if > 0 && nb_if < op->L.nblocks;
  {
    ProfScope ps(m->ctx, split ? "stiffness_if" : "stiffness");
    FUSCHK(launch(0, split ? nb_if : -1));
  }
  // boundary terms of the shared boundary dofs become one more partial each
  hipStream_t st = m->ctx->stream;
  if (bnd_launch)
  {
    ProfScope ps(m->ctx, "boundary");
    hipLaunchKernelGGL((k_boundary_partial<T>), dim3(nblk(nbs)), dim3(256), 0, st, nbs,
                       S.bnd_idx + m->bnd.nb_int, S.bnd_src + m->bnd.nb_int, S.bnd_abs + m->bnd.nb_int, S.gval,
                       S.bnd_src2 ? S.bnd_src2 + m->bnd.nb_int : nullptr, S.dgval, vstage,
                       static_cast<T*>(op->d_partial) + op->L.n_partial);
  }
  // interface dofs (held by other ranks too): this rank's partials are summed into b and into the
  // send buffer by one kernel; the event hands the buffer to the exchange
  if (!op->neigh.empty())
  {
    ProfScope ps(m->ctx, "halo");
    hipLaunchKernelGGL((k_if_reduce_pack<T>), dim3(nblk(op->n_halo)), dim3(256), 0, st, op->n_halo,
                       op->d_pack_idx, op->L.n_int_pad, m->bnd.d_sh_ptr32.as<int32_t>(), m->bnd.d_sh_pairs32.as<int32_t>(),
                       static_cast<const T*>(op->d_partial), b, static_cast<T*>(op->d_sendbuf));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(m->ctx->ev_packed, st));
  }
  HIPCHK(hipGetLastError());
  if (split)
  {
    ProfScope ps(m->ctx, "stiffness");
    FUSCHK(launch(nb_if, op->L.nblocks - nb_if));
  }
  return FUS_OK;
}

// Stage i, second half, shared dofs only.  Rank-local shared dofs: fixed-order sum of the block
// partials fused with the stage update (k_shared_stage).  Interface dofs: ordered sum of the
// sharers' totals fused with the same update (k_if_unpack_stage).
template <typename T>
static int stage_end(fus_model* m, int i, double t, double dt)
{
  fus_op* op = m->op;
  fus_ctx* c = m->ctx;
  hipStream_t st = c->stream;
  const StageScalars sc = stage_scalars<T>(m, i, t, dt);
  const T adt = (T)sc.adt, bdt = (T)sc.bdt;
  const StageVel<T> V = stage_vel<T>(m, i);
  T *u0 = static_cast<T*>(m->u0), *v0 = static_cast<T*>(m->v0), *u_ = V.u_, *v_ = V.v_,
    *un = static_cast<T*>(m->un), *vn = V.vn, *b = static_cast<T*>(m->b);
  const T* minv = static_cast<const T*>(m->minv);
  const T* partial = static_cast<const T*>(op->d_partial);
  const int64_t off = op->L.n_int_pad, nloc = op->L.n_shared_local;
  const int32_t *sh_ptr32 = m->bnd.d_sh_ptr32.as<int32_t>(), *sh_pairs32 = m->bnd.d_sh_pairs32.as<int32_t>();
  // Westervelt: m0 and mn1 on the shared range (nullptr otherwise)
  const T* m0p = m->mn1 ? static_cast<const T*>(m->m) + off : nullptr;
  const T* mn1p = m->mn1 ? static_cast<const T*>(m->mn1) + off : nullptr;
  // RK4: this stage's kernels also leave the next stage's boundary terms of the shared boundary dofs
  // in their pseudo partial slots (next stage of this step, or stage 0 of the next step at t + dt,
  // advanced the way the step loops do: in T for fus_model_rk4, whose t is a T)
  BndNext<T> B{};
  const int64_t nbs = m->bnd.nb - m->bnd.nb_int;
  m->bnd_valid = false;
  if (m->rk_order == 4 && nbs > 0 && op->L.n_partial + nbs < INT32_MAX)
  {
    const StageScalars scn = i < 3 ? stage_scalars<T>(m, i + 1, t, dt)
                                   : stage_scalars<T>(m, 0, (double)((T)t + (T)dt), dt);
    B.enabled = 1, B.npairs = (int32_t)op->L.n_partial;
    B.srcw = m->bnd.d_bsrc.as<const T>() + m->bnd.nb_int;
    B.absw = m->bnd.d_babs.as<const T>() + m->bnd.nb_int;
    B.src2w = m->bnd.d_bsrc2 ? m->bnd.d_bsrc2.as<const T>() + m->bnd.nb_int : nullptr;
    B.gnext = (T)scn.gval, B.dgnext = (T)scn.dgval;
    B.partial = static_cast<T*>(op->d_partial);
    m->bnd_valid = true, m->bnd_tn = scn.tn;
    op->bnd_owner = m;
    if (m->src.mode >= 2)
    {
      // the kernels below read the shared entries for the next stage's time; the same launch leaves the
      // block-interior entries for the next stage's block kernel (this stage's has run: same stream)
      B.gnext = T(1), B.dgnext = T(1);
      const bool need_int = !(m->src.tn_int == scn.tn);
      if (need_int || !(m->src.tn_sh == scn.tn))
        FUSCHK(source_entries<T>(m, need_int ? 0 : m->bnd.nb_int, m->bnd.nb, scn.tn));
    }
  }
  const LeanRK<T> R{(T)sc.b0dt, (T)sc.pdt, T(1) / T(3)};
  const int kind = stage_kind(m, i);
  if (nloc > 0 && c->planes && (int)op->L.plane_cnt.size() <= (c->planes == 1 ? FUS_MAX_PLANES : c->planes))
  {
    ProfScope ps(c, "stage");
    constexpr int W = 16 / (int)sizeof(T);   // dofs per thread: 16-byte accesses
    const dim3 grid(nblk((nloc + W - 1) / W)), blk(256);
    PartialPlanes PL{};
    PL.bnd0 = (int32_t)op->L.n_partial;
    for (size_t j = 0; j < op->L.plane_cnt.size(); ++j)
      PL.cnt[j] = (int32_t)op->L.plane_cnt[j], PL.off[j] = (int32_t)op->L.plane_off[j];
    FUSCHK(with_kind<FUS_STAGE_KINDS>(kind, [&](auto K) -> int
    {
      hipLaunchKernelGGL((k_shared_stage_planes<T, decltype(K)::value>), grid, blk, 0, st, nloc, PL,
                         m->bnd.d_bnd_mask.as<uint64_t>(), m->bnd.d_bnd_base.as<int32_t>(),
                         partial, minv + off, vn + off, un + off, u0 + off, v0 + off, u_ + off, v_ + off, adt, bdt,
                         m0p, mn1p, B, R);
      return FUS_OK;
    }));
  }
  else if (nloc > 0)
  {
    ProfScope ps(c, "stage");
    const dim3 grid(nblk(nloc)), blk(256);
    FUSCHK(with_kind<FUS_STAGE_KINDS>(kind, [&](auto K) -> int
    {
      hipLaunchKernelGGL((k_shared_stage<T, decltype(K)::value>), grid, blk, 0, st, nloc, sh_ptr32, sh_pairs32, partial,
                         minv + off, vn + off, un + off, u0 + off, v0 + off, u_ + off, v_ + off, adt, bdt, m0p, mn1p, B,
                         R);
      return FUS_OK;
    }));
  }
  if (!op->neigh.empty())
  {
    // (the rank-local shared dofs above ran while the interface planes were in flight)
    // ordered sum of the sharers' totals fused with the stage update of the interface dofs
    if (!c->local_group)
      HIPCHK(hipStreamWaitEvent(st, c->ev_recv, 0));
    ProfScope ps(c, "stage");
    const dim3 grid(nblk(op->n_uidx)), blk(256);
    const T* recv = static_cast<const T*>(op->d_recvbuf);
    const T* m0f = m->mn1 ? static_cast<const T*>(m->m) : nullptr;
    const T* mn1f = m->mn1 ? static_cast<const T*>(m->mn1) : nullptr;
    FUSCHK(with_kind<FUS_STAGE_KINDS>(kind, [&](auto K) -> int
    {
      hipLaunchKernelGGL((k_if_unpack_stage<T, decltype(K)::value>), grid, blk, 0, st, op->n_uidx, op->d_uidx, op->d_uptr, op->d_usrc,
                         recv, b, minv, vn, un, u0, v0, u_, v_, adt, bdt, m0f, mn1f, op->L.n_int_pad, sh_ptr32, sh_pairs32, B, R);
      return FUS_OK;
    }));
  }
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

// One of the model's internal vectors (u0, v0, m) to the caller's numbering, or the caller's vector into it
template <typename T>
static int model_getset(fus_model* m, void* vec_, void* host_or_dev, int space, bool set)
{
  fus_op* op = m->op;
  hipStream_t st = m->ctx->stream;
  T* vec = static_cast<T*>(vec_);
  T* tc = static_cast<T*>(op->d_tmp_c);
  if (set)
  {
    const T* src = static_cast<const T*>(host_or_dev);
    if (space == FUS_HOST)
    {
      HIPCHK(hipMemcpyAsync(tc, host_or_dev, op->ndofs * sizeof(T), hipMemcpyHostToDevice, st));
      src = tc;
    }
    hipLaunchKernelGGL((k_to_internal<T>), dim3(nblk(op->ndofs)), dim3(256), 0, st, op->ndofs,
                       op->d_dof_perm, src, vec);
  }
  else
  {
    T* dst = space == FUS_HOST ? tc : static_cast<T*>(host_or_dev);
    hipLaunchKernelGGL((k_from_internal<T, 0>), dim3(nblk(op->ndofs)), dim3(256), 0, st, op->ndofs,
                       op->d_dof_perm, vec, dst);
    if (space == FUS_HOST)
      HIPCHK(hipMemcpyAsync(host_or_dev, tc, op->ndofs * sizeof(T), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

// ---- field monitor: typed launches (the C entry points are fus_model_monitor* below) ----
template <typename T, int NH>
static int launch_monitor(fus_model* m, const double* c, const double* s)
{
  const int64_t n = m->op->L.n_internal;
  const int64_t nvec = n / (16 / (int64_t)sizeof(T));
  MonPhase<NH> ph{};
  for (int k = 0; k < NH; ++k)
    ph.c[k] = c[k], ph.s[k] = s[k];
  const unsigned grid = (unsigned)std::min<int64_t>((nvec + 255) / 256, (int64_t)m->ctx->num_cus * 8);
  T* ext = m->mon.d_mon.as<T>();
  double* acc = reinterpret_cast<double*>(ext + 2 * n);
  hipLaunchKernelGGL((k_monitor_accumulate<T, NH>), dim3(grid), dim3(256), 0, m->ctx->stream, nvec, n,
                     m->mon.n == 0 ? 1 : 0, static_cast<const T*>(m->mon.which == FUS_U ? m->u0 : m->v0), ext, acc, ph);
  return FUS_OK;
}

template <typename T>
static int launch_monitor_nh(fus_model* m, const double* c, const double* s)
{
  return with_kind<0, 1, 2, 3, 4, 5, 6, 7, 8>(m->mon.nharm, [&](auto NH) { return launch_monitor<T, decltype(NH)::value>(m, c, s); });
}

template <typename T>
static int monitor_get(fus_model* m, int quantity, int k, void* out, int space)
{
  fus_op* op = m->op;
  hipStream_t st = m->ctx->stream;
  const int64_t n = op->L.n_internal;
  const T* ext = m->mon.d_mon.as<const T>();
  const double* acc = reinterpret_cast<const double*>(ext + 2 * n);
  const T* src = nullptr;
  if (quantity == FUS_MON_MAX || quantity == FUS_MON_MIN)
    src = ext + (quantity == FUS_MON_MIN ? n : 0);   // already a T vector in internal numbering
  else
  {
    const int plane = quantity == FUS_MON_MEAN ? 0 : quantity == FUS_MON_RMS ? 1
                      : quantity == FUS_MON_COS ? 1 + k : 1 + m->mon.nharm + k;
    const double num = (quantity == FUS_MON_COS || quantity == FUS_MON_SIN) ? 2.0 : 1.0;
    T* fin = static_cast<T*>(op->d_tmp_x);
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)m->ctx->num_cus * 8);
    hipLaunchKernelGGL((k_monitor_finalise<T>), dim3(grid), dim3(256), 0, st, n, acc + (size_t)plane * n, num,
                       (double)m->mon.n, quantity == FUS_MON_RMS ? 1 : 0, fin);
    src = fin;
  }
  T* tc = static_cast<T*>(op->d_tmp_c);
  T* dst = space == FUS_HOST ? tc : static_cast<T*>(out);
  hipLaunchKernelGGL((k_from_internal<T, 0>), dim3(nblk(op->ndofs)), dim3(256), 0, st, op->ndofs, op->d_dof_perm, src, dst);
  if (space == FUS_HOST)
    HIPCHK(hipMemcpyAsync(out, tc, op->ndofs * sizeof(T), hipMemcpyDeviceToHost, st));
  if (src == op->d_tmp_x)   // the operator's scratch vector keeps zeros in its padding slots
    HIPCHK(hipMemsetAsync(op->d_tmp_x, 0, (size_t)n * sizeof(T), st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

// "The next step must not trust what the last one left", by what changed; each level includes those before it.
// CHANGED_ORDER: the pseudo boundary partials were left for a stage time of the old scheme.  CHANGED_STATE: they carry the
// old state, and the next step runs directly, not as a graph replay.  CHANGED_SOURCE: they carry the old source, and the
// per-entry weights in d_bsrc / d_bsrc2 hold no stage time any more.
enum { CHANGED_ORDER, CHANGED_STATE, CHANGED_SOURCE };
static void model_changed(fus_model* m, int what)
{
  m->bnd_valid = false;
  if (what >= CHANGED_STATE)
    m->gsteps = 0;
  if (what >= CHANGED_SOURCE)
    m->src.tn_int = m->src.tn_sh = NAN;
}

// ---- phased / apodised source (fusmi.h) ----
// (not a hot path: every copy on the model's stream, complete on return)
static int copy_sync(hipStream_t st, void* dst, const void* src, size_t nbytes, hipMemcpyKind kind)
{
  if (nbytes > 0)
    HIPCHK(hipMemcpyAsync(dst, src, nbytes, kind, st));
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

// A caller vector of ndofs T as a host pointer: v itself, or its copy in buf when it lives on the device (NULL stays NULL)
template <typename T>
static int caller_on_host(fus_model* m, const void* v, int space, std::vector<T>& buf, const T** out)
{
  *out = static_cast<const T*>(v);
  if (!v || space != FUS_DEVICE)
    return FUS_OK;
  buf.resize(m->op->ndofs);
  *out = buf.data();
  return copy_sync(m->ctx->stream, buf.data(), v, buf.size() * sizeof(T), hipMemcpyDeviceToHost);
}

// What the two per-entry setters (fn: the one that was called) start from, in boundary-entry order: the source weights
// base / base2 as the setup (or fus_model_set_source_weights) left them, and for the entries that carry one the caller's
// dof with the validated amplitude and delay (dof -1, amplitude and delay 0 at the others: pure absorbing entries).
// keep / keep2: device copies of base / base2 for ModelSource::Arrays when the model does not keep them yet.
template <typename T>
struct FUS_HIDDEN SourcePrep
{
  std::vector<int32_t> dof;
  std::vector<T> base, base2, amp, tau;
  DevBuf keep, keep2;
};

// Fills P and changes nothing of the model.
template <typename T>
static int source_prepare(fus_model* m, const char* fn, const void* amplitude, const void* delay, int space, SourcePrep<T>* P)
{
  fus_op* op = m->op;
  hipStream_t st = m->ctx->stream;
  const ModelEntries& B = m->bnd;
  const ModelSource::Arrays& D = m->src.d;
  const int64_t nb = B.nb;
  std::vector<int32_t> bidx(nb);
  P->base.resize(nb), P->base2.resize(B.d_bsrc2 ? nb : 0);
  FUSCHK(copy_sync(st, bidx.data(), B.d_bidx.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost));
  FUSCHK(copy_sync(st, P->base.data(), (D.base ? D.base : B.d_bsrc).p, (size_t)nb * sizeof(T), hipMemcpyDeviceToHost));
  FUSCHK(copy_sync(st, P->base2.data(), (D.base2 ? D.base2 : B.d_bsrc2).p, P->base2.size() * sizeof(T), hipMemcpyDeviceToHost));
  std::vector<T> hbuf[2];
  const T* h[2];
  FUSCHK(caller_on_host(m, amplitude, space, hbuf[0], &h[0]));
  FUSCHK(caller_on_host(m, delay, space, hbuf[1], &h[1]));
  // gather through dof_perm into boundary-entry order; only the entries with a source weight count
  std::vector<int32_t> caller(op->L.n_internal, -1);
  for (int64_t d = 0; d < op->ndofs; ++d)
    caller[op->L.dof_perm[d]] = (int32_t)d;
  P->dof.assign(nb, -1), P->amp.assign(nb, T(0)), P->tau.assign(nb, T(0));
  for (int64_t k = 0; k < nb; ++k)
  {
    if (P->base[k] == T(0) && (P->base2.empty() || P->base2[k] == T(0)))
      continue;
    const int32_t d = caller[bidx[k]];
    const T a = h[0] ? h[0][d] : T(1), td = h[1] ? h[1][d] : T(0);
    if (!std::isfinite((double)a) || a < T(0) || !std::isfinite((double)td) || td < T(0))
      return fail(FUS_ERR_ARG, std::string(fn) + ": negative or non-finite amplitude / delay at dof " + std::to_string(d)
                                   + " of the source");
    P->dof[k] = d, P->amp[k] = a, P->tau[k] = td;
  }
  if (!D.base)
  {
    FUSCHK(upload(P->keep, P->base, st, "source weights"));
    if (B.d_bsrc2)
      FUSCHK(upload(P->keep2, P->base2, st, "source weights"));
    HIPCHK(hipStreamSynchronize(st));
  }
  return FUS_OK;
}

// The per-entry arrays A go in force (moves: nothing can fail); the unmodified weights stay the ones the model keeps
// already, or become P's copies.  Whatever A leaves empty is freed: the sampled signals, if a call without them was made
template <typename T>
static void source_install(fus_model* m, ModelSource::Arrays& A, SourcePrep<T>& P)
{
  ModelSource::Arrays& D = m->src.d;
  if (!D.base)
    D.base = std::move(P.keep), D.base2 = std::move(P.keep2);
  A.base = std::move(D.base), A.base2 = std::move(D.base2);
  D = std::move(A);
}

template <typename T>
static int model_set_source(fus_model* m, const void* amplitude, const void* delay, double duration, int space)
{
  hipStream_t st = m->ctx->stream;
  ModelEntries& B = m->bnd;
  ModelSource& S = m->src;
  const size_t bytes = (size_t)B.nb * sizeof(T), bytes2 = B.d_bsrc2 ? bytes : 0;
  HIPCHK(hipStreamSynchronize(st));
  if (!amplitude && !delay && duration == 0.0)
  {
    // the default source: the facet weights go back where the kernels read them
    if (S.d.base)
    {
      FUSCHK(copy_sync(st, B.d_bsrc.p, S.d.base.p, bytes, hipMemcpyDeviceToDevice));
      FUSCHK(copy_sync(st, B.d_bsrc2.p, S.d.base2.p, bytes2, hipMemcpyDeviceToDevice));
      S.d = {};
    }
    S.mode = 0, S.dur = 0.0;
    model_changed(m, CHANGED_SOURCE);
    return FUS_OK;
  }
  if (!source_duration_ok(m->freq, duration))
    return fail(FUS_ERR_ARG, "fus_model_set_source: duration is 0 (continuous) or at least two ramp lengths, 8 / freq");
  SourcePrep<T> P;
  FUSCHK(source_prepare<T>(m, "fus_model_set_source", amplitude, delay, space, &P));
  const bool fold = !delay && duration == 0.0;   // amplitude only: folded into the weights once, the scalar path stays
  ModelSource::Arrays A;
  if (!fold)
  {
    FUSCHK(upload(A.amp, P.amp, st, "per-entry amplitudes (fus_model_set_source)"));
    FUSCHK(upload(A.tau, P.tau, st, "per-entry delays (fus_model_set_source)"));
    HIPCHK(hipStreamSynchronize(st));
  }
  // from here on the model changes
  source_install(m, A, P);
  if (fold)
  {
    std::vector<T> w(P.base.size()), w2(P.base2.size());
    for (size_t k = 0; k < w.size(); ++k)
      w[k] = P.base[k] * P.amp[k];
    for (size_t k = 0; k < w2.size(); ++k)
      w2[k] = P.base2[k] * P.amp[k];
    FUSCHK(copy_sync(st, B.d_bsrc.p, w.data(), bytes, hipMemcpyHostToDevice));
    FUSCHK(copy_sync(st, B.d_bsrc2.p, w2.data(), bytes2, hipMemcpyHostToDevice));
  }
  S.mode = fold ? 1 : 2, S.dur = fold ? 0.0 : duration;
  model_changed(m, CHANGED_SOURCE);
  return FUS_OK;
}

// ---- source weights at any dof (fus_model_set_source_weights, fusmi.h) ----
template <typename T>
static int model_set_source_weights(fus_model* m, const void* weights, int space)
{
  fus_op* op = m->op;
  HIPCHK(hipStreamSynchronize(m->ctx->stream));
  std::vector<T> vol, hbuf;
  const T* w;
  FUSCHK(caller_on_host(m, weights, space, hbuf, &w));
  if (w)
  {
    for (int64_t d = 0; d < op->ndofs; ++d)
      if (!std::isfinite((double)w[d]))
        return fail(FUS_ERR_ARG, "fus_model_set_source_weights: non-finite weight at dof " + std::to_string(d));
    vol.assign(op->L.n_internal, T(0));
    for (int64_t d = 0; d < op->ndofs; ++d)
      vol[op->L.dof_perm[d]] = w[d];
  }
  FUSCHK(model_build_entries<T>(m, w ? vol.data() : nullptr));
  // the new lists are in force: the default source function on them (the per-entry arrays were in the old lists' order)
  m->src.d = {};
  m->src.mode = 0, m->src.dur = 0.0;
  model_changed(m, CHANGED_SOURCE);
  return FUS_OK;
}

// ---- sampled drive signals (fus_model_set_source_signals, fusmi.h) ----
template <typename T>
static int model_set_source_signals(fus_model* m, int64_t nchan, int64_t nsamp, double t_first, double ds,
                                    const double* signals, const int32_t* channel, const void* amplitude,
                                    const void* delay, int space)
{
  hipStream_t st = m->ctx->stream;
  const int64_t nb = m->bnd.nb;
  HIPCHK(hipStreamSynchronize(st));
  for (int64_t i = 0; i < nchan * nsamp; ++i)
    if (!std::isfinite(signals[i]))
      return fail(FUS_ERR_ARG, "fus_model_set_source_signals: non-finite sample " + std::to_string(i % nsamp) + " of channel "
                                   + std::to_string(i / nsamp));
  SourcePrep<T> P;
  FUSCHK(source_prepare<T>(m, "fus_model_set_source_signals", amplitude, delay, space, &P));
  // the channels of the entries with a source weight, renumbered in order of first use along the entry list
  // (k_source_entries_signal: rows read contiguously)
  std::vector<int32_t> chan(nb, -1), renum(nchan, -1), used;
  for (int64_t k = 0; k < nb; ++k)
  {
    const int32_t d = P.dof[k];
    if (d < 0)
      continue;
    const int32_t c = channel ? channel[d] : 0;
    if (c < -1 || c >= nchan)
      return fail(FUS_ERR_ARG, "fus_model_set_source_signals: channel " + std::to_string(c) + " at dof " + std::to_string(d)
                                   + " is neither -1 nor in [0, nchan)");
    if (c < 0)
      continue;
    if (renum[c] < 0)
      renum[c] = (int32_t)used.size(), used.push_back(c);
    chan[k] = renum[c];
  }
  const int64_t ncu = std::max<int64_t>((int64_t)used.size(), 1);
  std::vector<double> table((size_t)ncu * nsamp, 0.0);
  for (size_t c = 0; c < used.size(); ++c)
    for (int64_t j = 0; j < nsamp; ++j)
      table[(size_t)j * ncu + c] = signals[(size_t)used[c] * nsamp + j];
  // the new arrays first: a failed allocation leaves the source as it was
  ModelSource::Arrays A;
  FUSCHK(upload(A.table, table, st, "sample table (fus_model_set_source_signals)"));
  FUSCHK(upload(A.chan, chan, st, "channel list (fus_model_set_source_signals)"));
  FUSCHK(upload(A.amp, P.amp, st, "per-entry amplitudes (fus_model_set_source_signals)"));
  FUSCHK(upload(A.tau, P.tau, st, "per-entry delays (fus_model_set_source_signals)"));
  HIPCHK(hipStreamSynchronize(st));
  // from here on the model changes
  source_install(m, A, P);
  m->src.sig = SourceSignal{t_first, ds, nsamp, ncu};
  m->src.mode = 3, m->src.dur = 0.0;
  model_changed(m, CHANGED_SOURCE);
  return FUS_OK;
}

// ---- receivers: point samples of the resident solution (reference: Function::eval at located cells,
// python/src/fenicsxfus/utils.py:10-47, cpp/mwe/parallel_eval_line/main.cpp:49-84) ----
template <typename T>
static int launch_sample(fus_model* m, int which, void* out)
{
  fus_op* op = m->op;
  const T* vec = static_cast<const T*>(which == FUS_U ? m->u0 : m->v0);
  const dim3 grid((unsigned)((m->rc.n + 3) / 4)), blockd(256);
  return with_kind<2, 3>(op->tdim, [&](auto TD) -> int
  {
    hipLaunchKernelGGL((k_sample<T, decltype(TD)::value>), grid, blockd, 0, m->ctx->stream, m->rc.n, op->N, m->rc.d_idx.as<int32_t>(),
                       m->rc.d_bas.as<const T>(), vec, static_cast<T*>(out));
    HIPCHK(hipGetLastError());
    return FUS_OK;
  });
}

// after a step that ended at time t: every rec_every-th step, one sample of the receivers into the record buffer
static int model_record_step(fus_model* m, double t)
{
  if (m->rc.rec_every <= 0)
    return FUS_OK;
  ++m->rc.rec_step;
  if (m->rc.rec_step % m->rc.rec_every != 0 || m->rc.rec_n >= m->rc.rec_cap)
    return FUS_OK;
  if (m->rc.n > 0)  // a rank that holds none of the receivers still counts the record and its time
    FUSCHK(FUS_BY_DTYPE(m->op->dtype, launch_sample, m, m->rc.rec_which,
                        m->rc.d_rec.as<char>() + (size_t)m->rc.rec_n * m->rc.n * m->op->ts));
  m->rc.rec_times.push_back(t);
  ++m->rc.rec_n;
  return FUS_OK;
}

// ---- field monitor: whole-field maps over a window of steps, accumulated on the device (fusmi.h) ----
static size_t monitor_bytes(const fus_model* m, int nharm)
{
  return (size_t)m->op->L.n_internal * (2 * m->op->ts + (size_t)(2 + 2 * nharm) * sizeof(double));
}

// after a step that ended at time t (s = steps since fus_model_monitor): a sample when s > skip,
// (s - skip) % every == 0 and the count allows; an ordinary launch on the model's stream, nothing when off.
// No hipSetDevice here: the callers have made the model's device current, and fus_group_rk4_steps launches it,
// like the stage calls of its loop, with the device that is current -- the members of a group share one device.
static int model_after_step(fus_model* m, double t)
{
  if (m->mon.every <= 0)
    return FUS_OK;
  const int64_t s = ++m->mon.step;
  if (s <= m->mon.skip || (s - m->mon.skip) % m->mon.every != 0 || (m->mon.count > 0 && m->mon.n >= m->mon.count))
    return FUS_OK;
  double c[8], sn[8];
  for (int k = 1; k <= m->mon.nharm; ++k)
  {
    const double arg = 2.0 * M_PI * k * m->mon.freq * t;
    c[k - 1] = std::cos(arg), sn[k - 1] = std::sin(arg);
  }
  {
    ProfScope ps(m->ctx, "monitor");
    FUSCHK(FUS_BY_DTYPE(m->op->dtype, launch_monitor_nh, m, c, sn));
  }
  HIPCHK(hipGetLastError());
  if (m->mon.n == 0)
    m->mon.t_first = t;
  m->mon.t_last = t;
  ++m->mon.n;
  return FUS_OK;
}

// ---- relaxation absorption (fus_model_set_relaxation, fusmi.h) ----
// One sub-step of length h on the resident (v0, z): an ordinary launch on the model's stream, nothing when relaxation is
// off.  The coefficients p, e, g of wave_kernels.hpp are formed here in double and rounded once to T.  v0 changes, so the
// boundary terms the last stage left for the next step's first stage (boundary_next) are stale afterwards.
template <typename T, int R>
static int launch_relax(fus_model* m, double h)
{
  const int64_t n = m->op->L.n_internal;
  const int64_t nvec = n / (16 / (int64_t)sizeof(T));
  RelaxCoef<T, R> c;
  for (int k = 0; k < R; ++k)
  {
    const double hw = h * m->rx.omega[k], d = 1.0 + 0.5 * hw;
    c.p[k] = (T)((1.0 - 0.5 * hw) / d), c.e[k] = (T)((0.5 * h) / d), c.g[k] = (T)(hw / d);
  }
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nvec + 255) / 256, (int64_t)m->ctx->num_cus * 8));
  hipLaunchKernelGGL((k_relax_substep<T, R>), dim3(grid), dim3(256), 0, m->ctx->stream, nvec, n, static_cast<T*>(m->v0),
                     m->rx.z.as<T>(), m->rx.A.as<const T>(), c);
  return FUS_OK;
}

template <typename T>
static int launch_relax_r(fus_model* m, double h)
{
  return with_kind<1, 2, 3, 4>(m->rx.nrelax, [&](auto R) { return launch_relax<T, decltype(R)::value>(m, h); });
}

static int relax_apply(fus_model* m, double h)
{
  if (m->rx.nrelax == 0)
    return FUS_OK;
  {
    ProfScope ps(m->ctx, "relax");
    FUSCHK(FUS_BY_DTYPE(m->op->dtype, launch_relax_r, m, h));
  }
  HIPCHK(hipGetLastError());
  m->bnd_valid = false;
  return FUS_OK;
}

// ---- absorbing layers (fus_model_set_sponge, fusmi.h) ----
// One sub-step of length h on the resident (u0, v0) and, with relaxation on, its memory variables: an ordinary launch on
// the model's stream over the listed tiles, nothing when the sponge is off.  v0 changes, so the boundary terms the last
// stage left for the next step's first stage are stale afterwards.  No exchange: the sharers of a DOF hold the same sigma.
template <typename T, int R>
static int launch_sponge(fus_model* m, double h)
{
  const unsigned grid = (unsigned)std::min<int64_t>(m->sp.ntiles, (int64_t)m->ctx->num_cus * 8);
  hipLaunchKernelGGL((k_sponge_substep<T, R>), dim3(grid), dim3(256), 0, m->ctx->stream, m->sp.ntiles,
                     m->sp.tiles.as<const int32_t>(), m->op->L.n_internal, h, m->sp.sigma.as<const T>(),
                     static_cast<T*>(m->u0), static_cast<T*>(m->v0), m->rx.z.as<T>());
  return FUS_OK;
}

template <typename T>
static int launch_sponge_r(fus_model* m, double h)
{
  return with_kind<0, 1, 2, 3, 4>(m->rx.nrelax, [&](auto R) { return launch_sponge<T, decltype(R)::value>(m, h); });
}

static int sponge_apply(fus_model* m, double h)
{
  if (m->sp.ntiles == 0)
    return FUS_OK;
  {
    ProfScope ps(m->ctx, "sponge");
    FUSCHK(FUS_BY_DTYPE(m->op->dtype, launch_sponge_r, m, h));
  }
  HIPCHK(hipGetLastError());
  m->bnd_valid = false;
  return FUS_OK;
}

// sigma (host, caller numbering, checked) into a new plane in internal numbering and its tile list, built beside those in
// force and replacing them at the end: an error leaves the model as it was.  An all-zero sigma switches the sponge off.
template <typename T>
static int model_set_sponge(fus_model* m, const void* sigma_)
{
  fus_op* op = m->op;
  hipStream_t st = m->ctx->stream;
  const int64_t n = op->L.n_internal;
  const T* s = static_cast<const T*>(sigma_);
  for (int64_t i = 0; i < op->ndofs; ++i)
    if (!(s[i] >= T(0)) || !std::isfinite((double)s[i]))
      return fail(FUS_ERR_ARG, "fus_model_set_sponge: negative or non-finite sigma at DOF " + std::to_string(i));
  HIPCHK(hipStreamSynchronize(st));
  const char* what = "sponge plane and tile list (fus_model_set_sponge)";
  ModelSponge S;
  FUSCHK(S.sigma.alloc((size_t)n * sizeof(T), what));
  HIPCHK(hipMemsetAsync(S.sigma.p, 0, S.sigma.bytes, st));
  FUSCHK(model_getset<T>(m, S.sigma.p, const_cast<void*>(sigma_), FUS_HOST, true));
  std::vector<T> si((size_t)n);
  FUSCHK(copy_sync(st, si.data(), S.sigma.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
  const int64_t tile = 256 * (16 / (int64_t)sizeof(T));
  S.ntiles_total = (n + tile - 1) / tile;
  std::vector<int32_t> tiles;
  for (int64_t t = 0; t < S.ntiles_total; ++t)
  {
    int64_t cnt = 0;
    for (int64_t i = t * tile; i < std::min(n, (t + 1) * tile); ++i)
      cnt += si[i] != T(0);
    if (cnt > 0)
      tiles.push_back((int32_t)t);
    S.ndofs_active += cnt;
  }
  S.ntiles = (int64_t)tiles.size();
  const bool was_on = m->sp.ntiles > 0;
  if (S.ntiles == 0)
    S = ModelSponge{};
  else
  {
    FUSCHK(upload(S.tiles, tiles, st, what));
    HIPCHK(hipStreamSynchronize(st));
  }
  m->sp = std::move(S);
  if (was_on || m->sp.ntiles > 0)
    model_changed(m, CHANGED_STATE);
  return FUS_OK;
}

// a member of an in-process group whose strengths still wait for the sharers' parts must not step
static int relax_ready(const fus_model* m)
{
  return m->rx.pending ? fail(FUS_ERR_STATE, "relaxation strengths are not summed over the sharers: call "
                                             "fus_group_relaxation_finish on the group first")
                       : FUS_OK;
}

// A_nu = num_nu / den on the planes of R (in place), once both are complete
template <typename T>
static int relax_divide(fus_model* m, ModelRelax& R)
{
  const int64_t n = m->op->L.n_internal;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)m->ctx->num_cus * 8));
  hipLaunchKernelGGL((k_relax_strength<T>), dim3(grid), dim3(256), 0, m->ctx->stream, n, R.nrelax, R.A.as<T>(),
                     R.den.as<const T>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(m->ctx->stream));
  R.den.reset();
  R.pending = false;
  return FUS_OK;
}

// The planes are built beside those in force and replace them at the end: an error leaves the model as it was.
template <typename T>
static int model_set_relaxation(fus_model* m, int nrelax, const double* omega, const void* strength_)
{
  fus_op* op = m->op;
  hipStream_t st = m->ctx->stream;
  const int64_t n = op->L.n_internal, nc = op->ncells;
  const T* a = static_cast<const T*>(strength_);
  for (int64_t i = 0; i < (int64_t)nrelax * nc; ++i)
    if (!(a[i] >= T(0)) || !std::isfinite((double)a[i]))
      return fail(FUS_ERR_ARG, "fus_model_set_relaxation: negative or non-finite strength of process " + std::to_string(i / nc)
                                   + " in cell " + std::to_string(i % nc));
  HIPCHK(hipStreamSynchronize(st));
  const char* what = "relaxation planes (fus_model_set_relaxation)";
  ModelRelax R;
  R.nrelax = nrelax;
  for (int k = 0; k < nrelax; ++k)
    R.omega[k] = omega[k];
  FUSCHK(R.z.alloc((size_t)nrelax * n * sizeof(T), what));
  FUSCHK(R.A.alloc((size_t)nrelax * n * sizeof(T), what));
  FUSCHK(R.den.alloc((size_t)n * sizeof(T), what));
  DevBuf ones, coef;
  FUSCHK(ones.alloc((size_t)n * sizeof(T), what));
  FUSCHK(coef.alloc((size_t)nc * sizeof(T), what));
  HIPCHK(hipMemsetAsync(R.z.p, 0, R.z.bytes, st));
  HIPCHK(hipMemsetAsync(R.A.p, 0, R.A.bytes, st));
  HIPCHK(hipMemsetAsync(R.den.p, 0, R.den.bytes, st));
  hipLaunchKernelGGL((k_fill<T>), dim3(1024), dim3(256), 0, st, n, ones.as<T>(), T(1));
  // the lumped vectors, this rank's cells: den = M(1/(rho c^2)) 1, num_nu = M(a_nu/(rho c^2)) 1 (into A_nu)
  std::vector<T> mc(nc), cf(nc);
  HIPCHK(hipMemcpyAsync(mc.data(), m->mcoef, (size_t)nc * sizeof(T), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  FUSCHK(d_apply_internal(op, OP_MASS, m->mcoef, ones.p, R.den.p));
  for (int k = 0; k < nrelax; ++k)
  {
    for (int64_t e = 0; e < nc; ++e)
      cf[e] = a[(int64_t)k * nc + op->L.cell_perm[e]] * mc[e];
    HIPCHK(hipMemcpyAsync(coef.p, cf.data(), (size_t)nc * sizeof(T), hipMemcpyHostToDevice, st));
    FUSCHK(d_apply_internal(op, OP_MASS, coef.p, ones.p, R.A.as<T>() + (int64_t)k * n));
    HIPCHK(hipStreamSynchronize(st));   // cf is rewritten
  }
  // the sharers' parts: over RCCL here (collective), in a group by fus_group_relaxation_finish
  const bool multi = !op->neigh.empty();
  if (multi && !m->ctx->local_group)
  {
    FUSCHK(d_halo_sum(op, R.den.p));
    for (int k = 0; k < nrelax; ++k)
      FUSCHK(d_halo_sum(op, R.A.as<T>() + (int64_t)k * n));
  }
  if (multi && m->ctx->local_group)
    R.pending = true;
  else
    FUSCHK(relax_divide<T>(m, R));
  HIPCHK(hipStreamSynchronize(st));
  m->rx = std::move(R);
  model_changed(m, CHANGED_STATE);   // the mass actions went through the partial slab
  return FUS_OK;
}

// The stages of one step of the members' RK order from time t (Linear.hpp:273-295; ops[i] = ms[i]->op): per stage the first
// halves of all members (they end with the pack), the exchange, the second halves.  A single object -- one rank, or several
// over RCCL -- exchanges on the comm stream (nothing without neighbours), the members of an in-process group through
// device copies: the rule of thermal_run.
template <typename T>
static int wave_stages(fus_model** ms, fus_op** ops, int n, double t, double dt)
{
  const bool rccl = n == 1 && !ms[0]->ctx->local_group;
  for (int st = 0; st < ms[0]->rk_order; ++st)
  {
    for (int i = 0; i < n; ++i)
      FUSCHK(stage_begin<T>(ms[i], st, t, dt));
    if (!rccl)
      FUSCHK(halo_exchange_local(ops, n));
    else if (!ops[0]->neigh.empty())
    {
      ProfScope ps(ms[0]->ctx, "halo");
      FUSCHK(halo_exchange_rccl(ops[0]));
    }
    for (int i = 0; i < n; ++i)
      FUSCHK(stage_end<T>(ms[i], st, t, dt));
  }
  return FUS_OK;
}

// wave_stages, as a graph replay where option "graph" asks for it (a single model on one rank, no per-kernel events): the
// stages' launches are captured into a graph and replayed as ONE submission -- for launch-bound sizes (BASELINE config 1:
// eight kernels of a few microseconds).  The stage scalars (source value at the stage times) are kernel arguments, so
// every step is re-captured and the executable graph updated in place (hipGraphExecUpdate: same topology, new
// arguments); the first step after init / set runs directly (it has one more launch, k_boundary_partial, and sets the
// kernels' attributes).  What ends the step (wave_step_end) stays outside the capture.
static int d_model_step(fus_model** ms, fus_op** ops, int n, double t, double dt)
{
  fus_model* m = ms[0];
  fus_ctx* c = m->ctx;
  const bool graphed = n == 1 && c->graph && c->nranks <= 1 && !c->prof && m->op->neigh.empty() && m->gsteps > 0;
  ++m->gsteps;
  if (!graphed)
    return FUS_BY_DTYPE(m->op->dtype, wave_stages, ms, ops, n, t, dt);
  HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  const int r = FUS_BY_DTYPE(m->op->dtype, wave_stages, ms, ops, n, t, dt);
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(c->stream, &g);
  if (r != FUS_OK || e != hipSuccess || !g)
  {
    if (g)
      (void)hipGraphDestroy(g);
    return r != FUS_OK ? r : fail(FUS_ERR_HIP, std::string("graph capture of the RK step failed: ") + hipGetErrorString(e));
  }
  if (m->gexec)
  {
    hipGraphNode_t bad = nullptr;
    hipGraphExecUpdateResult res;
    if (hipGraphExecUpdate(m->gexec, g, &bad, &res) != hipSuccess)
    {
      (void)hipGetLastError();
      (void)hipGraphExecDestroy(m->gexec);
      m->gexec = nullptr;
    }
  }
  if (!m->gexec)
  {
    const hipError_t ei = hipGraphInstantiate(&m->gexec, g, nullptr, nullptr, 0);
    if (ei != hipSuccess)
    {
      (void)hipGraphDestroy(g);
      m->gexec = nullptr;
      return fail(FUS_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
    }
  }
  const hipError_t el = hipGraphLaunch(m->gexec, c->stream);
  (void)hipGraphDestroy(g);
  if (el != hipSuccess)
    return fail(FUS_ERR_HIP, std::string("hipGraphLaunch: ") + hipGetErrorString(el));
  return FUS_OK;
}

// What ends a step of length dt whose last stage has run, t_next the new time: at the orders 1-3 the accumulated solution
// becomes the next step's start state (RK4's last stage writes u0, v0 itself); the trailing relaxation half-step on that
// state and then the trailing sponge half-step (the mirror image of wave_step's order: the composition stays symmetric);
// then the receiver record and the monitor sample, which see the synchronised state
static int wave_step_end(fus_model** ms, int n, double dt, double t_next)
{
  for (int i = 0; i < n; ++i)
  {
    fus_model* m = ms[i];
    if (m->rk_order != 4)
      std::swap(m->u_, m->u0), std::swap(m->v_, m->v0);
    FUSCHK(relax_apply(m, 0.5 * dt));
    FUSCHK(sponge_apply(m, 0.5 * dt));
    FUSCHK(model_record_step(m, t_next));
    FUSCHK(model_after_step(m, t_next));
  }
  return FUS_OK;
}

// One step of n models from time t, state in (u0, v0) on entry and exit; the callers keep the clock and pass the new time.
// With relaxation (Strang splitting): a half-step of it, the RK step as it is, the second half-step in wave_step_end --
// two launches per step, both outside the graph capture of d_model_step, so a run split into several calls gives the
// bits of one call.  With absorbing layers the sponge half-steps go outside the relaxation ones in the same manner.
static int wave_step(fus_model** ms, fus_op** ops, int n, double t, double dt, double t_next)
{
  for (int i = 0; i < n; ++i)
  {
    FUSCHK(sponge_apply(ms[i], 0.5 * dt));
    FUSCHK(relax_apply(ms[i], 0.5 * dt));
  }
  FUSCHK(d_model_step(ms, ops, n, t, dt));
  return wave_step_end(ms, n, dt, t_next);
}

static int d_stage_end(fus_model* m, int i, double t, double dt) { return FUS_BY_DTYPE(m->op->dtype, stage_end, m, i, t, dt); }
static int d_setup_finish(fus_model* m) { return FUS_BY_DTYPE(m->op->dtype, model_setup_finish, m); }

static int group_halo(fus_model** ms, int n, int which_setup_vec)
{
  std::vector<fus_op*> ops(n);
  for (int i = 0; i < n; ++i)
  {
    ops[i] = ms[i]->op;
    void* v = which_setup_vec >= 0 ? setup_halo_vector(ms[i], which_setup_vec) : ms[i]->b;
    FUSCHK(d_halo_pack(ops[i], v));
  }
  FUSCHK(halo_exchange_local(ops.data(), n));
  if (which_setup_vec >= 0)
    for (int i = 0; i < n; ++i)
      FUSCHK(d_halo_unpack(ops[i], setup_halo_vector(ms[i], which_setup_vec)));
  return FUS_OK;
}

static int external_model(fus_model* m)
{
  if (!m)
    return fail(FUS_ERR_ARG, "null model");
  if (!m->ctx->external_transport)
    return fail(FUS_ERR_STATE, "set option external_transport before fus_comm_init to drive the halves yourself");
  HIPCHK(hipSetDevice(m->ctx->device));
  return FUS_OK;
}

// fus_model_rk4's loop: steps of dt from t0 until tf is reached, the last one shortened, with the clock kept in the
// model's scalar type T like the reference's (stage_end predicts the next step's first stage time the same way)
template <typename T>
static int model_rk(fus_model* m, double t0, double tf_, double dt_, int64_t* step)
{
  T t = (T)t0, tf = (T)tf_, dt = (T)dt_;
  while (t < tf)
  {
    dt = std::min(dt, tf - t);
    const T t_next = t + dt;
    FUSCHK(wave_step(&m, &m->op, 1, t, dt, t_next));
    t = t_next;
    ++*step;
  }
  return FUS_OK;
}

extern "C"
{

int fus_facet_diag(fus_op* op, int64_t nfacets, const int32_t* fc, const int32_t* fl,
                   const void* cellcoef, void* out)
{
  if (!op || !out || (nfacets > 0 && (!fc || !fl || !cellcoef)))
    return fail(FUS_ERR_ARG, "null argument");
  for (int64_t f = 0; f < nfacets; ++f)
    if (fc[f] < 0 || fc[f] >= op->ncells || fl[f] < 0 || fl[f] > 5)
      return fail(FUS_ERR_ARG, "facet (cell, local facet) out of range");
  if (op->dtype == FUS_F64)
    facet_diag_host<double>(op, nfacets, fc, fl, static_cast<const double*>(cellcoef),
                            static_cast<double*>(out));
  else
    facet_diag_host<float>(op, nfacets, fc, fl, static_cast<const float*>(cellcoef),
                           static_cast<float*>(out));
  return FUS_OK;
}

int fus_model_create(fus_ctx* c, int kind, fus_op* op, const void* c0, const void* rho0,
                     const void* delta0, const void* beta0, int64_t nfacets,
                     const int32_t* facet_cells, const int32_t* facet_local,
                     const int32_t* facet_tags, double freq, double amp, double speed,
                     fus_model** out)
{
  if (!c || !op || !c0 || !rho0 || !out)
    return fail(FUS_ERR_ARG, "null argument");
  if (kind != FUS_LINEAR && kind != FUS_LOSSY && kind != FUS_WESTERVELT)
    return fail(FUS_ERR_ARG, "unknown model kind");
  if (kind == FUS_LINEAR && (delta0 || beta0))
    return fail(FUS_ERR_ARG, "delta0/beta0 must be NULL for FUS_LINEAR");
  if (kind == FUS_LOSSY && (!delta0 || beta0))
    return fail(FUS_ERR_ARG, "FUS_LOSSY needs delta0 (and no beta0)");
  if (kind == FUS_WESTERVELT && (!delta0 || !beta0))
    return fail(FUS_ERR_ARG, "FUS_WESTERVELT needs delta0 and beta0");
  if (kind != FUS_LINEAR && op->nfields < 2)
    return fail(FUS_ERR_STATE, "FUS_LOSSY / FUS_WESTERVELT need operator data created with option fields=2");
  if (nfacets > 0 && (!facet_cells || !facet_local || !facet_tags))
    return fail(FUS_ERR_ARG, "null facet arrays");
  if (!(freq > 0) || !(speed > 0))
    return fail(FUS_ERR_ARG, "freq and speed must be positive");
  HIPCHK(hipSetDevice(c->device));
  std::unique_ptr<fus_model> m(new fus_model());
  m->ctx = c, m->op = op, m->kind = kind, m->freq = freq, m->amp = amp, m->speed = speed;
  m->forms = c->forms;
  m->lean_rk4 = c->lean_rk4;
  int r = FUS_BY_DTYPE(op->dtype, model_setup, m.get(), c0, rho0, delta0, beta0, nfacets, facet_cells, facet_local, facet_tags);
  if (r == FUS_OK && !c->local_group)
  {
    // add the sharers' parts of the lumped mass over RCCL, then finish; with the in-process
    // transport this happens in fus_group_finish_setup once every member exists.  The boundary
    // weights of interface dofs stay per-rank: each rank adds the term of its own facets to its
    // partial b and the exchange sums them (v_n is identical on all sharers).
    r = d_halo_sum(op, setup_halo_vector(m.get(), 0));
    if (r == FUS_OK && m->mn1)
      r = d_halo_sum(op, setup_halo_vector(m.get(), 1));
    if (r == FUS_OK)
      r = d_setup_finish(m.get());
  }
  if (r != FUS_OK)
    return r;   // (m frees what the setup had allocated)
  *out = m.release();
  return FUS_OK;
}

int fus_group_finish_setup(fus_model** ms, int n)
{
  if (!ms || n < 1)
    return fail(FUS_ERR_ARG, "bad group");
  FUSCHK(group_halo(ms, n, 0));  // lumped mass (see fus_model_create)
  if (ms[0]->mn1)
    FUSCHK(group_halo(ms, n, 1));  // Westervelt: diagonal of M(nlin1)
  for (int i = 0; i < n; ++i)
    FUSCHK(d_setup_finish(ms[i]));
  return FUS_OK;
}

int fus_group_rk4_steps(fus_model** ms, int n, double t0, double dt, int64_t nsteps)
{
  if (!ms || n < 1)
    return fail(FUS_ERR_ARG, "bad group");
  for (int i = 0; i < n; ++i)
    if (!ms[i] || !ms[i]->setup_done || !ms[i]->initialised)
      return fail(FUS_ERR_STATE, "group member not set up / initialised");
  // one stage loop steps every member: they must be the same scheme on the same model and scalar type
  for (int i = 1; i < n; ++i)
    if (ms[i]->rk_order != ms[0]->rk_order || ms[i]->kind != ms[0]->kind || ms[i]->op->dtype != ms[0]->op->dtype)
      return fail(FUS_ERR_ARG, "group members differ in rk_order, model kind or scalar type");
  for (int i = 0; i < n; ++i)
    FUSCHK(relax_ready(ms[i]));
  std::vector<fus_op*> ops(n);
  for (int i = 0; i < n; ++i)
    ops[i] = ms[i]->op;
  double t = t0;
  for (int64_t s = 0; s < nsteps; ++s)
  {
    FUSCHK(wave_step(ms, ops.data(), n, t, dt, t + dt));
    t += dt;
  }
  for (int i = 0; i < n; ++i)
    HIPCHK(hipStreamSynchronize(ms[i]->ctx->stream));
  return FUS_OK;
}

int fus_model_setup_count(fus_model* m) { return m ? (m->mn1 ? 2 : 1) : 0; }

int fus_model_setup_pack(fus_model* m, int k)
{
  FUSCHK(external_model(m));
  if (k < 0 || k >= fus_model_setup_count(m))
    return fail(FUS_ERR_ARG, "setup vector index out of range");
  FUSCHK(d_halo_pack(m->op, setup_halo_vector(m, k)));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));   // the send buffer is complete on return
  return FUS_OK;
}

int fus_model_setup_unpack(fus_model* m, int k)
{
  FUSCHK(external_model(m));
  if (k < 0 || k >= fus_model_setup_count(m))
    return fail(FUS_ERR_ARG, "setup vector index out of range");
  return d_halo_unpack(m->op, setup_halo_vector(m, k));
}

int fus_model_setup_finish(fus_model* m)
{
  FUSCHK(external_model(m));
  return d_setup_finish(m);
}

int fus_model_stage_begin(fus_model* m, int stage, double t, double dt)
{
  FUSCHK(external_model(m));
  if (!m->initialised || !m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_setup_finish and fus_model_init come first");
  if (stage < 0 || stage >= m->rk_order)
    return fail(FUS_ERR_ARG, "stage out of range");
  FUSCHK(relax_ready(m));
  if (stage == 0)   // the leading half-steps (wave_step)
  {
    FUSCHK(sponge_apply(m, 0.5 * dt));
    FUSCHK(relax_apply(m, 0.5 * dt));
  }
  FUSCHK(FUS_BY_DTYPE(m->op->dtype, stage_begin, m, stage, t, dt));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));   // the send buffer is complete on return
  return FUS_OK;
}

int fus_model_stage_end(fus_model* m, int stage, double t, double dt)
{
  FUSCHK(external_model(m));
  if (stage < 0 || stage >= m->rk_order)
    return fail(FUS_ERR_ARG, "stage out of range");
  FUSCHK(d_stage_end(m, stage, t, dt));
  return stage == m->rk_order - 1 ? wave_step_end(&m, 1, dt, t + dt) : FUS_OK;
}

int fus_model_set_rk_order(fus_model* m, int order)
{
  if (!m || order < 1 || order > 4)
    return fail(FUS_ERR_ARG, "rk order must be 1, 2, 3 or 4");
  m->rk_order = order;
  model_changed(m, CHANGED_ORDER);
  return FUS_OK;
}

int fus_model_destroy(fus_model* m)
{
  if (!m)
    return FUS_OK;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  if (m->gexec)
    (void)hipGraphExecDestroy(m->gexec);
  if (m->op && m->op->bnd_owner == m)
    m->op->bnd_owner = nullptr;
  delete m;   // frees its arrays: nothing on the stream reads them any more
  return FUS_OK;
}

int fus_model_init(fus_model* m)
{
  if (!m)
    return fail(FUS_ERR_ARG, "null model");
  HIPCHK(hipSetDevice(m->ctx->device));
  const size_t bytes = (size_t)m->op->L.n_internal * m->op->ts;
  for (void* v : {m->u0, m->v0, m->u_, m->v_, m->un, m->vn, m->b})
    HIPCHK(hipMemsetAsync(v, 0, bytes, m->ctx->stream));
  if (m->rx.z)   // the memory variables start from rest with the fields (fus_model_set leaves them alone)
    HIPCHK(hipMemsetAsync(m->rx.z.p, 0, m->rx.z.bytes, m->ctx->stream));
  m->initialised = true;
  model_changed(m, CHANGED_STATE);
  return FUS_OK;
}

int fus_model_set_receivers(fus_model* m, int64_t npts, const int32_t* cells, const double* refcoords)
{
  if (!m || npts < 0 || (npts > 0 && (!cells || !refcoords)))
    return fail(FUS_ERR_ARG, "bad argument");
  fus_op* op = m->op;
  HIPCHK(hipSetDevice(m->ctx->device));
  const int N = op->N, Nd = op->Nd, td = op->tdim;
  for (int64_t r = 0; r < npts; ++r)
    if (cells[r] < 0 || cells[r] >= op->ncells)
      return fail(FUS_ERR_ARG, "receiver cell index out of range (points outside the local mesh must be dropped by the caller)");
  // internal indices of each receiver's cell dofs; 1-D Lagrange basis on the operator's nodes at the reference coordinates
  std::vector<int32_t> idx((size_t)npts * Nd);
  std::vector<double> bas((size_t)npts * td * N);
  for (int64_t r = 0; r < npts; ++r)
  {
    const int32_t* dm = op->h_dofmap.data() + (size_t)cells[r] * Nd;
    for (int k = 0; k < Nd; ++k)
      idx[(size_t)r * Nd + k] = op->L.dof_perm[dm[k]];
    for (int d = 0; d < td; ++d)
    {
      const double X = refcoords[r * td + d];
      for (int i = 0; i < N; ++i)
      {
        double l = 1.0;
        for (int j = 0; j < N; ++j)
          if (j != i)
            l *= (X - op->nodes[j]) / (op->nodes[i] - op->nodes[j]);
        bas[((size_t)r * td + d) * N + i] = l;
      }
    }
  }
  hipStream_t st = m->ctx->stream;
  HIPCHK(hipStreamSynchronize(st));
  // the new receivers beside those in force; they replace them, and drop the records taken at the old points, at the end
  ModelReceivers R;
  const char* what = "receiver arrays (fus_model_set_receivers)";
  R.n = npts;
  FUSCHK(upload(R.d_idx, idx, st, what));
  if (op->dtype == FUS_F64)
    FUSCHK(upload(R.d_bas, bas, st, what));
  else
  {
    const std::vector<float> bf(bas.begin(), bas.end());
    FUSCHK(upload(R.d_bas, bf, st, what));
    HIPCHK(hipStreamSynchronize(st));  // bf leaves scope
  }
  FUSCHK(R.d_out.alloc((size_t)npts * op->ts, what));
  HIPCHK(hipMemsetAsync(R.d_out.p, 0, std::max<size_t>(R.d_out.bytes, 16), st));
  HIPCHK(hipStreamSynchronize(st));   // the host vectors leave scope
  m->rc = std::move(R);
  return FUS_OK;
}

int fus_model_sample(fus_model* m, int which, void* out, int space)
{
  if (!m || !out || (which != FUS_U && which != FUS_V))
    return fail(FUS_ERR_ARG, "bad argument");
  if (m->rc.n == 0)
    return m->rc.d_idx ? FUS_OK : fail(FUS_ERR_STATE, "fus_model_set_receivers has not been called");
  HIPCHK(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  FUSCHK(FUS_BY_DTYPE(m->op->dtype, launch_sample, m, which, space == FUS_HOST ? m->rc.d_out.p : out));
  if (space == FUS_HOST)
    HIPCHK(hipMemcpyAsync(out, m->rc.d_out.p, (size_t)m->rc.n * m->op->ts, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

int fus_model_record(fus_model* m, int which, int every, int64_t capacity)
{
  if (!m || (which != FUS_U && which != FUS_V) || every < 0 || capacity < 0)
    return fail(FUS_ERR_ARG, "bad argument");
  if (every > 0 && !m->rc.d_idx)
    return fail(FUS_ERR_STATE, "fus_model_set_receivers has not been called");
  HIPCHK(hipSetDevice(m->ctx->device));
  m->rc.rec_every = every, m->rc.rec_which = which, m->rc.rec_n = 0, m->rc.rec_step = 0, m->rc.rec_times.clear();
  if (every > 0)
  {
    const size_t need = (size_t)capacity * std::max<int64_t>(m->rc.n, 1) * m->op->ts;
    if (need > m->rc.d_rec.bytes)   // it only grows: the records of the recording before go with the old buffer
    {
      HIPCHK(hipStreamSynchronize(m->ctx->stream));
      FUSCHK(m->rc.d_rec.alloc(need, "record buffer (fus_model_record)"));
    }
    m->rc.rec_cap = capacity;  // the limit of this recording, whatever an earlier one allocated
  }
  return FUS_OK;
}

int fus_model_get_records(fus_model* m, void* out, double* times, int64_t* nrec)
{
  if (!m || !nrec)
    return fail(FUS_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->ctx->device));
  const int64_t n = m->rc.rec_n;
  if (out && n > 0 && m->rc.n > 0)
  {
    HIPCHK(hipMemcpyAsync(out, m->rc.d_rec.p, (size_t)n * m->rc.n * m->op->ts, hipMemcpyDeviceToHost, m->ctx->stream));
    HIPCHK(hipStreamSynchronize(m->ctx->stream));
  }
  if (times)
    for (int64_t k = 0; k < n; ++k)
      times[k] = m->rc.rec_times[k];
  *nrec = n;
  return FUS_OK;
}

int fus_model_monitor(fus_model* m, int which, int nharm, double freq, int64_t skip, int every, int64_t count)
{
  if (!m)
    return fail(FUS_ERR_ARG, "null model");
  HIPCHK(hipSetDevice(m->ctx->device));
  if (every == 0)
  {
    HIPCHK(hipStreamSynchronize(m->ctx->stream));
    m->mon.d_mon.reset();
    m->mon.every = 0, m->mon.n = 0, m->mon.step = 0;
    return FUS_OK;
  }
  if ((which != FUS_U && which != FUS_V) || nharm < 0 || nharm > 8 || every < 0 || skip < 0 || count < 0
      || !(freq >= 0.0) || !std::isfinite(freq))
    return fail(FUS_ERR_ARG, "fus_model_monitor: which is FUS_U | FUS_V, nharm 0..8, freq >= 0, skip >= 0, every > 0 (0: off), count >= 0");
  const size_t bytes = monitor_bytes(m, nharm);
  if (bytes != m->mon.d_mon.bytes)
  {
    HIPCHK(hipStreamSynchronize(m->ctx->stream));
    m->mon.every = 0;   // off, should the allocation fail
    FUSCHK(m->mon.d_mon.alloc(bytes, "monitor accumulators (fus_model_monitor)"));
  }
  HIPCHK(hipMemsetAsync(m->mon.d_mon.p, 0, bytes, m->ctx->stream));
  m->mon.which = which, m->mon.nharm = nharm, m->mon.freq = freq == 0.0 ? m->freq : freq;
  m->mon.skip = skip, m->mon.every = every, m->mon.count = count;
  m->mon.step = 0, m->mon.n = 0, m->mon.t_first = m->mon.t_last = 0.0;
  return FUS_OK;
}

int fus_model_monitor_info(fus_model* m, int64_t* nsamples, double* t_first, double* t_last)
{
  if (!m)
    return fail(FUS_ERR_ARG, "null model");
  if (m->mon.every <= 0)
    return fail(FUS_ERR_STATE, "the monitor is off (fus_model_monitor)");
  if (nsamples)
    *nsamples = m->mon.n;
  if (t_first)
    *t_first = m->mon.t_first;
  if (t_last)
    *t_last = m->mon.t_last;
  return FUS_OK;
}

int fus_model_monitor_get(fus_model* m, int quantity, int k, void* out, int space)
{
  if (!m || !out || quantity < FUS_MON_MAX || quantity > FUS_MON_SIN || (space != FUS_HOST && space != FUS_DEVICE))
    return fail(FUS_ERR_ARG, "fus_model_monitor_get: bad model, quantity, out or space");
  if (m->mon.every <= 0)
    return fail(FUS_ERR_STATE, "the monitor is off (fus_model_monitor)");
  if ((quantity == FUS_MON_COS || quantity == FUS_MON_SIN) && (k < 1 || k > m->mon.nharm))
    return fail(FUS_ERR_ARG, "fus_model_monitor_get: harmonic k outside 1..nharm");
  if (m->mon.n == 0)
    return fail(FUS_ERR_STATE, "the monitor has taken no sample yet");
  HIPCHK(hipSetDevice(m->ctx->device));
  return FUS_BY_DTYPE(m->op->dtype, monitor_get, m, quantity, k, out, space);
}

int fus_model_rk4(fus_model* m, double t0, double tf_, double dt_, int64_t* nsteps)
{
  if (!m)
    return fail(FUS_ERR_ARG, "null model");
  if (!m->initialised || !m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_init (or fus_model_set) must be called before rk4");
  if (!(dt_ > 0))
    return fail(FUS_ERR_ARG, "dt must be positive");
  if (m->ctx->local_group)
    return fail(FUS_ERR_STATE, "in-process transport: use fus_group_rk4_steps");
  FUSCHK(relax_ready(m));
  HIPCHK(hipSetDevice(m->ctx->device));
  int64_t step = 0;
  FUSCHK(FUS_BY_DTYPE(m->op->dtype, model_rk, m, t0, tf_, dt_, &step));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));
  if (nsteps)
    *nsteps = step;
  return FUS_OK;
}

int fus_model_rk4_steps(fus_model* m, double t0, double dt, int64_t nsteps)
{
  if (!m)
    return fail(FUS_ERR_ARG, "null model");
  if (!m->initialised || !m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_init (or fus_model_set) must be called before rk4");
  if (m->ctx->local_group)
    return fail(FUS_ERR_STATE, "in-process transport: use fus_group_rk4_steps");
  FUSCHK(relax_ready(m));
  HIPCHK(hipSetDevice(m->ctx->device));
  double t = t0;
  for (int64_t s = 0; s < nsteps; ++s)
  {
    FUSCHK(wave_step(&m, &m->op, 1, t, dt, t + dt));
    t += dt;
  }
  return FUS_OK;
}

int fus_model_get(fus_model* m, int which, void* out, int space)
{
  if (!m || !out || (which != FUS_U && which != FUS_V))
    return fail(FUS_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->ctx->device));
  return FUS_BY_DTYPE(m->op->dtype, model_getset, m, which == FUS_U ? m->u0 : m->v0, out, space, false);
}

int fus_model_set(fus_model* m, int which, const void* in, int space)
{
  if (!m || !in || (which != FUS_U && which != FUS_V))
    return fail(FUS_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(m->ctx->device));
  m->initialised = true;
  model_changed(m, CHANGED_STATE);
  return FUS_BY_DTYPE(m->op->dtype, model_getset, m, which == FUS_U ? m->u0 : m->v0, const_cast<void*>(in), space, true);
}

// ---- phased / apodised source (fusmi.h) ----
int fus_model_set_source(fus_model* m, const void* amplitude, const void* delay, double duration, int space)
{
  if (!m || (space != FUS_HOST && space != FUS_DEVICE) || !(duration >= 0.0))
    return fail(FUS_ERR_ARG, "fus_model_set_source: bad model, space or duration");
  if (!m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_set_source: the model's setup is not finished");
  HIPCHK(hipSetDevice(m->ctx->device));
  return FUS_BY_DTYPE(m->op->dtype, model_set_source, m, amplitude, delay, duration, space);
}

int fus_model_set_source_weights(fus_model* m, const void* weights, int space)
{
  if (!m || (space != FUS_HOST && space != FUS_DEVICE))
    return fail(FUS_ERR_ARG, "fus_model_set_source_weights: bad model or space");
  if (!m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_set_source_weights: the model's setup is not finished");
  HIPCHK(hipSetDevice(m->ctx->device));
  return FUS_BY_DTYPE(m->op->dtype, model_set_source_weights, m, weights, space);
}

int fus_model_set_source_signals(fus_model* m, int64_t nchan, int64_t nsamp, double t_first, double ds,
                                 const double* signals, const int32_t* channel, const void* amplitude,
                                 const void* delay, int space)
{
  if (!m || (space != FUS_HOST && space != FUS_DEVICE) || !signals || nchan < 1 || (!channel && nchan != 1))
    return fail(FUS_ERR_ARG, "fus_model_set_source_signals: bad model, space, signals or channel (NULL only with nchan == 1)");
  if (!source_signal_ok(nsamp, t_first, ds))
    return fail(FUS_ERR_ARG, "fus_model_set_source_signals: nsamp >= 2, ds > 0 and t_first finite are required");
  if (nchan > INT32_MAX || nsamp > INT64_MAX / (int64_t)sizeof(double) / nchan)
    return fail(FUS_ERR_ARG, "fus_model_set_source_signals: nchan * nsamp * 8 bytes exceed the address range");
  if (!m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_set_source_signals: the model's setup is not finished");
  HIPCHK(hipSetDevice(m->ctx->device));
  return FUS_BY_DTYPE(m->op->dtype, model_set_source_signals, m, nchan, nsamp, t_first, ds, signals, channel, amplitude,
                      delay, space);
}

// ---- relaxation absorption (fusmi.h) ----
int fus_model_set_relaxation(fus_model* m, int nrelax, const double* omega, const void* strength)
{
  if (!m)
    return fail(FUS_ERR_ARG, "null model");
  if (nrelax < 0 || nrelax > 4)
    return fail(FUS_ERR_ARG, "fus_model_set_relaxation: nrelax is 0 (off) to 4");
  if (nrelax > 0 && strength && !omega)
    return fail(FUS_ERR_ARG, "fus_model_set_relaxation: null omega");
  if (!m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_set_relaxation: the model's setup is not finished");
  HIPCHK(hipSetDevice(m->ctx->device));
  if (nrelax == 0 || !strength)
  {
    HIPCHK(hipStreamSynchronize(m->ctx->stream));
    const bool was_on = m->rx.nrelax > 0;
    m->rx = ModelRelax{};
    if (was_on)
      model_changed(m, CHANGED_STATE);
    return FUS_OK;
  }
  for (int k = 0; k < nrelax; ++k)
    if (!(omega[k] > 0.0) || !std::isfinite(omega[k]))
      return fail(FUS_ERR_ARG, "fus_model_set_relaxation: relaxation frequency " + std::to_string(k) + " is not positive and finite");
  if (!m->op->neigh.empty() && m->ctx->external_transport)
    return fail(FUS_ERR_STATE, "fus_model_set_relaxation: a model with neighbours under the external transport is not "
                               "supported (the strengths' sums over the sharers have no entry points there)");
  return FUS_BY_DTYPE(m->op->dtype, model_set_relaxation, m, nrelax, omega, strength);
}

static int relax_plane(fus_model* m, int nu, const void* p, int space, void** plane)
{
  if (!m || !p || (space != FUS_HOST && space != FUS_DEVICE))
    return fail(FUS_ERR_ARG, "fus_model_relaxation_get / _set: bad model, pointer or space");
  if (m->rx.nrelax == 0)
    return fail(FUS_ERR_STATE, "relaxation is off (fus_model_set_relaxation)");
  if (nu < 0 || nu >= m->rx.nrelax)
    return fail(FUS_ERR_ARG, "fus_model_relaxation_get / _set: process index outside 0..nrelax-1");
  HIPCHK(hipSetDevice(m->ctx->device));
  *plane = m->rx.z.as<char>() + (size_t)nu * m->op->L.n_internal * m->op->ts;
  return FUS_OK;
}

int fus_model_relaxation_get(fus_model* m, int nu, void* out, int space)
{
  void* plane;
  FUSCHK(relax_plane(m, nu, out, space, &plane));
  return FUS_BY_DTYPE(m->op->dtype, model_getset, m, plane, out, space, false);
}

int fus_model_relaxation_set(fus_model* m, int nu, const void* in, int space)
{
  void* plane;
  FUSCHK(relax_plane(m, nu, in, space, &plane));
  return FUS_BY_DTYPE(m->op->dtype, model_getset, m, plane, const_cast<void*>(in), space, true);
}

int fus_model_relaxation_strength(fus_model* m, int nu, void* out, int space)
{
  void* plane;
  FUSCHK(relax_plane(m, nu, out, space, &plane));
  FUSCHK(relax_ready(m));
  plane = m->rx.A.as<char>() + (static_cast<char*>(plane) - m->rx.z.as<char>());
  return FUS_BY_DTYPE(m->op->dtype, model_getset, m, plane, out, space, false);
}

int fus_model_relaxation_apply(fus_model* m, double h)
{
  if (!m || !(h >= 0.0) || !std::isfinite(h))
    return fail(FUS_ERR_ARG, "fus_model_relaxation_apply: bad model or sub-step length");
  if (!m->initialised || !m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_init (or fus_model_set) must be called before fus_model_relaxation_apply");
  FUSCHK(relax_ready(m));
  HIPCHK(hipSetDevice(m->ctx->device));
  FUSCHK(relax_apply(m, h));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));
  return FUS_OK;
}

int fus_group_relaxation_finish(fus_model** ms, int n)
{
  if (!ms || n < 1)
    return fail(FUS_ERR_ARG, "bad group");
  for (int i = 0; i < n; ++i)
    if (!ms[i] || ms[i]->rx.nrelax != ms[0]->rx.nrelax || ms[i]->op->dtype != ms[0]->op->dtype)
      return fail(FUS_ERR_ARG, "fus_group_relaxation_finish: group members differ in nrelax or scalar type");
  for (int i = 0; i < n; ++i)
    if (ms[i]->rx.nrelax > 0 && !ms[i]->rx.pending)
      return fail(FUS_ERR_STATE, "fus_group_relaxation_finish: a member's strengths are complete already");
  if (ms[0]->rx.nrelax == 0)
    return FUS_OK;
  // den and the nrelax numerators, summed over the sharers after the pattern of thermal_sum
  std::vector<fus_op*> ops(n);
  const size_t plane = (size_t)ms[0]->op->ts;
  for (int k = 0; k <= ms[0]->rx.nrelax; ++k)
  {
    auto vec = [&](fus_model* m) -> void*
    { return k == 0 ? m->rx.den.p : m->rx.A.as<char>() + (size_t)(k - 1) * m->op->L.n_internal * plane; };
    for (int i = 0; i < n; ++i)
    {
      ops[i] = ms[i]->op;
      FUSCHK(d_halo_pack(ops[i], vec(ms[i])));
    }
    FUSCHK(halo_exchange_local(ops.data(), n));
    for (int i = 0; i < n; ++i)
      FUSCHK(d_halo_unpack(ops[i], vec(ms[i])));
  }
  for (int i = 0; i < n; ++i)
    FUSCHK(FUS_BY_DTYPE(ms[i]->op->dtype, relax_divide, ms[i], ms[i]->rx));
  return FUS_OK;
}

// ---- absorbing layers (fusmi.h) ----
int fus_model_set_sponge(fus_model* m, const void* sigma, int space)
{
  if (!m || (sigma && space != FUS_HOST && space != FUS_DEVICE))
    return fail(FUS_ERR_ARG, "fus_model_set_sponge: bad model or space");
  if (!m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_set_sponge: the model's setup is not finished");
  HIPCHK(hipSetDevice(m->ctx->device));
  if (!sigma)
  {
    HIPCHK(hipStreamSynchronize(m->ctx->stream));
    const bool was_on = m->sp.ntiles > 0;
    m->sp = ModelSponge{};
    if (was_on)
      model_changed(m, CHANGED_STATE);
    return FUS_OK;
  }
  std::vector<char> host;   // a device vector is checked, and its tiles listed, on the host
  if (space == FUS_DEVICE)
  {
    host.resize((size_t)m->op->ndofs * m->op->ts);
    FUSCHK(copy_sync(m->ctx->stream, host.data(), sigma, host.size(), hipMemcpyDeviceToHost));
    sigma = host.data();
  }
  return FUS_BY_DTYPE(m->op->dtype, model_set_sponge, m, sigma);
}

int fus_model_sponge_get(fus_model* m, void* out, int space)
{
  if (!m || !out || (space != FUS_HOST && space != FUS_DEVICE))
    return fail(FUS_ERR_ARG, "fus_model_sponge_get: bad model, pointer or space");
  if (m->sp.ntiles == 0)
    return fail(FUS_ERR_STATE, "the sponge is off (fus_model_set_sponge)");
  HIPCHK(hipSetDevice(m->ctx->device));
  return FUS_BY_DTYPE(m->op->dtype, model_getset, m, m->sp.sigma.p, out, space, false);
}

int fus_model_sponge_apply(fus_model* m, double h)
{
  if (!m || !(h >= 0.0) || !std::isfinite(h))
    return fail(FUS_ERR_ARG, "fus_model_sponge_apply: bad model or sub-step length");
  if (m->sp.ntiles == 0)
    return fail(FUS_ERR_STATE, "the sponge is off (fus_model_set_sponge)");
  if (!m->initialised || !m->setup_done)
    return fail(FUS_ERR_STATE, "fus_model_init (or fus_model_set) must be called before fus_model_sponge_apply");
  HIPCHK(hipSetDevice(m->ctx->device));
  FUSCHK(sponge_apply(m, h));
  HIPCHK(hipStreamSynchronize(m->ctx->stream));
  return FUS_OK;
}

int fus_model_sponge_info(fus_model* m, int64_t* ndofs_active, int64_t* ntiles_active, int64_t* ntiles_total)
{
  if (!m)
    return fail(FUS_ERR_ARG, "null model");
  if (ndofs_active)
    *ndofs_active = m->sp.ndofs_active;
  if (ntiles_active)
    *ntiles_active = m->sp.ntiles;
  if (ntiles_total)   // also while the sponge is off: what listing every tile would take
  {
    const int64_t tile = 256 * (16 / (int64_t)m->op->ts);
    *ntiles_total = (m->op->L.n_internal + tile - 1) / tile;
  }
  return FUS_OK;
}

int fus_model_get_mass(fus_model* m, void* out)
{
  if (!m || !out)
    return fail(FUS_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(m->ctx->device));
  return FUS_BY_DTYPE(m->op->dtype, model_getset, m, m->m, out, FUS_HOST, false);
}

int64_t fus_model_ndofs(fus_model* m) { return m ? m->op->ndofs : 0; }

} // extern "C"
