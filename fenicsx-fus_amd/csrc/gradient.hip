// gradient.hip -- the nodal gradient operator and its pair form (fusmi.h "gradient", "intensity"): one kernel body over
// the operator's blocks, compiled once for every degree (the degree is a run-time argument), and the three entry points
// fus_op_gradient, fus_op_gradient_pairs and fus_model_intensity.
//
//   gradient:  y_d[i] += sum_{(e,q)->i} c_e W_e(q) (grad x)_{e,d}(q)
//   pairs:     y_d[i] += sum_{(e,q)->i} W_e(q) sum_k c_{k,e} [ a_k(i) (grad b_k)_{e,d}(q) - b_k(i) (grad a_k)_{e,d}(q) ]
//
// with (grad x)_e(q) = K(q)^T grad_xi x_e(q), K = J^-1 and W_e(q) = |det J_e(q)| w_q.  J(q) is rebuilt at every point
// from the cell's coordinates (geom.hpp), so no per-point geometry array has to exist.
//
// The kernel reuses the block layout of the operator (layout.hpp): one workgroup per block, an fp64 accumulator image of
// the block's local dofs per component in LDS, the elements visited round by round (the elements of a round share no dof:
// plain LDS read-modify-writes, a barrier between rounds, so the order of the additions at a dof is fixed and the result
// is the same bits on every call, whatever the context option "deterministic" says).  Interior dofs leave LDS once, into the
// internal vector; shared dofs as per-(block, dof) partial sums in planes of their own, reduced by k_shared_reduce in
// ascending block order.  The pair form loops over k inside the element visit and scatters once.
#include <memory>
#include <mutex>
#include <set>

#include "core.hpp"

using namespace fus;

namespace
{

// how a kernel reads an input value: a T vector as it is, or a monitor accumulator plane -- double, scaled and rounded to T
// exactly as k_monitor_finalise (fus_model_monitor_get) does it
template <typename T, typename In>
struct GradIn
{
  const In* a;        // planes a_k (gradient form: the field x)
  const In* b;        // planes b_k (pair form only)
  int64_t stride;     // values between two planes
  double num, den;    // In = double: value = (T)((num * plane[i]) / den)
  __device__ __forceinline__ T get(const In* p, int k, int64_t i) const
  {
    if constexpr (std::is_same<In, double>::value)
      return (T)((num * p[k * stride + i]) / den);
    else
      return p[k * stride + i];
  }
};

template <typename T, typename In>
struct GradArgs
{
  BlockArgs A;
  const int32_t* cell_perm;
  const int32_t* xdm;     // geometry dofmap, caller cell order
  const T* xg;            // node coordinates, 3 per node
  const double* pts;      // 1-D GLL points and weights
  const double* wts;
  const T* Dg;            // derivative table, d[q * N + i] = phi_i'(x_q)
  int N, Nd, slots;
  int gs;                 // threads per element group: 64, 128 or 256
  int comp0, ncomp;       // the components this launch accumulates: [comp0, comp0 + ncomp)
  int nk;                 // pairs K (gradient form: 1)
  GradIn<T, In> in;
  const T* coef;          // [nk][ncells] in internal cell order, or null (= 1)
  int64_t ncells;
  T* y;                   // [tdim][n_internal]
  T* partial;             // [tdim][npart]
  int64_t n_internal, npart;
};

constexpr int GRAD_THREADS = 256;
constexpr int GRAD_QMAX = 6;   // points per thread at the most: 11^3 / 256 rounded up (kernel variant QM = 6; QM = 1
                               // where a group has a thread per point: every quadrilateral, hexahedra up to degree 5)

template <typename T, int TD>
__device__ __forceinline__ void grad_ref_derivs(const T* __restrict__ s, const T* __restrict__ D_l, int N, int q, T (&d)[TD])
{
  if constexpr (TD == 3)
  {
    const int N2 = N * N;
    const int i0 = q / N2, r = q - i0 * N2, i1 = r / N, i2 = r - i1 * N;
    T d0 = T(0), d1 = T(0), d2 = T(0);
    for (int m = 0; m < N; ++m)
    {
      d0 += D_l[i0 * N + m] * s[m * N2 + i1 * N + i2];
      d1 += D_l[i1 * N + m] * s[i0 * N2 + m * N + i2];
      d2 += D_l[i2 * N + m] * s[i0 * N2 + i1 * N + m];
    }
    d[0] = d0, d[1] = d1, d[2] = d2;
  }
  else
  {
    const int i0 = q / N, i1 = q - i0 * N;
    T d0 = T(0), d1 = T(0);
    for (int m = 0; m < N; ++m)
    {
      d0 += D_l[i0 * N + m] * s[m * N + i1];
      d1 += D_l[i1 * N + m] * s[i0 * N + m];
    }
    d[0] = d0, d[1] = d1;
  }
}

// K = J^-1 (K[j][d] = d xi_j / d x_d) and W = |det J| w at point q of the cell whose coordinates are cd
template <typename T, int TD, int GORD>
__device__ __forceinline__ T grad_point_geometry(const T* __restrict__ cd, const double* __restrict__ pts_l,
                                                 const double* __restrict__ wts_l, int N, int q, T (&K)[TD][TD])
{
  if constexpr (TD == 3)
  {
    const int N2 = N * N;
    const int i0 = q / N2, r = q - i0 * N2, i1 = r / N, i2 = r - i1 * N;
    T J[3][3];
    if constexpr (GORD == 1)
      jacobian3<T>(reinterpret_cast<const T(*)[3]>(cd), pts_l[i0], pts_l[i1], pts_l[i2], J);
    else
      jacobian3_q2<T>(reinterpret_cast<const T(*)[3]>(cd), pts_l[i0], pts_l[i1], pts_l[i2], J);
    const T c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const T c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const T c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const T det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    K[0][0] = c00 / det;
    K[1][0] = c01 / det;
    K[2][0] = c02 / det;
    K[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det;
    K[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det;
    K[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) / det;
    K[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) / det;
    K[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
    K[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) / det;
    return (det < 0 ? -det : det) * (T)(wts_l[i0] * wts_l[i1] * wts_l[i2]);
  }
  else
  {
    const int i0 = q / N, i1 = q - i0 * N;
    T J[2][2];
    if constexpr (GORD == 1)
      jacobian2<T>(reinterpret_cast<const T(*)[3]>(cd), pts_l[i0], pts_l[i1], J);
    else
      jacobian2_q2<T>(reinterpret_cast<const T(*)[3]>(cd), pts_l[i0], pts_l[i1], J);
    const T det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    K[0][0] = J[1][1] / det, K[0][1] = -J[0][1] / det, K[1][0] = -J[1][0] / det, K[1][1] = J[0][0] / det;
    return (det < 0 ? -det : det) * (T)(wts_l[i0] * wts_l[i1]);
  }
}

// LDS image (bytes), the same carve on the host (grad_lds_bytes) and in the kernel:
//   double y_l[ncomp][lds_nloc], pts_l[N], wts_l[N]; int32 gi_l[lds_nloc]; T D_l[N * N]; per group T s_a[Nd],
//   s_b[Nd], cd_l[27 * 3] (+ 1 to keep the groups' arrays 8-byte aligned for every T)
static size_t grad_lds_bytes(size_t ts, int ncomp, int lds_nloc, int N, int Nd, int gs)
{
  const size_t ngroups = GRAD_THREADS / gs;
  return (size_t)ncomp * lds_nloc * 8 + 2 * (size_t)N * 8 + (size_t)lds_nloc * 4
         + (((size_t)N * N + 1) & ~(size_t)1) * ts + ngroups * (2 * (((size_t)Nd + 1) & ~(size_t)1) + 82) * ts;
}

template <typename T, typename In, int TD, int GORD, bool PAIRS, int QM>
__global__ void __launch_bounds__(GRAD_THREADS) k_grad_block(const GradArgs<T, In> g)
{
  constexpr int NV = GORD == 1 ? (TD == 3 ? 8 : 4) : (TD == 3 ? 27 : 9);
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int tid = threadIdx.x;
  const int N = g.N, Nd = g.Nd, lds_nloc = g.A.lds_nloc, ncomp = g.ncomp, comp0 = g.comp0;
  const int gs = g.gs, ngroups = GRAD_THREADS / gs, grp = tid / gs, lt = tid - grp * gs;
  const int NdE = (Nd + 1) & ~1;

  double* y_l = reinterpret_cast<double*>(smem_raw);
  double* pts_l = y_l + (size_t)ncomp * lds_nloc;
  double* wts_l = pts_l + N;
  int32_t* gi_l = reinterpret_cast<int32_t*>(wts_l + N);
  T* D_l = reinterpret_cast<T*>(gi_l + lds_nloc);   // lds_nloc is even
  T* s_a = D_l + ((N * N + 1) & ~1) + (size_t)grp * (2 * NdE + 82);
  T* s_b = s_a + NdE;
  T* cd_l = s_b + NdE;

  const BlockRecord* R = g.A.blk_rec + blockIdx.x;
  const int elem_off = R->elem_off, int_off = R->int_off, nelem = R->nelem, nloc = R->nloc, nint = R->nint;
  const int nrounds = R->nrounds;
  const int64_t sh_off = R->sh_off, rounds_off = R->rounds_off, ldm_off = R->ldm_off;
  const int nsh = nloc - nint;

  // ---- prologue: clear the accumulators, the block's local -> internal index table, the 1-D tables ----
  for (int i = tid; i < ncomp * lds_nloc; i += GRAD_THREADS)
    y_l[i] = 0.0;
  for (int i = tid; i < nint; i += GRAD_THREADS)
    gi_l[i] = int_off + i;
  for (int i = tid; i < nsh; i += GRAD_THREADS)
    gi_l[nint + i] = g.A.sh_gidx[sh_off + i];
  for (int i = tid; i < N * N; i += GRAD_THREADS)
    D_l[i] = g.Dg[i];
  if (tid < N)
    pts_l[tid] = g.pts[tid], wts_l[tid] = g.wts[tid];
  __syncthreads();

  // ---- the elements, round by round; the groups of the workgroup take the slots of a round in turn ----
  for (int r = 0; r < nrounds; ++r)
    for (int s0 = 0; s0 < g.slots; s0 += ngroups)
    {
      const int s = s0 + grp;
      int er = (s < g.slots) ? (int)g.A.rounds[rounds_off + (int64_t)r * g.slots + s] : -1;
      if (er >= nelem)
        er = -1;
      const uint16_t* ldm = g.A.ldm + ldm_off + (int64_t)(er < 0 ? 0 : er) * Nd;
      T acc[QM][TD];
#pragma unroll
      for (int j = 0; j < QM; ++j)
#pragma unroll
        for (int d = 0; d < TD; ++d)
          acc[j][d] = T(0);
      if (er >= 0)
      {
        const int64_t cell = g.cell_perm[elem_off + er];
        for (int i = lt; i < NV * 3; i += gs)
          cd_l[i] = g.xg[3 * (int64_t)g.xdm[cell * NV + i / 3] + i % 3];
      }
      for (int k = 0; k < g.nk; ++k)
      {
        if (er >= 0)
          for (int q = lt; q < Nd; q += gs)
          {
            const int64_t gi = gi_l[ldm[q]];
            s_a[q] = g.in.get(g.in.a, k, gi);
            if constexpr (PAIRS)
              s_b[q] = g.in.get(g.in.b, k, gi);
          }
        __syncthreads();
        if (er >= 0)
        {
          const T ck = g.coef ? g.coef[(int64_t)k * g.ncells + elem_off + er] : T(1);
#pragma unroll
          for (int j = 0; j < QM; ++j)
          {
            const int q = lt + j * gs;
            if (q < Nd)
            {
              T da[TD];
              grad_ref_derivs<T, TD>(s_a, D_l, N, q, da);
              if constexpr (PAIRS)
              {
                T db[TD];
                grad_ref_derivs<T, TD>(s_b, D_l, N, q, db);
                const T av = s_a[q], bv = s_b[q];
#pragma unroll
                for (int d = 0; d < TD; ++d)
                  acc[j][d] += ck * (av * db[d] - bv * da[d]);
              }
              else
              {
#pragma unroll
                for (int d = 0; d < TD; ++d)
                  acc[j][d] += ck * da[d];
              }
            }
          }
        }
        __syncthreads();   // the group's values are read; the next k overwrites them
      }
      if (er >= 0)
      {
#pragma unroll
        for (int j = 0; j < QM; ++j)
        {
          const int q = lt + j * gs;
          if (q < Nd)
          {
            T K[TD][TD];
            const T W = grad_point_geometry<T, TD, GORD>(cd_l, pts_l, wts_l, N, q, K);
            const int l = ldm[q];
#pragma unroll
            for (int d = 0; d < TD; ++d)
              if (d >= comp0 && d < comp0 + ncomp)
              {
                T gd = T(0);
#pragma unroll
                for (int jj = 0; jj < TD; ++jj)
                  gd += K[jj][d] * acc[j][jj];
                y_l[(size_t)(d - comp0) * lds_nloc + l] += (double)(W * gd);   // no other element of this round holds dof l
              }
          }
        }
      }
      __syncthreads();   // rounds are ordered; the group's coordinates are free again
    }

  // ---- epilogue: every dof written once, rounded to T ----
  for (int c = 0; c < ncomp; ++c)
  {
    const double* yc = y_l + (size_t)c * lds_nloc;
    T* yo = g.y + (int64_t)(comp0 + c) * g.n_internal + int_off;
    for (int i = tid; i < nint; i += GRAD_THREADS)
      yo[i] = (T)yc[i];
    T* po = g.partial + (int64_t)(comp0 + c) * g.npart;
    for (int i = tid; i < nsh; i += GRAD_THREADS)
      po[g.A.sh_ppos[sh_off + i]] = (T)yc[nint + i];
  }
}

// out[d][i] (caller numbering) from y[d][perm[i]] (internal): mode 0 accumulates the weighted sums, mode 1 overwrites with
// the recovered nodal value y / den
template <typename T>
__global__ void k_grad_out(int64_t ndofs, int tdim, int64_t n_internal, const int32_t* __restrict__ perm,
                           const T* __restrict__ y, const T* __restrict__ den, int nodal, T* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ndofs)
    return;
  const int64_t p = perm[i];
  for (int d = 0; d < tdim; ++d)
  {
    const T v = y[d * n_internal + p];
    if (nodal)
      out[d * ndofs + i] = v / den[p];
    else
      out[d * ndofs + i] += v;
  }
}

// c[k][e] = 1 / (2 rho_e omega_k), omega_k = 2 pi (k + 1) f: formed in double, rounded to T
template <typename T>
__global__ void k_intensity_coef(int64_t ncells, int nk, double two_pi_f, const T* __restrict__ rho, T* __restrict__ c)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ncells)
    return;
  for (int k = 0; k < nk; ++k)
    c[(int64_t)k * ncells + e] = (T)(1.0 / (2.0 * (double)rho[e] * (two_pi_f * (double)(k + 1))));
}

// -------------------------------------------------------------------------------------------------
// host
// -------------------------------------------------------------------------------------------------
struct GradPlan
{
  int gs, ncomp;
  size_t lds;
};

// The components a launch holds in LDS: all of them where the image fits, else one per launch (component passes: 12
// bytes per local dof and the groups' element images, against the 8 + sizeof(T) bytes per local dof, the exchange tiles and
// the local dofmaps of the block kernel's own image, which op_setup_device checked against the same 160 KB), and last the
// component passes with one element group of the whole workgroup.
static GradPlan grad_plan(const fus_op* op)
{
  const int gs = op->Nd <= 64 ? 64 : (op->Nd <= 128 ? 128 : 256);
  const GradPlan tries[3] = {{gs, op->tdim, 0}, {gs, 1, 0}, {GRAD_THREADS, 1, 0}};
  GradPlan p{};
  for (const GradPlan& t : tries)
  {
    p = t;
    p.lds = grad_lds_bytes(op->ts, p.ncomp, op->A.lds_nloc, op->N, op->Nd, p.gs);
    if (p.lds <= 160 * 1024)
      break;
  }
  return p;
}

template <typename T>
static int grad_ensure(fus_op* op)
{
  hipStream_t st = op->ctx->stream;
  const Layout& L = op->L;
  if (!op->d_grad_y)
  {
    FUSCHK(dalloc_bytes(op->allocs, &op->d_grad_part, (size_t)op->tdim * L.n_partial * sizeof(T), true, st));
    FUSCHK(dalloc_bytes(op->allocs, &op->d_grad_coef, (size_t)16 * op->ncells * sizeof(T), true, st));
    FUSCHK(dalloc_bytes(op->allocs, &op->d_grad_y, (size_t)op->tdim * L.n_internal * sizeof(T), true, st));
  }
  return FUS_OK;
}

// den = M(1) 1 in internal numbering, once per operator (local: no sum over the sharers of an interface dof)
template <typename T>
static int grad_denominator(fus_op* op)
{
  if (op->d_grad_den)
    return FUS_OK;
  hipStream_t st = op->ctx->stream;
  const int64_t n = op->L.n_internal;
  void* den = nullptr;
  FUSCHK(dalloc_bytes(op->allocs, &den, (size_t)n * sizeof(T), true, st));
  T* ones = static_cast<T*>(op->d_tmp_x);
  T* cone = static_cast<T*>(op->d_tmp_coef);
  hipLaunchKernelGGL((k_fill<T>), dim3(nblk(n)), dim3(256), 0, st, n, ones, T(1));
  hipLaunchKernelGGL((k_fill<T>), dim3(nblk(op->ncells)), dim3(256), 0, st, op->ncells, cone, T(1));
  HIPCHK(hipGetLastError());
  FUSCHK(d_apply_internal(op, OP_MASS, cone, ones, den));
  HIPCHK(hipMemsetAsync(ones, 0, (size_t)n * sizeof(T), st));   // the operator's scratch vector keeps zeros in its padding slots
  op->d_grad_den = den;
  return FUS_OK;
}

template <typename T, typename In, bool PAIRS>
static int grad_launch(fus_op* op, int nk, const GradIn<T, In>& in, const T* coef_internal)
{
  fus_ctx* c = op->ctx;
  hipStream_t st = c->stream;
  const Layout& L = op->L;
  const GradPlan plan = grad_plan(op);
  if (plan.lds > 160 * 1024)
    return fail(FUS_ERR_STATE, "gradient kernel: the one-component LDS image exceeds the block kernel's");
  GradArgs<T, In> g{};
  g.A = op->A;
  g.cell_perm = op->d_cell_perm, g.xdm = op->d_xdm, g.xg = static_cast<const T*>(op->d_xg);
  g.pts = static_cast<const double*>(op->d_pts), g.wts = static_cast<const double*>(op->d_wts);
  g.Dg = static_cast<const T*>(op->d_Dg);
  g.N = op->N, g.Nd = op->Nd, g.slots = L.slots, g.gs = plan.gs;
  g.nk = nk, g.in = in, g.coef = coef_internal, g.ncells = op->ncells;
  g.y = static_cast<T*>(op->d_grad_y), g.partial = static_cast<T*>(op->d_grad_part);
  g.n_internal = L.n_internal, g.npart = L.n_partial;

  void (*kern)(const GradArgs<T, In>) = nullptr;
  if (op->tdim == 2)
    kern = op->geom_order == 1 ? &k_grad_block<T, In, 2, 1, PAIRS, 1> : &k_grad_block<T, In, 2, 2, PAIRS, 1>;
  else if (op->Nd <= plan.gs)
    kern = op->geom_order == 1 ? &k_grad_block<T, In, 3, 1, PAIRS, 1> : &k_grad_block<T, In, 3, 2, PAIRS, 1>;
  else
    kern = op->geom_order == 1 ? &k_grad_block<T, In, 3, 1, PAIRS, GRAD_QMAX> : &k_grad_block<T, In, 3, 2, PAIRS, GRAD_QMAX>;
  if (plan.lds > 64 * 1024)
  {
    // the attribute is per device and kernel: set once (again, harmlessly, if two threads race on the first launch)
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(c->device, reinterpret_cast<const void*>(kern));
    if (!done.count(key))
    {
      HIPCHK(hipFuncSetAttribute(key.second, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      done.insert(key);
    }
  }
  {
    ProfScope ps(c, "gradient");
    for (int c0 = 0; c0 < op->tdim; c0 += plan.ncomp)
    {
      g.comp0 = c0, g.ncomp = plan.ncomp;
      hipLaunchKernelGGL(kern, dim3(L.nblocks), dim3(GRAD_THREADS), plan.lds, st, g);
      HIPCHK(hipGetLastError());
    }
    if (L.n_shared > 0)
      for (int d = 0; d < op->tdim; ++d)
      {
        hipLaunchKernelGGL((k_shared_reduce<T, int64_t>), dim3(nblk(L.n_shared)), dim3(256), 0, st, (int64_t)0, L.n_shared,
                           op->d_sh_ptr, op->d_sh_pairs, static_cast<const T*>(op->d_grad_part) + (int64_t)d * g.npart,
                           static_cast<T*>(op->d_grad_y) + (int64_t)d * L.n_internal + L.n_int_pad);
        HIPCHK(hipGetLastError());
      }
  }
  return FUS_OK;
}

// the sums in op->d_grad_y -> out (T[tdim][ndofs], caller numbering, `space`)
template <typename T>
static int grad_finish(fus_op* op, void* out, int mode, int space)
{
  hipStream_t st = op->ctx->stream;
  const int64_t nd = op->ndofs, nout = nd * op->tdim;
  const bool nodal = mode == FUS_GRAD_NODAL;
  if (nodal)
    FUSCHK(grad_denominator<T>(op));
  DevBuf stage;
  T* dst = static_cast<T*>(out);
  if (space == FUS_HOST)
  {
    FUSCHK(stage.alloc(nout * sizeof(T), "gradient output staging"));
    dst = stage.as<T>();
    if (!nodal)
      HIPCHK(hipMemcpyAsync(dst, out, nout * sizeof(T), hipMemcpyHostToDevice, st));
  }
  hipLaunchKernelGGL((k_grad_out<T>), dim3(nblk(nd)), dim3(256), 0, st, nd, op->tdim, op->L.n_internal, op->d_dof_perm,
                     static_cast<const T*>(op->d_grad_y), static_cast<const T*>(op->d_grad_den), nodal ? 1 : 0, dst);
  HIPCHK(hipGetLastError());
  if (space == FUS_HOST)
    HIPCHK(hipMemcpyAsync(out, dst, nout * sizeof(T), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return FUS_OK;
}

// rows of per-cell coefficients (T[rows][ncells], caller cell order, `space`) -> op->d_grad_coef in internal cell order
template <typename T>
static int grad_coef(fus_op* op, int rows, const void* coeffs, int space, const T** out)
{
  hipStream_t st = op->ctx->stream;
  const int64_t nc = op->ncells;
  T* ci = static_cast<T*>(op->d_grad_coef);
  T* cc = ci + 8 * nc;
  const T* src = static_cast<const T*>(coeffs);
  if (space == FUS_HOST)
  {
    HIPCHK(hipMemcpyAsync(cc, coeffs, (size_t)rows * nc * sizeof(T), hipMemcpyHostToDevice, st));
    src = cc;
  }
  for (int k = 0; k < rows; ++k)
    hipLaunchKernelGGL((k_cells_to_internal<T>), dim3(nblk(nc)), dim3(256), 0, st, nc, op->d_cell_perm, src + (int64_t)k * nc,
                       ci + (int64_t)k * nc);
  HIPCHK(hipGetLastError());
  *out = ci;
  return FUS_OK;
}

// planes of caller-numbered vectors (T[rows][ndofs], `space`) -> internal numbering, T[rows][n_internal] in `dst`
template <typename T>
static int grad_to_internal(fus_op* op, int rows, const void* v, int space, DevBuf& stage, T* dst)
{
  hipStream_t st = op->ctx->stream;
  const int64_t nd = op->ndofs, n = op->L.n_internal;
  const T* src = static_cast<const T*>(v);
  if (space == FUS_HOST)
  {
    FUSCHK(stage.alloc((size_t)rows * nd * sizeof(T), "gradient input staging"));
    HIPCHK(hipMemcpyAsync(stage.p, v, (size_t)rows * nd * sizeof(T), hipMemcpyHostToDevice, st));
    src = stage.as<const T>();
  }
  for (int k = 0; k < rows; ++k)
    hipLaunchKernelGGL((k_to_internal<T>), dim3(nblk(nd)), dim3(256), 0, st, nd, op->d_dof_perm, src + (int64_t)k * nd,
                       dst + (int64_t)k * n);
  HIPCHK(hipGetLastError());
  return FUS_OK;
}

template <typename T>
static int op_gradient(fus_op* op, int npairs, const void* a, const void* b, const void* coeffs, void* out, int mode, int space)
{
  hipStream_t st = op->ctx->stream;
  const int64_t n = op->L.n_internal;
  FUSCHK(grad_ensure<T>(op));
  const bool pairs = b != nullptr;
  const int rows = pairs ? 2 * npairs : 1;
  DevBuf st_a, st_b;
  const size_t need = (size_t)rows * n * sizeof(T);
  if (need > op->grad_in_bytes)   // it only grows
  {
    HIPCHK(hipStreamSynchronize(st));
    if (op->d_grad_in)
    {
      op->allocs.erase(std::find(op->allocs.begin(), op->allocs.end(), op->d_grad_in));
      (void)hipFree(op->d_grad_in);
      op->d_grad_in = nullptr, op->grad_in_bytes = 0;
    }
    FUSCHK(dalloc_bytes(op->allocs, &op->d_grad_in, need, false, st));
    op->grad_in_bytes = need;
  }
  T* ai = static_cast<T*>(op->d_grad_in);
  FUSCHK(grad_to_internal<T>(op, npairs, a, space, st_a, ai));
  if (pairs)
    FUSCHK(grad_to_internal<T>(op, npairs, b, space, st_b, ai + (int64_t)npairs * n));
  const T* ci = nullptr;
  if (coeffs)
    FUSCHK(grad_coef<T>(op, npairs, coeffs, space, &ci));
  const GradIn<T, T> in{ai, pairs ? ai + (int64_t)npairs * n : ai, n, 1.0, 1.0};
  if (pairs)
    FUSCHK((grad_launch<T, T, true>(op, npairs, in, ci)));
  else
    FUSCHK((grad_launch<T, T, false>(op, 1, in, ci)));
  FUSCHK(grad_finish<T>(op, out, mode, space));
  HIPCHK(hipStreamSynchronize(st));   // the staging buffers go out of scope
  return FUS_OK;
}

template <typename T>
static int model_intensity(fus_model* m, int nharm, const void* coef, void* out, int space)
{
  fus_op* op = m->op;
  hipStream_t st = m->ctx->stream;
  const int64_t n = op->L.n_internal, nc = op->ncells;
  FUSCHK(grad_ensure<T>(op));
  const T* ci = nullptr;
  if (coef)
  {
    std::vector<T> h((size_t)nharm * nc);
    if (space == FUS_HOST)
      memcpy(h.data(), coef, h.size() * sizeof(T));
    else
      HIPCHK(hipMemcpy(h.data(), coef, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    for (const T v : h)
      if (!std::isfinite((double)v))
        return fail(FUS_ERR_ARG, "fus_model_intensity: coef must be finite in every cell and row");
    FUSCHK(grad_coef<T>(op, nharm, coef, space, &ci));
  }
  else
  {
    T* cd = static_cast<T*>(op->d_grad_coef);
    hipLaunchKernelGGL((k_intensity_coef<T>), dim3(nblk(nc)), dim3(256), 0, st, nc, nharm, 2.0 * M_PI * m->mon.freq,
                       static_cast<const T*>(m->d_rho0), cd);
    HIPCHK(hipGetLastError());
    ci = cd;
  }
  // the accumulator planes, read in place: sum, sum of squares, cos_1.., sin_1.. (ModelMonitor, core.hpp)
  const double* acc = reinterpret_cast<const double*>(m->mon.d_mon.as<const T>() + 2 * n);
  const GradIn<T, double> in{acc + 2 * n, acc + (size_t)(2 + m->mon.nharm) * n, n, 2.0, (double)m->mon.n};
  FUSCHK((grad_launch<T, double, true>(op, nharm, in, ci)));
  return grad_finish<T>(op, out, FUS_GRAD_NODAL, space);
}

} // namespace

extern "C"
{

int fus_op_gradient(fus_op* op, const void* x, const void* coeffs, void* out, int mode, int space)
{
  if (!op || !x || !out)
    return fail(FUS_ERR_ARG, "fus_op_gradient: null argument");
  if (mode != FUS_GRAD_WEIGHTED && mode != FUS_GRAD_NODAL)
    return fail(FUS_ERR_ARG, "fus_op_gradient: mode must be FUS_GRAD_WEIGHTED or FUS_GRAD_NODAL");
  if (space != FUS_HOST && space != FUS_DEVICE)
    return fail(FUS_ERR_ARG, "fus_op_gradient: space must be FUS_HOST or FUS_DEVICE");
  HIPCHK(hipSetDevice(op->ctx->device));
  return FUS_BY_DTYPE(op->dtype, op_gradient, op, 1, x, nullptr, coeffs, out, mode, space);
}

int fus_op_gradient_plan(fus_op* op, int64_t out[4])
{
  if (!op || !out)
    return fail(FUS_ERR_ARG, "fus_op_gradient_plan: null argument");
  const GradPlan p = grad_plan(op);
  out[0] = (op->tdim + p.ncomp - 1) / p.ncomp, out[1] = p.ncomp, out[2] = p.gs, out[3] = (int64_t)p.lds;
  return FUS_OK;
}

int fus_op_gradient_pairs(fus_op* op, int npairs, const void* a, const void* b, const void* coeffs, void* out, int mode,
                          int space)
{
  if (!op || !a || !b || !coeffs || !out)
    return fail(FUS_ERR_ARG, "fus_op_gradient_pairs: null argument");
  if (npairs < 1 || npairs > 8)
    return fail(FUS_ERR_ARG, "fus_op_gradient_pairs: npairs must lie in 1..8");
  if (mode != FUS_GRAD_WEIGHTED && mode != FUS_GRAD_NODAL)
    return fail(FUS_ERR_ARG, "fus_op_gradient_pairs: mode must be FUS_GRAD_WEIGHTED or FUS_GRAD_NODAL");
  if (space != FUS_HOST && space != FUS_DEVICE)
    return fail(FUS_ERR_ARG, "fus_op_gradient_pairs: space must be FUS_HOST or FUS_DEVICE");
  HIPCHK(hipSetDevice(op->ctx->device));
  return FUS_BY_DTYPE(op->dtype, op_gradient, op, npairs, a, b, coeffs, out, mode, space);
}

int fus_model_intensity(fus_model* m, int nharm, const void* coef, void* out, int space)
{
  if (!m || !out)
    return fail(FUS_ERR_ARG, "fus_model_intensity: null argument");
  if (space != FUS_HOST && space != FUS_DEVICE)
    return fail(FUS_ERR_ARG, "fus_model_intensity: space must be FUS_HOST or FUS_DEVICE");
  if (!m->op->neigh.empty())
    return fail(FUS_ERR_STATE, "fus_model_intensity: the operator has neighbours; the sums over the sharers of an interface "
                               "dof have no exchange here (use fus_op_gradient_pairs, FUS_GRAD_WEIGHTED)");
  if (m->mon.every <= 0)
    return fail(FUS_ERR_STATE, "fus_model_intensity: the model's monitor is off (fus_model_monitor)");
  if (m->mon.which != FUS_U)
    return fail(FUS_ERR_STATE, "fus_model_intensity: the monitor watches FUS_V; the intensity needs the pressure, FUS_U");
  if (m->mon.n == 0)
    return fail(FUS_ERR_STATE, "fus_model_intensity: the monitor has taken no sample yet");
  if (nharm < 1 || nharm > 8)
    return fail(FUS_ERR_ARG, "fus_model_intensity: nharm must lie in 1..8");
  if (m->mon.nharm < nharm)
    return fail(FUS_ERR_STATE, "fus_model_intensity: the monitor holds fewer harmonics than nharm asks for");
  HIPCHK(hipSetDevice(m->ctx->device));
  return FUS_BY_DTYPE(m->op->dtype, model_intensity, m, nharm, coef, out, space);
}

} // extern "C"
