// wave_kernels.hpp -- the device kernels that only the wave models launch (wave.hip alone includes this): the shared-DOF
// and interface stage kernels, the boundary partials, the field monitor, the receivers and the per-entry source.  The
// stage algebra they share with the block kernel's epilogue (stage_update_dof and what it uses) is in kernels.hpp.
#ifndef FUS_WAVE_KERNELS_HPP
#define FUS_WAVE_KERNELS_HPP

#include "kernels.hpp"
#include "source_signal.hpp"
#include "source_wave.hpp"

namespace fus
{

// Boundary term of a shared boundary dof for the NEXT stage, produced where that dof's stage update
// has just finished (its new stage velocity is in a register): the dof's last CSR entry is a pseudo
// pair (index >= npairs) exactly when it is a boundary dof, and slot k = pair - npairs holds
//   g(t_next) src[k] - abs[k] v_next (+ dg(t_next) src2[k])        (Linear.hpp:205; forms.py:38-39)
// -- what k_boundary_partial computes in a launch of its own.  enabled = 0: leave the slots alone.
template <typename T>
struct BndNext
{
  int enabled;
  int32_t npairs;
  const T *srcw, *absw, *src2w;
  T gnext, dgnext;
  T* partial;
};

template <typename T>
__device__ __forceinline__ void boundary_next(const BndNext<T>& B, int32_t last_pair, T vnext)
{
#pragma clang fp contract(off)   // written out like stage_update_regs: the same bits from every kernel form
  if (B.enabled && last_pair >= B.npairs)
  {
    const int32_t k = last_pair - B.npairs;
    T v = fmadd(B.gnext, B.srcw[k], -(B.absw[k] * vnext));
    if (B.src2w)
      v = fmadd(B.dgnext, B.src2w[k], v);
    B.partial[last_pair] = v;
  }
}



// The partial sums of the rank-local shared dofs as planes (Layout::pair_pos): plane j holds, at the dof's own
// index, the contribution of the dof's j-th sharing block; cnt[j] dofs (a prefix of the range) have one.
constexpr int FUS_MAX_PLANES = 16;
struct PartialPlanes
{
  int32_t bnd0;                  // slot of the first boundary term (after every pair's partial sum)
  int32_t cnt[FUS_MAX_PLANES];   // 0 for the planes that do not exist
  int32_t off[FUS_MAX_PLANES];
};

// Shared dofs of one rank, partial sums in planes: sum over the planes in ascending order (= ascending block
// order, the order of the CSR form below: same bits), then the boundary term of a shared boundary dof
// (bnd_mask: one bit per dof, bnd_base: boundary dofs ahead of the 64-dof word; the k-th boundary dof's term is
// in slot PL.bnd0 + k), fused with the RK4 stage update.  No index list is read: every access is at s.
// A thread takes 16 bytes of consecutive dofs (two in fp64, four in fp32): planes, minv and the stage's vectors move
// in 16-byte accesses, non-temporal where this kernel is their last reader; the sum of each dof is formed exactly as
// above (the vectors passed in start on a 16-byte boundary: the shared range does, Layout::n_int_pad).
template <typename T, int STAGE>
__global__ void __launch_bounds__(256)
k_shared_stage_planes(int64_t n, const PartialPlanes PL, const uint64_t* __restrict__ bnd_mask,
                      const int32_t* __restrict__ bnd_base, const T* __restrict__ partial,
                      const T* __restrict__ minv, T* __restrict__ vn, T* __restrict__ un, T* __restrict__ u0,
                      T* __restrict__ v0, T* __restrict__ u_, T* __restrict__ v_, T adt, T bdt,
                      const T* __restrict__ m0, const T* __restrict__ mn1, const BndNext<T> B, const LeanRK<T> R)
{
  constexpr int W = 16 / (int)sizeof(T);
  typedef T V __attribute__((ext_vector_type(W)));
  const int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * W;
  if (s >= n)
    return;
  T acc[W];
#pragma unroll
  for (int e = 0; e < W; ++e)
    acc[e] = T(0);
#pragma unroll
  for (int j = 0; j < FUS_MAX_PLANES; ++j)
  {
    const int64_t cnt = PL.cnt[j], off = PL.off[j];
    if (s + W <= cnt)   // (plane_off is a multiple of 16 dofs: verify_layout)
    {
      const V v = __builtin_nontemporal_load(reinterpret_cast<const V*>(partial + off + s));
#pragma unroll
      for (int e = 0; e < W; ++e)
        acc[e] += v[e];
    }
    else
    {
      // the plane ends inside this vector: dof by dof
#pragma unroll
      for (int e = 0; e < W; ++e)
        if (s + e < cnt)
          acc[e] += partial[off + s + e];
    }
  }
  int32_t pair[W];
#pragma unroll
  for (int e = 0; e < W; ++e)
    pair[e] = -1;
  if (bnd_mask)
  {
    // s is a multiple of W, W divides 64: the W dofs share one mask word
    const uint64_t w = bnd_mask[s >> 6];
    const int bit0 = (int)(s & 63);
    if ((w >> bit0) & ((1ull << W) - 1ull))
    {
      const int32_t base = PL.bnd0 + bnd_base[s >> 6];
#pragma unroll
      for (int e = 0; e < W; ++e)
        if ((w >> (bit0 + e)) & 1ull)
        {
          pair[e] = base + __builtin_popcountll(w & ((1ull << (bit0 + e)) - 1ull));
          acc[e] += partial[pair[e]];
        }
    }
  }
  V av;
#pragma unroll
  for (int e = 0; e < W; ++e)
    av[e] = acc[e];
  // (the last thread of a range whose length is no multiple of W updates fewer dofs)
  const int nv = (n - s < W) ? (int)(n - s) : W;
  const V vnext = stage_update_dof<T, STAGE, V>(s, av, minv, vn, un, u0, v0, u_, v_, adt, bdt, m0, mn1, R, nv);
#pragma unroll
  for (int e = 0; e < W; ++e)
    if (e < nv)
      boundary_next<T>(B, pair[e], vnext[e]);
}

// Shared dofs of one rank, CSR form (more than FUS_MAX_PLANES sharers of one dof, or option "planes" = 0):
// fixed-order sum of the partials fused with the RK4 stage update of
// stage_update_dof; vectors are passed offset to the shared range.
template <typename T, int STAGE>
__global__ void __launch_bounds__(256)
k_shared_stage(int64_t n, const int32_t* __restrict__ sh_ptr, const int32_t* __restrict__ sh_pairs,
               const T* __restrict__ partial, const T* __restrict__ minv, T* __restrict__ vn,
               T* __restrict__ un, T* __restrict__ u0, T* __restrict__ v0, T* __restrict__ u_,
               T* __restrict__ v_, T adt, T bdt, const T* __restrict__ m0,
               const T* __restrict__ mn1, const BndNext<T> B, const LeanRK<T> R)
{
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n)
    return;
  T acc = T(0);
  int32_t pair = 0;
  for (int32_t k = sh_ptr[s]; k < sh_ptr[s + 1]; ++k)
  {
    pair = sh_pairs[k];
    acc += partial[pair];
  }
  const T vnext = stage_update_dof<T, STAGE>(s, acc, minv, vn, un, u0, v0, u_, v_, adt, bdt, m0, mn1, R);
  boundary_next<T>(B, pair, vnext);
}

// Interface dofs (held by other ranks too), first half of the exchange: this rank's total of each
// packed dof = fixed-order sum of its block partials, written to the send buffer and to b.
// pack_idx[k] is the dof's index in the internal vectors, sh0 the index of shared slot 0; a dof
// listed for two neighbours is summed twice to the same bits.
template <typename T>
__global__ void k_if_reduce_pack(int64_t n, const int32_t* __restrict__ pack_idx, int64_t sh0,
                                 const int32_t* __restrict__ sh_ptr,
                                 const int32_t* __restrict__ sh_pairs,
                                 const T* __restrict__ partial, T* __restrict__ b,
                                 T* __restrict__ sendbuf)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n)
    return;
  const int64_t u = pack_idx[k], s = u - sh0;
  T acc = T(0);
  for (int32_t q = sh_ptr[s]; q < sh_ptr[s + 1]; ++q)
    acc += partial[sh_pairs[q]];
  sendbuf[k] = acc;
  b[u] = acc;
}

// Second half: every sharer adds the ranks' totals of an interface dof in ascending rank order
// (identical bits everywhere, see k_unpack_ordered) and finishes the RK stage for it.  Vectors are
// passed whole (internal numbering); sh0 = internal index of shared slot 0 (for the dof's CSR row).
template <typename T, int STAGE>
__global__ void __launch_bounds__(256)
k_if_unpack_stage(int64_t nu, const int32_t* __restrict__ uidx, const int32_t* __restrict__ uptr,
                  const int32_t* __restrict__ usrc, const T* __restrict__ recvbuf,
                  const T* __restrict__ b, const T* __restrict__ minv, T* __restrict__ vn,
                  T* __restrict__ un, T* __restrict__ u0, T* __restrict__ v0, T* __restrict__ u_,
                  T* __restrict__ v_, T adt, T bdt, const T* __restrict__ m0,
                  const T* __restrict__ mn1, int64_t sh0, const int32_t* __restrict__ sh_ptr,
                  const int32_t* __restrict__ sh_pairs, const BndNext<T> B, const LeanRK<T> R)
{
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nu)
    return;
  const int64_t u = uidx[j];
  const T own = b[u];
  T acc = T(0);
  for (int32_t k = uptr[j]; k < uptr[j + 1]; ++k)
  {
    const int32_t sidx = usrc[k];
    acc += (sidx < 0) ? own : recvbuf[sidx];
  }
  const T vnext = stage_update_dof<T, STAGE>(u, acc, minv, vn, un, u0, v0, u_, v_, adt, bdt, m0, mn1, R);
  if (B.enabled)
    boundary_next<T>(B, sh_pairs[sh_ptr[u - sh0 + 1] - 1], vnext);
}

// Boundary term of shared boundary dofs, written as one more partial (summed last):
// slot[k] = g(t) src[k] - abs[k] * v_stage[idx[k]]     (Linear.hpp:205; forms.py:38-39)
template <typename T>
__global__ void k_boundary_partial(int64_t nb, const int32_t* __restrict__ idx,
                                   const T* __restrict__ srcw, const T* __restrict__ absw, T gval,
                                   const T* __restrict__ src2w, T dgval,
                                   const T* __restrict__ vstage, T* __restrict__ slot)
{
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nb)
  {
    T v = gval * srcw[k] - absw[k] * vstage[idx[k]];
    if (src2w)
      v += dgval * src2w[k];
    slot[k] = v;
  }
}

// ---- steady-state field monitor (fus_model_monitor, fusmi.h) ---------------------------------------------------
// One sample = one streaming read-modify-write pass over the per-DOF accumulator planes (structure of arrays, each
// plane n = n_internal long, n a multiple of 16):
//   ext  T[2][n]               running max, running min
//   acc  double[2 + 2 NH][n]   sum, sum of squares, cos_1..cos_NH, sin_1..sin_NH  (always fp64, also for T = float)
// A thread takes 16 bytes of the state (2 doubles / 4 floats) and updates every plane of those DOFs: one read of the
// state, one read and one write of each plane, all 16-byte accesses, the planes non-temporal (they are streamed once
// per sample and are far larger than the last-level cache at production sizes).  The 2 NH phase factors
// cos / sin(2 pi k f t_j) are computed on the host in double and arrive by value in the kernarg segment; NH is a
// template parameter so that the plane loop unrolls and nothing is indexed at run time (no scratch).
// first != 0: the first sample of a window -- max = min = x without reading the (zeroed) extremum planes.
template <int NH>
struct MonPhase
{
  double c[NH > 0 ? NH : 1], s[NH > 0 ? NH : 1];
};

template <typename T, int NH>
__global__ void __launch_bounds__(256)
k_monitor_accumulate(int64_t nvec, int64_t n, int first, const T* __restrict__ x, T* __restrict__ ext,
                     double* __restrict__ acc, const MonPhase<NH> ph)
{
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T TV __attribute__((ext_vector_type(VEC)));
  typedef double D2 __attribute__((ext_vector_type(2)));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256)
  {
    const TV xv = *reinterpret_cast<const TV*>(x + i * VEC);
    TV* pmax = reinterpret_cast<TV*>(ext + i * VEC);
    TV* pmin = reinterpret_cast<TV*>(ext + n + i * VEC);
    TV mx = xv, mn = xv;
    if (!first)
    {
      const TV omx = __builtin_nontemporal_load(pmax), omn = __builtin_nontemporal_load(pmin);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        mx[j] = xv[j] > omx[j] ? xv[j] : omx[j], mn[j] = xv[j] < omn[j] ? xv[j] : omn[j];
    }
    __builtin_nontemporal_store(mx, pmax);
    __builtin_nontemporal_store(mn, pmin);
#pragma unroll
    for (int h = 0; h < VEC / 2; ++h)
    {
      const D2 xd = {(double)xv[2 * h], (double)xv[2 * h + 1]};
      D2* p = reinterpret_cast<D2*>(acc + i * VEC + 2 * h);
      const int64_t stride = n / 2;   // plane stride in D2
      __builtin_nontemporal_store(__builtin_nontemporal_load(p) + xd, p);
      __builtin_nontemporal_store(__builtin_nontemporal_load(p + stride) + xd * xd, p + stride);
#pragma unroll
      for (int k = 0; k < NH; ++k)
      {
        D2* pc = p + (2 + k) * stride;
        D2* ps = p + (2 + NH + k) * stride;
        __builtin_nontemporal_store(__builtin_nontemporal_load(pc) + xd * ph.c[k], pc);
        __builtin_nontemporal_store(__builtin_nontemporal_load(ps) + xd * ph.s[k], ps);
      }
    }
  }
}

// ---- relaxation absorption (fus_model_set_relaxation, fusmi.h) -------------------------------------------------
// One sub-step of length h of the local system  v' = -sum_nu A_nu (v - w_nu z_nu),  z_nu' = v - w_nu z_nu  by the
// trapezoidal rule, in closed form (d = 1 + h w / 2;  p = (1 - h w / 2) / d,  e = (h / 2) / d,  g = h w / d):
//   s = sum_nu A_nu e_nu,   r = sum_nu (A_nu g_nu) z_nu                      (ascending nu)
//   v+ = ((1 - s) v + r) / (1 + s),   z_nu+ = p_nu z_nu + e_nu (v + v+)
// p, e, g are computed on the host in double, rounded once to T and arrive by value.  The arithmetic stands once, on
// registers, for the 16-byte path and the DOF-by-DOF tail, written out without contraction like stage_update_regs: a
// DOF's bits do not depend on the path that took it.  s == 0 (no strength at this DOF, padding): v keeps its bits.
template <typename T, int R>
struct RelaxCoef
{
  T p[R], e[R], g[R];
};

template <typename T, int R>
__device__ __forceinline__ void relax_substep_regs(T& v, T (&z)[R], const T (&A)[R], const RelaxCoef<T, R>& c)
{
#pragma clang fp contract(off)
  T s = A[0] * c.e[0], r = (A[0] * c.g[0]) * z[0];
#pragma unroll
  for (int k = 1; k < R; ++k)
  {
    s = s + A[k] * c.e[k];
    r = r + (A[k] * c.g[k]) * z[k];
  }
  const T vp = s == T(0) ? v : ((T(1) - s) * v + r) / (T(1) + s);
  const T vs = v + vp;
#pragma unroll
  for (int k = 0; k < R; ++k)
    z[k] = c.p[k] * z[k] + c.e[k] * vs;
  v = vp;
}

// The streaming form of k_monitor_accumulate: a thread takes 16 bytes of consecutive DOFs (2 doubles / 4 floats) of v
// and of every plane z_nu, A_nu (n = n_internal each, a multiple of 16); all accesses 16-byte and non-temporal, one
// read of A_nu, one read and one write of v and z_nu: (3 R + 2) sizeof(T) bytes per DOF.  R is a template parameter:
// the plane loops unroll and nothing is indexed at run time (no scratch).  No LDS, no atomics.  DOFs past the last
// whole vector (none while n is a multiple of 16) go one by one through the same arithmetic.
template <typename T, int R>
__global__ void __launch_bounds__(256)
k_relax_substep(int64_t nvec, int64_t n, T* __restrict__ v, T* __restrict__ z, const T* __restrict__ A,
                const RelaxCoef<T, R> c)
{
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T TV __attribute__((ext_vector_type(VEC)));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256)
  {
    TV* pv = reinterpret_cast<TV*>(v + i * VEC);
    TV vv = __builtin_nontemporal_load(pv);
    TV zv[R], Av[R];
#pragma unroll
    for (int k = 0; k < R; ++k)
    {
      zv[k] = __builtin_nontemporal_load(reinterpret_cast<const TV*>(z + k * n + i * VEC));
      Av[k] = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A + k * n + i * VEC));
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j)
    {
      T x = vv[j], zz[R], aa[R];
#pragma unroll
      for (int k = 0; k < R; ++k)
        zz[k] = zv[k][j], aa[k] = Av[k][j];
      relax_substep_regs<T, R>(x, zz, aa, c);
      vv[j] = x;
#pragma unroll
      for (int k = 0; k < R; ++k)
        zv[k][j] = zz[k];
    }
    __builtin_nontemporal_store(vv, pv);
#pragma unroll
    for (int k = 0; k < R; ++k)
      __builtin_nontemporal_store(zv[k], reinterpret_cast<TV*>(z + k * n + i * VEC));
  }
  // the tail [nvec VEC, n): fewer than VEC DOFs, the first threads of block 0
  const int64_t d = nvec * VEC + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < VEC && d < n)
  {
    T x = v[d], zz[R], aa[R];
#pragma unroll
    for (int k = 0; k < R; ++k)
      zz[k] = z[k * n + d], aa[k] = A[k * n + d];
    relax_substep_regs<T, R>(x, zz, aa, c);
    v[d] = x;
#pragma unroll
    for (int k = 0; k < R; ++k)
      z[k * n + d] = zz[k];
  }
}

// Per-DOF strengths from the lumped mass actions: A_nu = num_nu / den where den != 0, 0 in the padding slots
// (num = M(a_nu / (rho c^2)) 1 in place, den = M(1 / (rho c^2)) 1, both summed over the sharers beforehand)
template <typename T>
__global__ void __launch_bounds__(256)
k_relax_strength(int64_t n, int nplanes, T* __restrict__ A, const T* __restrict__ den)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
  {
    const T d = den[i];
    for (int k = 0; k < nplanes; ++k)
      A[k * n + i] = d != T(0) ? A[k * n + i] / d : T(0);
  }
}

// ---- absorbing layers (fus_model_set_sponge, fusmi.h) ----------------------------------------------------------
// One sub-step of length h of  u' = -sigma u,  v' = -sigma v  (and z_nu' = -sigma z_nu with relaxation on), solved
// exactly: every field of the DOF is multiplied by g = exp(-sigma h), formed in double and rounded once to T.  The
// arithmetic stands once, on registers, for the 16-byte path and the DOF-by-DOF tail, without contraction: a DOF's
// bits do not depend on the path that took it.  sigma == 0 gives g == 1 exactly and the DOF keeps its bits.
template <typename T, int R>
__device__ __forceinline__ void sponge_substep_regs(T& u, T& v, T (&z)[R > 0 ? R : 1], T sigma, double h)
{
#pragma clang fp contract(off)
  const T g = (T)exp(-(double)sigma * h);
  u = g * u;
  v = g * v;
#pragma unroll
  for (int k = 0; k < R; ++k)
    z[k] = g * z[k];
}

// A sibling of k_relax_substep that runs over the layers only.  A tile is the 256 consecutive 16-byte vectors one
// workgroup takes in one trip (512 doubles / 1024 floats); tiles[0..ntiles) is the ascending list of the tiles that
// hold a nonzero sigma (built by the host at fus_model_set_sponge), the grid strides over that list, and DOFs of
// unlisted tiles are neither read nor written.  Per DOF of a listed tile: sigma, u, v in, u, v out and every z_nu
// in and out, (3 + 2 R + 2) sizeof(T) bytes, all 16-byte and non-temporal.  R is a template parameter: the plane
// loops unroll and nothing is indexed at run time (no scratch).  No LDS, no atomics.  The last tile of the vector
// may be short (n = n_internal is a multiple of 16, not of the tile): every access is bounded by n, and DOFs past
// the last whole vector (none while n is a multiple of 16) go one by one through the same arithmetic.
template <typename T, int R>
__global__ void __launch_bounds__(256)
k_sponge_substep(int64_t ntiles, const int32_t* __restrict__ tiles, int64_t n, double h, const T* __restrict__ sigma,
                 T* __restrict__ u, T* __restrict__ v, T* __restrict__ z)
{
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int RN = R > 0 ? R : 1;
  typedef T TV __attribute__((ext_vector_type(VEC)));
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x)
  {
    const int64_t d = ((int64_t)tiles[t] * 256 + threadIdx.x) * VEC;   // this thread's first DOF
    if (d + VEC <= n)
    {
      const TV sv = __builtin_nontemporal_load(reinterpret_cast<const TV*>(sigma + d));
      TV uv = __builtin_nontemporal_load(reinterpret_cast<const TV*>(u + d));
      TV vv = __builtin_nontemporal_load(reinterpret_cast<const TV*>(v + d));
      TV zv[RN];
#pragma unroll
      for (int k = 0; k < R; ++k)
        zv[k] = __builtin_nontemporal_load(reinterpret_cast<const TV*>(z + k * n + d));
#pragma unroll
      for (int j = 0; j < VEC; ++j)
      {
        T a = uv[j], b = vv[j], zz[RN];
#pragma unroll
        for (int k = 0; k < R; ++k)
          zz[k] = zv[k][j];
        sponge_substep_regs<T, R>(a, b, zz, sv[j], h);
        uv[j] = a, vv[j] = b;
#pragma unroll
        for (int k = 0; k < R; ++k)
          zv[k][j] = zz[k];
      }
      __builtin_nontemporal_store(uv, reinterpret_cast<TV*>(u + d));
      __builtin_nontemporal_store(vv, reinterpret_cast<TV*>(v + d));
#pragma unroll
      for (int k = 0; k < R; ++k)
        __builtin_nontemporal_store(zv[k], reinterpret_cast<TV*>(z + k * n + d));
    }
    else
      for (int64_t e = d; e < n; ++e)   // fewer than VEC DOFs, one thread of the last tile
      {
        T a = u[e], b = v[e], zz[RN];
#pragma unroll
        for (int k = 0; k < R; ++k)
          zz[k] = z[k * n + e];
        sponge_substep_regs<T, R>(a, b, zz, sigma[e], h);
        u[e] = a, v[e] = b;
#pragma unroll
        for (int k = 0; k < R; ++k)
          z[k * n + e] = zz[k];
      }
  }
}

// Monitor read-out in internal numbering: out = (num * plane) / den, or its square root (RMS), rounded to T.
template <typename T>
__global__ void __launch_bounds__(256)
k_monitor_finalise(int64_t n, const double* __restrict__ plane, double num, double den, int root, T* __restrict__ out)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
  {
    const double q = (num * plane[i]) / den;
    out[i] = (T)(root ? sqrt(q) : q);
  }
}

// Receiver sampling (the reference evaluates its solution at points with Function::eval after locating their cells:
// python/src/fenicsxfus/utils.py:10-47, cpp/mwe/parallel_eval_line/main.cpp:49-84).  One wave per receiver r:
//   out[r] = sum_{i0,i1,i2} l_i0(X0) l_i1(X1) l_i2(X2) vec[idx[r][i0,i1,i2]]
// on the RESIDENT vector in internal numbering (idx = dof_perm of the receiver's cell dofs, bas = the 1-D Lagrange
// basis values at the receiver's reference coordinates, both built once in fus_model_set_receivers); lane k adds
// the entries k, k + 64, ... in that order, then a fixed butterfly: the same bits on every call.
template <typename T, int TD>
__global__ void __launch_bounds__(256)
k_sample(int64_t npts, int N, const int32_t* __restrict__ idx, const T* __restrict__ bas,
         const T* __restrict__ vec, T* __restrict__ out)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= npts)
    return;  // (the whole wave leaves)
  const int N2 = N * N, Nd = (TD == 3) ? N2 * N : N2;
  const int32_t* __restrict__ ix = idx + r * Nd;
  const T* __restrict__ b = bas + r * (TD * N);
  T acc = T(0);
  for (int k = lane; k < Nd; k += 64)
  {
    T w;
    if (TD == 3)
    {
      const int i0 = k / N2, rem = k - i0 * N2, i1 = rem / N, i2 = rem - i1 * N;
      w = b[i0] * b[N + i1] * b[2 * N + i2];
    }
    else
    {
      const int i0 = k / N, i1 = k - i0 * N;
      w = b[i0] * b[N + i1];
    }
    acc += w * vec[ix[k]];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    acc += __shfl_xor(acc, o, 64);
  if (lane == 0)
    out[r] = acc;
}

// ---- phased / apodised source (fus_model_set_source, fusmi.h) ---------------------------------------------------
// The block kernel and the shared-dof kernels read the source as  gval * bnd_src[k] (+ dgval * bnd_src2[k]).  A source
// with its own time history per entry keeps those kernels as they are: this kernel evaluates the waveform of
// source_wave.hpp per boundary entry into the weight arrays they read,
//   out[k] = base[k] g_k(t),   out2[k] = base2[k] dg_k(t)   (base2 / out2 only where the model has a dg term),
// for the entries [k0, k1), and the scalars are passed as 1.  base / base2 are the facet weights as the setup left
// them, amp / tau the per-entry amplitude and delay.  An entry without a source weight (a pure absorbing entry)
// stores zeros and evaluates nothing.  One thread per entry, every access at k; the waveform in double, rounded
// to T on store.
template <typename T>
__global__ void __launch_bounds__(256)
k_source_entries(int64_t k0, int64_t k1, const T* __restrict__ base, const T* __restrict__ base2,
                 const T* __restrict__ amp, const T* __restrict__ tau, const SourceWave W, double t,
                 T* __restrict__ out, T* __restrict__ out2)
{
  const int64_t k = k0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= k1)
    return;
  const double b = (double)base[k], b2 = base2 ? (double)base2[k] : 0.0;
  double g = 0.0, dg = 0.0;
  if (b != 0.0 || b2 != 0.0)
    source_wave(W, (double)amp[k], t - (double)tau[k], &g, &dg);
  out[k] = (T)(b * g);
  if (out2)
    out2[k] = (T)(b2 * dg);
}

// ---- sampled drive signals (fus_model_set_source_signals, fusmi.h) ----------------------------------------------
// The sibling of k_source_entries for a source whose time history is a table of samples: the same range [k0, k1),
// the same out / out2 and the same rule about the time a range holds; g_k(t) = amp[k] S_c(t - tau[k]) with
// c = chan[k] and S_c the cubic of source_signal.hpp.  An entry without a source weight or with channel -1 stores
// zeros and reads no sample.  One thread per entry, every per-entry access at k.
// The table is time-major, double[nsamp][nchan], and the channels are numbered in order of first use along the entry
// list (the host renumbers them): the 64 entries of a wavefront that drive one channel each with equal delays (a
// time-reversal mirror) read four contiguous 512-byte rows; with a few channels over many entries (element groups)
// the lanes of a row hit the same few cache lines and the whole table stays in L2.  The segment index depends on the
// entry's delay, so it is a vector value and the samples come through vector loads.
template <typename T>
__global__ void __launch_bounds__(256)
k_source_entries_signal(int64_t k0, int64_t k1, const T* __restrict__ base, const T* __restrict__ base2,
                        const T* __restrict__ amp, const T* __restrict__ tau, const int32_t* __restrict__ chan,
                        const double* __restrict__ table, const SourceSignal P, double t, T* __restrict__ out,
                        T* __restrict__ out2)
{
  const int64_t k = k0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= k1)
    return;
  const double b = (double)base[k], b2 = base2 ? (double)base2[k] : 0.0;
  const int32_t c = chan[k];
  double g = 0.0, dg = 0.0;
  if ((b != 0.0 || b2 != 0.0) && c >= 0)
    source_signal(P, table, c, (double)amp[k], t - (double)tau[k], &g, &dg);
  out[k] = (T)(b * g);
  if (out2)
    out2[k] = (T)(b2 * dg);
}

} // namespace fus

#endif
