// thermal_kernels.hpp -- the device kernels of the bioheat model, launched by thermal.hip alone
#ifndef FUS_THERMAL_KERNELS_HPP
#define FUS_THERMAL_KERNELS_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "thermal_response.hpp"

namespace fus
{

// ---- Pennes bioheat model (fus_thermal_*, fusmi.h) -------------------------------------------------------------------
// State: the temperature rise theta over the baseline, rho C dtheta/dt = div(k grad theta) - W theta + Q, discretised as
//   dtheta/dt = f(theta) = (K(-k) theta - m_W .* theta + sigma h) ./ m_C
// with the diagonal vectors m_C = M(rho C) 1, m_W = M(W) 1 and the heat load h (W per DOF).  One launch per RK4 stage
// after the operator's two (k_block_op, k_shared_reduce) finishes the stage: with b = K(-k) Theta_i for the stage input
// Theta_i (Theta_0 = theta_0),
//   k_i = (b - m_W Theta_i + sigma h) / m_C
//   STAGE 0 (first):   acc = theta_0 + dt b_0 k_0,   Theta_1 = theta_0 + dt a_1 k_0      (theta_0 is the stage input)
//   STAGE 1 (middle):  acc += dt b_i k_i,            Theta_{i+1} = theta_0 + dt a_{i+1} k_i   (in place over Theta_i)
//   STAGE 3 (last):    theta_0 = acc + dt b_3 k_3,   D += (dt / 60) exp2(-c (43 - T)),  T = t_base + theta_0 in double,
//                      c = 1 for T >= 43, else 2 (CEM43, rectangle rule on the end-of-step temperature)
// A streaming kernel in the monitor kernel's form: a thread takes 16 bytes of every vector (2 doubles / 4 floats), all
// accesses 16-byte and non-temporal, a grid-stride loop, no LDS, no atomics.  All vectors are n_internal long (a multiple
// of 16) in internal numbering; their padding slots hold zeros and stay zero, since minv = 1 / m_C is 0 there.  The dose
// plane is double for every T and is read and written once per step, in the last stage's pass.
template <typename T>
struct ThermalStage
{
  const T* b;       // K(-k) Theta_i
  const T* th_in;   // stage input Theta_i (stage 0: theta_0)
  T* th_out;        // next stage input (stages 0-2; may alias th_in) | new theta_0 (last stage)
  const T* th0;     // theta_0 (middle stages)
  T* acc;           // accumulator (written by stage 0, read and written by the middle stages, read by the last)
  const T* minv;    // 1 / m_C, 0 in the padding slots
  const T* mw;      // m_W
  const T* h;       // heat load
  double* dose;     // CEM43 plane, minutes (last stage)
  T adt, bdt, sigma;
  double dt60, t_base;
};

// D + (dt / 60) 2^(-c (43 - T)), every operation rounded by itself (no contraction): numpy reproduces the argument of
// exp2 bit for bit and the sum up to the rounding of exp2
__device__ __forceinline__ double thermal_dose_add(double D, double theta, double t_base, double dt60)
{
#pragma clang fp contract(off)
  const double Tc = t_base + theta;
  const double c = Tc >= 43.0 ? 1.0 : 2.0;
  const double term = dt60 * exp2(-(c * (43.0 - Tc)));
  return D + term;
}

// The stage derivative of both schemes, k_i of RK4 and f of RKL2: (b - m_W x + sigma h) / m_C at the stage input x, on V = T
// (the interface kernels) or on 16-byte vectors of T (the streaming kernels) -- the same operations on every element
template <typename V, typename T>
__device__ __forceinline__ V thermal_rate(V b, V mw, V x, T sigma, V h, V minv)
{
  return (b - mw * x + sigma * h) * minv;
}

template <typename T, int STAGE>
__global__ void __launch_bounds__(256) k_thermal_stage(int64_t nvec, const ThermalStage<T> A)
{
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T TV __attribute__((ext_vector_type(VEC)));
  typedef double D2 __attribute__((ext_vector_type(2)));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256)
  {
    const TV b = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.b) + i);
    const TV th = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.th_in) + i);
    const TV mi = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.minv) + i);
    const TV mw = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.mw) + i);
    const TV h = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.h) + i);
    const TV k = thermal_rate(b, mw, th, A.sigma, h, mi);
    if (STAGE == 0)
    {
      __builtin_nontemporal_store(th + A.bdt * k, reinterpret_cast<TV*>(A.acc) + i);
      __builtin_nontemporal_store(th + A.adt * k, reinterpret_cast<TV*>(A.th_out) + i);
    }
    else if (STAGE == 1)
    {
      const TV t0 = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.th0) + i);
      const TV a = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.acc) + i);
      __builtin_nontemporal_store(a + A.bdt * k, reinterpret_cast<TV*>(A.acc) + i);
      __builtin_nontemporal_store(t0 + A.adt * k, reinterpret_cast<TV*>(A.th_out) + i);
    }
    else
    {
      const TV a = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.acc) + i);
      const TV tn = a + A.bdt * k;
      __builtin_nontemporal_store(tn, reinterpret_cast<TV*>(A.th_out) + i);
#pragma unroll
      for (int j = 0; j < VEC / 2; ++j)
      {
        D2* p = reinterpret_cast<D2*>(A.dose + i * VEC + 2 * j);
        D2 d = __builtin_nontemporal_load(p);
        d[0] = thermal_dose_add(d[0], (double)tn[2 * j], A.t_base, A.dt60);
        d[1] = thermal_dose_add(d[1], (double)tn[2 * j + 1], A.t_base, A.dt60);
        __builtin_nontemporal_store(d, p);
      }
    }
  }
}

// ---- super-time-stepping of the bioheat model (fus_thermal_steps_sts; coefficients: sts_coef.hpp) ----
// One launch per RKL2 stage after the operator's two finishes the stage: with b = K(-k) Y_{j-1},
//   f = (b - m_W Y_{j-1} + sigma h) / m_C
//   KIND 0 (first):   F_0 = f,  Y_1 = Y_0 + mdt f                                    (y1 = Y_0; out = Y_1)
//   KIND 1 (middle):  Y_j = mu Y_{j-1} + nu Y_{j-2} + om Y_0 + mdt f + gdt F_0       (out = the place of Y_{j-2}, or a
//                     buffer of its own for j = 2, where Y_{j-2} = Y_0 is kept)
//   KIND 2 (last):    theta = Y_s over Y_0 (same index, same thread; with s = 2 also y2 = Y_0), and the dose by the
//                     trapezoid rule on the temperatures at both ends of the step, in double:
//                     D += (dt / 120) (R(T_old) + R(T_new)),  R(T) = exp2(-c (43 - T)),  T = t_base + theta
// with om = 1 - mu - nu, mdt = mut_j dt, gdt = gat_j dt rounded to T on the host.  The form of k_thermal_stage: 16-byte
// non-temporal accesses, a grid-stride loop, no LDS, no atomics; n_internal-long vectors whose padding stays zero
// (minv = 0 there).  out may alias y2 and y0: every load of an index precedes its store in the one thread that owns it.
template <typename T>
struct ThermalSts
{
  const T* b;       // K(-k) Y_{j-1}
  const T* y1;      // Y_{j-1}
  const T* y2;      // Y_{j-2} (middle, last)
  const T* y0;      // Y_0 (middle, last)
  T* f0;            // F_0: written by the first stage, read by the others
  T* out;           // Y_j
  const T* minv;    // 1 / m_C, 0 in the padding slots
  const T* mw;      // m_W
  const T* h;       // heat load
  double* dose;     // CEM43 plane, minutes (last stage)
  T mu, nu, om, mdt, gdt, sigma;
  double dt120, t_base;
};

// D + (dt / 120) (R(T_old) + R(T_new)), every operation rounded by itself as in thermal_dose_add
__device__ __forceinline__ double thermal_dose_add_trapezoid(double D, double th_old, double th_new, double t_base,
                                                             double dt120)
{
#pragma clang fp contract(off)
  const double To = t_base + th_old, Tn = t_base + th_new;
  const double co = To >= 43.0 ? 1.0 : 2.0, cn = Tn >= 43.0 ? 1.0 : 2.0;
  const double ro = exp2(-(co * (43.0 - To))), rn = exp2(-(cn * (43.0 - Tn)));
  const double term = dt120 * (ro + rn);
  return D + term;
}

// Y_j of a middle or last RKL2 stage, on V = T or on 16-byte vectors of T like thermal_rate.  The weights come one by one:
// with the struct as the argument the fp32 streaming kernels allocate their scalar registers in another order
template <typename V, typename T>
__device__ __forceinline__ V thermal_sts_combine(T mu, V y1, T nu, V y2, T om, V y0, T mdt, V f, T gdt, V f0)
{
  return mu * y1 + nu * y2 + om * y0 + mdt * f + gdt * f0;
}

template <typename T, int KIND>
__global__ void __launch_bounds__(256) k_thermal_sts_stage(int64_t nvec, const ThermalSts<T> A)
{
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T TV __attribute__((ext_vector_type(VEC)));
  typedef double D2 __attribute__((ext_vector_type(2)));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256)
  {
    const TV b = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.b) + i);
    const TV y1 = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.y1) + i);
    const TV mi = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.minv) + i);
    const TV mw = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.mw) + i);
    const TV h = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.h) + i);
    const TV f = thermal_rate(b, mw, y1, A.sigma, h, mi);
    if (KIND == 0)
    {
      __builtin_nontemporal_store(f, reinterpret_cast<TV*>(A.f0) + i);
      __builtin_nontemporal_store(y1 + A.mdt * f, reinterpret_cast<TV*>(A.out) + i);
    }
    else
    {
      const TV y2 = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.y2) + i);
      const TV y0 = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.y0) + i);
      const TV f0 = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.f0) + i);
      const TV yn = thermal_sts_combine(A.mu, y1, A.nu, y2, A.om, y0, A.mdt, f, A.gdt, f0);
      __builtin_nontemporal_store(yn, reinterpret_cast<TV*>(A.out) + i);
      if (KIND == 2)
      {
#pragma unroll
        for (int j = 0; j < VEC / 2; ++j)
        {
          D2* p = reinterpret_cast<D2*>(A.dose + i * VEC + 2 * j);
          D2 d = __builtin_nontemporal_load(p);
          d[0] = thermal_dose_add_trapezoid(d[0], (double)y0[2 * j], (double)yn[2 * j], A.t_base, A.dt120);
          d[1] = thermal_dose_add_trapezoid(d[1], (double)y0[2 * j + 1], (double)yn[2 * j + 1], A.t_base, A.dt120);
          __builtin_nontemporal_store(d, p);
        }
      }
    }
  }
}

// Heat load h = m_q .* q with m_q = M(q_coef) 1, rounded to T once.  q != nullptr: a nodal field in internal numbering.
// Otherwise q = Q / nsamp in double from the field monitor's sum-of-squares plane Q (k_monitor_accumulate, acc plane 1):
// the squared RMS pressure, which never leaves the device and never passes through a square root.
template <typename T>
__global__ void __launch_bounds__(256)
k_thermal_heat(int64_t nvec, const T* __restrict__ mq, const T* __restrict__ q, const double* __restrict__ Q, double nsamp,
               T* __restrict__ h)
{
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T TV __attribute__((ext_vector_type(VEC)));
  typedef double D2 __attribute__((ext_vector_type(2)));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256)
  {
    const TV m = __builtin_nontemporal_load(reinterpret_cast<const TV*>(mq) + i);
    TV out;
    if (q)
      out = m * __builtin_nontemporal_load(reinterpret_cast<const TV*>(q) + i);
    else
    {
#pragma unroll
      for (int j = 0; j < VEC / 2; ++j)
      {
        const D2 s = __builtin_nontemporal_load(reinterpret_cast<const D2*>(Q + i * VEC + 2 * j));
        out[2 * j] = (T)((double)m[2 * j] * (s[0] / nsamp));
        out[2 * j + 1] = (T)((double)m[2 * j + 1] * (s[1] / nsamp));
      }
    }
    __builtin_nontemporal_store(out, reinterpret_cast<TV*>(h) + i);
  }
}

// Per-harmonic heat load (fus_thermal_set_heat_from_harmonics), one launch per harmonic k in ascending order:
//   sum += (double) m_k .* (C_k^2 + S_k^2),   m_k = M(2 alpha_k / (rho c)) 1,
// C_k, S_k the field monitor's cosine / sine planes of harmonic k (k_monitor_accumulate).  The running sum lives in one
// double plane: `first` starts it (the plane is not read), every launch but the last stores it back, and the last one
// (scale != 0) forms sum * scale, scale = 2 / nsamp^2, rounds to T once and stores h -- so the fp32 error does not grow
// with the number of harmonics.  A single harmonic (first and last) touches no sum plane at all.  Streaming like
// k_thermal_heat: 16-byte accesses, grid-stride over nvec, no LDS, no atomics.
template <typename T>
__global__ void __launch_bounds__(256)
k_thermal_heat_harmonic(int64_t nvec, const T* __restrict__ mk, const double* __restrict__ Ck, const double* __restrict__ Sk,
                        double* __restrict__ sum, int first, double scale, T* __restrict__ h)
{
#pragma clang fp contract(off)
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T TV __attribute__((ext_vector_type(VEC)));
  typedef double D2 __attribute__((ext_vector_type(2)));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256)
  {
    const TV m = __builtin_nontemporal_load(reinterpret_cast<const TV*>(mk) + i);
    TV out;
#pragma unroll
    for (int j = 0; j < VEC / 2; ++j)
    {
      const int64_t at = i * VEC + 2 * j;
      const D2 c = __builtin_nontemporal_load(reinterpret_cast<const D2*>(Ck + at));
      const D2 s = __builtin_nontemporal_load(reinterpret_cast<const D2*>(Sk + at));
      D2 a;
      a[0] = (double)m[2 * j] * (c[0] * c[0] + s[0] * s[0]);
      a[1] = (double)m[2 * j + 1] * (c[1] * c[1] + s[1] * s[1]);
      if (!first)
        a = __builtin_nontemporal_load(reinterpret_cast<const D2*>(sum + at)) + a;
      if (scale != 0.0)
        out[2 * j] = (T)(a[0] * scale), out[2 * j + 1] = (T)(a[1] * scale);
      else
        __builtin_nontemporal_store(a, reinterpret_cast<D2*>(sum + at));
    }
    if (scale != 0.0)
      __builtin_nontemporal_store(out, reinterpret_cast<TV*>(h) + i);
  }
}

// ---- perfusion response and Arrhenius damage (fus_thermal_set_response, fus_thermal_set_damage; laws: thermal_response.hpp) ----
// One launch after a step's last stage (several ranks: after the interface kernel; RKL2: after the fixed values are put
// back), over all n_internal slots.  From the state the step ended in, T = t_base + (double) theta_{n+1} and D_{n+1}:
//   MODE & 1 (response):  m_Weff = (T)((double) m_W * (P(T) * S(D)))       the perfusion plane the NEXT step's stages read
//   MODE & 2 (damage):    Omega += dt2 * (r_prev + r(T)),  r_prev = r(T)   dt2 = dt / 2: the trapezoid rule over the step
// every operation rounded by itself.  prime != 0 is the launch before the first step after the state, the response or the
// boundary changed: m_Weff and r_prev are formed from the state as it stands, Omega and the old r_prev are not read.
// The form of k_thermal_stage: a thread takes 16 bytes of every T vector (and the 2 or 4 doubles that belong to them), all
// accesses 16-byte and non-temporal, a grid-stride loop, no LDS, no atomics.  The knot table and the scalars arrive by value
// in the arguments; P selects its segment by comparisons against them, never through an index into memory.  m_Weff is zero
// in the padding slots because m_W is; the padding slots of the double planes, like the dose plane's, hold values nobody
// reads.  Every operand has the same bits on all sharers of an interface DOF, so the results do too, without an exchange.
template <typename T>
struct ThermalRespond
{
  const T* th;          // theta_{n+1}
  const double* dose;   // D_{n+1} (response)
  const T* mw;          // m_W (response)
  T* mweff;             // m_Weff (response)
  double* omega;        // Omega (damage)
  double* rprev;        // r at the last state seen (damage)
  ThermalResponse R;
  double lnA, Ea, dt2, t_base;
  int prime;
};

template <typename T, int MODE>
__global__ void __launch_bounds__(256) k_thermal_response(int64_t nvec, const ThermalRespond<T> A)
{
#pragma clang fp contract(off)
  constexpr int VEC = 16 / (int)sizeof(T);
  typedef T TV __attribute__((ext_vector_type(VEC)));
  typedef double D2 __attribute__((ext_vector_type(2)));
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256)
  {
    const TV th = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.th) + i);
    TV mw, out;
    if (MODE & 1)
      mw = __builtin_nontemporal_load(reinterpret_cast<const TV*>(A.mw) + i);
#pragma unroll
    for (int j = 0; j < VEC / 2; ++j)
    {
      const int64_t at = i * VEC + 2 * j;
      const double T0 = A.t_base + (double)th[2 * j], T1 = A.t_base + (double)th[2 * j + 1];
      if (MODE & 1)
      {
        const D2 d = __builtin_nontemporal_load(reinterpret_cast<const D2*>(A.dose + at));
        const double phi0 = thermal_response_P(A.R, T0) * thermal_response_S(A.R, d[0]);
        const double phi1 = thermal_response_P(A.R, T1) * thermal_response_S(A.R, d[1]);
        out[2 * j] = (T)((double)mw[2 * j] * phi0), out[2 * j + 1] = (T)((double)mw[2 * j + 1] * phi1);
      }
      if (MODE & 2)
      {
        D2 rn;
        rn[0] = thermal_damage_rate(A.lnA, A.Ea, T0), rn[1] = thermal_damage_rate(A.lnA, A.Ea, T1);
        if (!A.prime)
        {
          const D2 ro = __builtin_nontemporal_load(reinterpret_cast<const D2*>(A.rprev + at));
          D2 om = __builtin_nontemporal_load(reinterpret_cast<const D2*>(A.omega + at));
          om[0] = om[0] + A.dt2 * (ro[0] + rn[0]), om[1] = om[1] + A.dt2 * (ro[1] + rn[1]);
          __builtin_nontemporal_store(om, reinterpret_cast<D2*>(A.omega + at));
        }
        __builtin_nontemporal_store(rn, reinterpret_cast<D2*>(A.rprev + at));
      }
    }
    if (MODE & 1)
      __builtin_nontemporal_store(out, reinterpret_cast<TV*>(A.mweff) + i);
  }
}

// q_coef = 2 alpha / (rho c) per cell, internal cell order (alpha: amplitude absorption, Np/m)
template <typename T>
__global__ void k_thermal_qcoef(int64_t n, const T* __restrict__ alpha, const T* __restrict__ rho, const T* __restrict__ c,
                                T* __restrict__ out)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n)
    out[e] = T(2) * alpha[e] / (rho[e] * c[e]);
}

// Power iteration of fus_thermal_lambda_max: y = (K(k) x + phi_max m_W x) / m_C from b = K(-k) x; phi_max bounds the
// perfusion response from above (1 without one: the product with m_W is then exact)
template <typename T>
__global__ void k_thermal_power(int64_t n, const T* __restrict__ b, const T* __restrict__ x, const T* __restrict__ mw,
                                T phi_max, const T* __restrict__ minv, T* __restrict__ y)
{
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = ((phi_max * mw[i]) * x[i] - b[i]) * minv[i];
}

// ---- boundary conditions of the bioheat model (fus_thermal_set_boundary; entry lists: thermal_bc.hpp) ----
// Both conditions are diagonal on the GLL-collocated space, so the stage kernels above stay as they are and the device
// work is proportional to the surface: sparse lists of internal DOF indices, unique and ascending (neighbouring lanes hit
// neighbouring lines), one thread per entry, every access at k or idx[k], no atomics, no LDS.
//
// Convective (Robin) faces, -k dtheta/dn = h_c (theta - theta_ext): with hw = m_H = sum_facets h_c |J_f| w_a w_b and
// r = m_H theta_ext, the surface term joins the operator result between the shared reduction and the stage kernel,
//   b[idx[k]] += r[k] - hw[k] x[idx[k]],
// x the vector the operator was applied to.  r == nullptr: the homogeneous part (the power iteration, whose
// y = (m_W x - b) / m_C thereby gains m_H x).
template <typename T>
__global__ void __launch_bounds__(256)
k_thermal_robin(int64_t nr, const int32_t* __restrict__ idx, const T* __restrict__ hw, const T* __restrict__ r,
                const T* __restrict__ x, T* __restrict__ b)
{
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nr)
    return;
  const int32_t i = idx[k];
  b[i] += (r ? r[k] : T(0)) - hw[k] * x[i];
}

// Fixed (Dirichlet) DOFs: theta[idx[k]] = val[k] (val == nullptr: 0).  With minv_bc != nullptr also minv_bc[idx[k]] = 0:
// the stage kernels and the power kernel read that copy of 1 / m_C in place of the original, so the stage derivative
// vanishes at a fixed DOF exactly as it does in a padding slot, and no mask is read in the streaming loops.
template <typename T>
__global__ void __launch_bounds__(256)
k_thermal_fix(int64_t nf, const int32_t* __restrict__ idx, const T* __restrict__ val, T* __restrict__ theta,
              T* __restrict__ minv_bc)
{
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nf)
    return;
  const int32_t i = idx[k];
  theta[i] = val ? val[k] : T(0);
  if (minv_bc)
    minv_bc[i] = T(0);
}

// ---- the bioheat model on several ranks: interface DOFs (fusmi.h "bioheat", several ranks) ----
// The streaming stage kernels above then stop at the first interface slot; the DOFs that other ranks hold too are
// finished here, after the exchange, in the form of k_if_unpack_stage: one thread per entry j of uidx, the ordered sum
// over usrc[uptr[j] .. uptr[j + 1]) of the rank's own total b[u] (-1) and the sharers' totals in the receive buffer
// (ascending rank order: the same bits on every sharer), then the stage update of that one DOF with the formulas, the
// argument structs and the dose functions of the streaming kernels.  Every other operand is identical on all sharers
// (m_C, m_W and the heat weight are ordered sums themselves, the state starts identical), so the results are too.
// uidx is ascending and mostly contiguous: neighbouring lanes hit neighbouring addresses.  No LDS, no atomics; a
// thread reads every value of its DOF before it writes one, so th_out / out may alias the inputs as they do above.
template <typename T>
__device__ __forceinline__ T thermal_if_sum(int64_t j, T own, const int32_t* __restrict__ uptr,
                                            const int32_t* __restrict__ usrc, const T* __restrict__ recvbuf)
{
  T acc = T(0);
  for (int32_t k = uptr[j]; k < uptr[j + 1]; ++k)
  {
    const int32_t sidx = usrc[k];
    acc += (sidx < 0) ? own : recvbuf[sidx];
  }
  return acc;
}

template <typename T, int STAGE>
__global__ void __launch_bounds__(256)
k_thermal_if_stage(int64_t nu, const int32_t* __restrict__ uidx, const int32_t* __restrict__ uptr,
                   const int32_t* __restrict__ usrc, const T* __restrict__ recvbuf, const ThermalStage<T> A)
{
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nu)
    return;
  const int64_t u = uidx[j];
  const T b = thermal_if_sum<T>(j, A.b[u], uptr, usrc, recvbuf);
  const T th = A.th_in[u];
  const T k = thermal_rate(b, A.mw[u], th, A.sigma, A.h[u], A.minv[u]);
  if (STAGE == 0)
  {
    A.acc[u] = th + A.bdt * k;
    A.th_out[u] = th + A.adt * k;
  }
  else if (STAGE == 1)
  {
    const T t0 = A.th0[u], a = A.acc[u];
    A.acc[u] = a + A.bdt * k;
    A.th_out[u] = t0 + A.adt * k;
  }
  else
  {
    const T tn = A.acc[u] + A.bdt * k;
    A.th_out[u] = tn;
    A.dose[u] = thermal_dose_add(A.dose[u], (double)tn, A.t_base, A.dt60);
  }
}

template <typename T, int KIND>
__global__ void __launch_bounds__(256)
k_thermal_if_sts_stage(int64_t nu, const int32_t* __restrict__ uidx, const int32_t* __restrict__ uptr,
                       const int32_t* __restrict__ usrc, const T* __restrict__ recvbuf, const ThermalSts<T> A)
{
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nu)
    return;
  const int64_t u = uidx[j];
  const T b = thermal_if_sum<T>(j, A.b[u], uptr, usrc, recvbuf);
  const T y1 = A.y1[u];
  const T f = thermal_rate(b, A.mw[u], y1, A.sigma, A.h[u], A.minv[u]);
  if (KIND == 0)
  {
    A.f0[u] = f;
    A.out[u] = y1 + A.mdt * f;
  }
  else
  {
    const T y2 = A.y2[u], y0 = A.y0[u], f0 = A.f0[u];
    const T yn = thermal_sts_combine(A.mu, y1, A.nu, y2, A.om, y0, A.mdt, f, A.gdt, f0);
    A.out[u] = yn;
    if (KIND == 2)
      A.dose[u] = thermal_dose_add_trapezoid(A.dose[u], (double)y0, (double)yn, A.t_base, A.dt120);
  }
}

} // namespace fus

#endif
