// rayleigh.hip -- the Rayleigh integral of a radiating surface (fusmi.h "transducers"): the complex pressure, its gradient
// and the distance to the nearest surface point at a list of targets, from surface points with complex volume velocities,
//
//   S(x)   = sum_s q_s e^{i k r_s} e^{-alpha r_s} / r_s,                                   r_s = |x - x_s|, k = 2 pi f / c
//   S_d(x) = sum_s q_s (i k - alpha - 1/r_s) e^{i k r_s} e^{-alpha r_s} / r_s (x - x_s)_d / r_s
//   P = -i f rho S,  dP/dx_d = -i f rho S_d                                                (omega rho / 2 pi = f rho)
//
// One thread owns one target and keeps its sums in double registers; the sources pass through the workgroup in LDS tiles
// of RAY_TILE points, every lane reading the same address (a broadcast).  Where the targets alone would leave compute units
// idle the sources are cut into chunks along grid.y: every (target block, chunk) workgroup writes its raw sums to a
// workspace [chunks][planes][ntgt] and k_rayleigh_reduce adds them in ascending chunk order and applies -i f rho.  With one
// chunk the main kernel applies it and writes the output itself.  No atomics anywhere: the order of every addition is
// fixed by (nsrc, ntgt, chunks), so two identical calls return the same bits.
//
// Flops per pair as the source below spells them (a multiply-add counts 2; a square root, a reciprocal, a rint, an
// exponential, a sine and a cosine 1 each, whatever the library spends on them): 27 for P, + 22 with the gradient, + 2
// when alpha != 0.  tools/rayleigh_profile.py turns pairs per second into a fraction of the vector rate with these.
#include "core.hpp"

namespace
{

constexpr int RAY_THREADS = 256;   // targets per workgroup, one per thread
constexpr int RAY_TILE = 256;      // sources per LDS tile: 5 doubles each, 10 KB
constexpr int RAY_MAX_CHUNKS = 1024;

struct RayArgs
{
  const double* sxyz;   // [nsrc][3]
  const double* sq;     // [nsrc][2]
  const double* txyz;   // [ntgt][3]
  int64_t nsrc, ntgt, chunk_len;
  double f_over_c;      // revolutions per metre
  double k, alpha;      // 2 pi f / c, Np/m
  double scale;         // f rho
  int planes, want_rmin, final;   // final: one chunk -- apply -i f rho and write `dst` = out; else raw sums, dst = workspace
  double* dst;
};

// e^{i 2 pi u} e^{-alpha r} / r and 1 / r in the scalar type of the precision: double (FUS_RAY_F64) or float (FUS_RAY_MIXED)
template <typename R>
__device__ __forceinline__ void ray_kernel_value(R u, R r, R ar, bool absorb, R& e_re, R& e_im, R& inv)
{
  R s, c;
  if constexpr (std::is_same<R, double>::value)
  {
    sincospi(2.0 * u, &s, &c);
    inv = 1.0 / r;
  }
  else
  {
    sincospif(2.0f * u, &s, &c);
    inv = 1.0f / r;
  }
  R a = inv;
  if (absorb)
  {
    if constexpr (std::is_same<R, double>::value)
      a *= exp(-ar);
    else
      a *= expf(-ar);
  }
  e_re = a * c, e_im = a * s;
}

// r^2 exactly as the documented arithmetic (and the tests' numpy restatement) rounds it: three products and two sums, no
// fused multiply-add -- the phase r f / c in revolutions then carries the same bits as the reference's
__device__ __forceinline__ double ray_r2(double dx, double dy, double dz)
{
#pragma clang fp contract(off)
  return (dx * dx + dy * dy) + dz * dz;
}

template <bool MIXED, bool GRAD>
__global__ void __launch_bounds__(RAY_THREADS) k_rayleigh(const RayArgs a)
{
  using R = typename std::conditional<MIXED, float, double>::type;
  __shared__ double xyz_l[RAY_TILE * 3];
  __shared__ double q_l[RAY_TILE * 2];
  const int tid = threadIdx.x;
  const int64_t t = (int64_t)blockIdx.x * RAY_THREADS + tid;
  const bool live = t < a.ntgt;
  const double tx = live ? a.txyz[3 * t] : 0.0, ty = live ? a.txyz[3 * t + 1] : 0.0, tz = live ? a.txyz[3 * t + 2] : 0.0;
  const int64_t s0 = (int64_t)blockIdx.y * a.chunk_len;
  const int64_t s1 = s0 + a.chunk_len < a.nsrc ? s0 + a.chunk_len : a.nsrc;
  const bool absorb = a.alpha != 0.0;
  const R kk = (R)a.k, al = (R)a.alpha;

  double p_re = 0.0, p_im = 0.0, g_re[3] = {0.0, 0.0, 0.0}, g_im[3] = {0.0, 0.0, 0.0};
  double rmin = INFINITY;

  for (int64_t base = s0; base < s1; base += RAY_TILE)
  {
    const int n = (int)(s1 - base < RAY_TILE ? s1 - base : RAY_TILE);
    __syncthreads();   // the tile before this one has been read
    for (int i = tid; i < 3 * n; i += RAY_THREADS)
      xyz_l[i] = a.sxyz[3 * base + i];
    for (int i = tid; i < 2 * n; i += RAY_THREADS)
      q_l[i] = a.sq[2 * base + i];
    __syncthreads();
    if (live)
      for (int j = 0; j < n; ++j)
      {
        const double dx = tx - xyz_l[3 * j], dy = ty - xyz_l[3 * j + 1], dz = tz - xyz_l[3 * j + 2];
        const double r2 = ray_r2(dx, dy, dz);
        const double r = sqrt(r2);
        rmin = r < rmin ? r : rmin;
        if (r > 0.0)   // a pair at distance 0 contributes nothing; rmin reports it
        {
          const double rev = r * a.f_over_c;
          const double u = rev - rint(rev);
          R e_re, e_im, inv;
          ray_kernel_value<R>((R)u, (R)r, (R)(a.alpha * r), absorb, e_re, e_im, inv);
          const R q_re = (R)q_l[2 * j], q_im = (R)q_l[2 * j + 1];
          const R w_re = q_re * e_re - q_im * e_im;
          const R w_im = q_re * e_im + q_im * e_re;
          p_re += (double)w_re, p_im += (double)w_im;
          if constexpr (GRAD)
          {
            const R cr = -al - inv;                       // (i k - alpha - 1/r) w
            const R v_re = cr * w_re - kk * w_im;
            const R v_im = cr * w_im + kk * w_re;
            const R n0 = (R)dx * inv, n1 = (R)dy * inv, n2 = (R)dz * inv;
            g_re[0] += (double)(v_re * n0), g_im[0] += (double)(v_im * n0);
            g_re[1] += (double)(v_re * n1), g_im[1] += (double)(v_im * n1);
            g_re[2] += (double)(v_re * n2), g_im[2] += (double)(v_im * n2);
          }
        }
      }
  }
  if (!live)
    return;
  // plane p of this chunk; -i f rho (s_re + i s_im) = f rho (s_im - i s_re)
  double* o = a.dst + (a.final ? 0 : (int64_t)blockIdx.y * a.planes * a.ntgt) + t;
  const double K = a.scale;
  o[0] = a.final ? K * p_im : p_re;
  o[a.ntgt] = a.final ? -K * p_re : p_im;
  int p = 2;
  if constexpr (GRAD)
  {
#pragma unroll
    for (int d = 0; d < 3; ++d, p += 2)
    {
      o[(int64_t)p * a.ntgt] = a.final ? K * g_im[d] : g_re[d];
      o[(int64_t)(p + 1) * a.ntgt] = a.final ? -K * g_re[d] : g_im[d];
    }
  }
  if (a.want_rmin)
    o[(int64_t)p * a.ntgt] = rmin;
}

// out[p][t] from ws[c][p][t]: the (re, im) plane pairs summed over the chunks in ascending order, then -i f rho; the rmin
// plane (the last one, where asked for) is the smallest of the chunks'
__global__ void k_rayleigh_reduce(int64_t ntgt, int chunks, int planes, int want_rmin, double scale,
                                  const double* __restrict__ ws, double* __restrict__ out)
{
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntgt)
    return;
  const int npairs = (planes - want_rmin) / 2;
  for (int pr = 0; pr < npairs; ++pr)
  {
    double s_re = 0.0, s_im = 0.0;
    for (int c = 0; c < chunks; ++c)
    {
      const double* w = ws + ((int64_t)c * planes + 2 * pr) * ntgt + t;
      s_re += w[0], s_im += w[ntgt];
    }
    out[(int64_t)(2 * pr) * ntgt + t] = scale * s_im;
    out[(int64_t)(2 * pr + 1) * ntgt + t] = -scale * s_re;
  }
  if (want_rmin)
  {
    double m = INFINITY;
    for (int c = 0; c < chunks; ++c)
    {
      const double v = ws[((int64_t)c * planes + planes - 1) * ntgt + t];
      m = v < m ? v : m;
    }
    out[(int64_t)(planes - 1) * ntgt + t] = m;
  }
}

// -------------------------------------------------------------------------------------------------
// host
// -------------------------------------------------------------------------------------------------
struct RayPlan
{
  int chunks;
  int64_t chunk_len;
  int planes, launches;
  size_t ws_bytes;
};

static int ray_planes(int what) { return 2 + ((what & FUS_RAY_GRAD) ? 6 : 0) + ((what & FUS_RAY_RMIN) ? 1 : 0); }

// Source chunks: option "rayleigh_chunks" when set; else as many as fill the device four workgroups deep -- one chunk where
// the target blocks alone do that -- with at least one full tile of sources each.  No chunk is empty: the count is
// recomputed from the chunk length.
static RayPlan ray_plan(const fus_ctx* c, int64_t nsrc, int64_t ntgt, int what)
{
  const int64_t tblocks = (ntgt + RAY_THREADS - 1) / RAY_THREADS;
  int64_t want = c->rayleigh_chunks;
  if (want <= 0)
  {
    want = (4 * (int64_t)c->num_cus + tblocks - 1) / tblocks;
    want = std::min<int64_t>(want, std::max<int64_t>(1, nsrc / RAY_TILE));
  }
  want = std::max<int64_t>(1, std::min<int64_t>({want, nsrc, (int64_t)RAY_MAX_CHUNKS}));
  RayPlan p{};
  p.chunk_len = (nsrc + want - 1) / want;
  p.chunks = (int)((nsrc + p.chunk_len - 1) / p.chunk_len);
  p.planes = ray_planes(what);
  p.launches = p.chunks > 1 ? 2 : 1;
  p.ws_bytes = p.chunks > 1 ? (size_t)p.chunks * p.planes * (size_t)ntgt * sizeof(double) : 0;
  return p;
}

static bool all_finite(const double* v, int64_t n)
{
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i]))
      return false;
  return true;
}

static int rayleigh(fus_ctx* c, int64_t nsrc, const double* src_xyz, const double* src_q, int64_t ntgt, const double* tgt_xyz,
                    double freq, double cs, double rho, double alpha, int what, int precision, double* out, int space)
{
  hipStream_t st = c->stream;
  const RayPlan plan = ray_plan(c, nsrc, ntgt, what);
  const size_t nout = (size_t)plan.planes * ntgt;
  DevBuf d_sxyz, d_sq, d_txyz, d_out, d_ws;
  RayArgs a{};
  a.sxyz = src_xyz, a.sq = src_q, a.txyz = tgt_xyz;
  double* dst = out;
  if (space == FUS_HOST)
  {
    FUSCHK(d_sxyz.alloc((size_t)nsrc * 3 * sizeof(double), "Rayleigh source points"));
    FUSCHK(d_sq.alloc((size_t)nsrc * 2 * sizeof(double), "Rayleigh source strengths"));
    FUSCHK(d_txyz.alloc((size_t)ntgt * 3 * sizeof(double), "Rayleigh targets"));
    FUSCHK(d_out.alloc(nout * sizeof(double), "Rayleigh output staging"));
    HIPCHK(hipMemcpyAsync(d_sxyz.p, src_xyz, d_sxyz.bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_sq.p, src_q, d_sq.bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_txyz.p, tgt_xyz, d_txyz.bytes, hipMemcpyHostToDevice, st));
    a.sxyz = d_sxyz.as<const double>(), a.sq = d_sq.as<const double>(), a.txyz = d_txyz.as<const double>();
    dst = d_out.as<double>();
  }
  if (plan.chunks > 1)
    FUSCHK(d_ws.alloc(plan.ws_bytes, "Rayleigh chunk workspace"));
  a.nsrc = nsrc, a.ntgt = ntgt, a.chunk_len = plan.chunk_len;
  a.f_over_c = freq / cs, a.k = 2.0 * M_PI * freq / cs, a.alpha = alpha, a.scale = freq * rho;
  a.planes = plan.planes, a.want_rmin = (what & FUS_RAY_RMIN) ? 1 : 0, a.final = plan.chunks == 1;
  a.dst = a.final ? dst : d_ws.as<double>();

  const bool grad = (what & FUS_RAY_GRAD) != 0, mixed = precision == FUS_RAY_MIXED;
  void (*kern)(const RayArgs) = mixed ? (grad ? &k_rayleigh<true, true> : &k_rayleigh<true, false>)
                                      : (grad ? &k_rayleigh<false, true> : &k_rayleigh<false, false>);
  {
    ProfScope ps(c, "rayleigh");
    hipLaunchKernelGGL(kern, dim3(nblk(ntgt, RAY_THREADS), plan.chunks), dim3(RAY_THREADS), 0, st, a);
    HIPCHK(hipGetLastError());
    if (plan.chunks > 1)
    {
      hipLaunchKernelGGL(k_rayleigh_reduce, dim3(nblk(ntgt)), dim3(256), 0, st, ntgt, plan.chunks, plan.planes, a.want_rmin,
                         a.scale, d_ws.as<const double>(), dst);
      HIPCHK(hipGetLastError());
    }
  }
  if (space == FUS_HOST)
    HIPCHK(hipMemcpyAsync(out, dst, nout * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // the staging buffers and the workspace go out of scope
  return FUS_OK;
}

} // namespace

extern "C"
{

int fus_rayleigh(fus_ctx* c, int64_t nsrc, const double* src_xyz, const double* src_q, int64_t ntgt, const double* tgt_xyz,
                 double freq, double cs, double rho, double alpha, int what, int precision, double* out, int space)
{
  if (!c || !src_xyz || !src_q || !tgt_xyz || !out)
    return fail(FUS_ERR_ARG, "fus_rayleigh: null argument");
  if (nsrc < 1 || ntgt < 1)
    return fail(FUS_ERR_ARG, "fus_rayleigh: nsrc and ntgt must be at least 1");
  if (!(freq > 0.0 && std::isfinite(freq)) || !(cs > 0.0 && std::isfinite(cs)) || !(rho > 0.0 && std::isfinite(rho)))
    return fail(FUS_ERR_ARG, "fus_rayleigh: freq, c and rho must be positive and finite");
  if (!(alpha >= 0.0 && std::isfinite(alpha)))
    return fail(FUS_ERR_ARG, "fus_rayleigh: alpha must be >= 0 and finite");
  if (what & ~(FUS_RAY_P | FUS_RAY_GRAD | FUS_RAY_RMIN))
    return fail(FUS_ERR_ARG, "fus_rayleigh: unknown bits in what");
  if (precision != FUS_RAY_F64 && precision != FUS_RAY_MIXED)
    return fail(FUS_ERR_ARG, "fus_rayleigh: precision must be FUS_RAY_F64 or FUS_RAY_MIXED");
  if (space != FUS_HOST && space != FUS_DEVICE)
    return fail(FUS_ERR_ARG, "fus_rayleigh: space must be FUS_HOST or FUS_DEVICE");
  if (space == FUS_HOST
      && !(all_finite(src_xyz, 3 * nsrc) && all_finite(src_q, 2 * nsrc) && all_finite(tgt_xyz, 3 * ntgt)))
    return fail(FUS_ERR_ARG, "fus_rayleigh: a coordinate or a source strength is not finite");
  HIPCHK(hipSetDevice(c->device));
  return rayleigh(c, nsrc, src_xyz, src_q, ntgt, tgt_xyz, freq, cs, rho, alpha, what, precision, out, space);
}

int fus_rayleigh_plan(fus_ctx* c, int64_t nsrc, int64_t ntgt, int what, int64_t out[4])
{
  if (!c || !out)
    return fail(FUS_ERR_ARG, "fus_rayleigh_plan: null argument");
  if (nsrc < 1 || ntgt < 1)
    return fail(FUS_ERR_ARG, "fus_rayleigh_plan: nsrc and ntgt must be at least 1");
  if (what & ~(FUS_RAY_P | FUS_RAY_GRAD | FUS_RAY_RMIN))
    return fail(FUS_ERR_ARG, "fus_rayleigh_plan: unknown bits in what");
  const RayPlan p = ray_plan(c, nsrc, ntgt, what);
  out[0] = p.chunks, out[1] = RAY_THREADS, out[2] = p.launches, out[3] = (int64_t)p.ws_bytes;
  return FUS_OK;
}

} // extern "C"
