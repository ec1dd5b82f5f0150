// Sampled drive signal of one boundary entry (fus_model_set_source_signals, fusmi.h): the cubic interpolant of a table
// of samples, its value and its time derivative.  Plain C++ like source_wave.hpp: no HIP header is needed, a host
// program may include this file; under hipcc the functions are __host__ __device__ and k_source_entries_signal
// (wave_kernels.hpp) calls them per entry.
//
// Channel c has the samples s_j = table[j * nchan + c], j in [0, nsamp), at the times t_first + j ds (the table is
// time-major: the four rows a wavefront reads are contiguous over the channels).  With x = (t - t_first) / ds,
// j = floor(x) and u = x - j in [0, 1), segment j is the Catmull-Rom cubic through s_{j-1} .. s_{j+2}, samples outside
// [0, nsamp) counting as 0:
//   S(t)  = w_0(u) s_{j-1} + w_1(u) s_j + w_2(u) s_{j+1} + w_3(u) s_{j+2}
//   S'(t) = (w_0'(u) s_{j-1} + w_1'(u) s_j + w_2'(u) s_{j+1} + w_3'(u) s_{j+2}) / ds
//   w_0 = (-u + 2u^2 - u^3) / 2   w_1 = (2 - 5u^2 + 3u^3) / 2   w_2 = (u + 4u^2 - 3u^3) / 2   w_3 = (-u^2 + u^3) / 2
// for the segments j = -1 .. nsamp - 1; S = S' = 0 exactly for t < t_first - ds and for t >= t_first + nsamp ds.
// S passes through the samples, S' is the analytic derivative of the same cubic and equals (s_{j+1} - s_{j-1}) / (2 ds)
// at sample j, from both sides: S is C^1 on the support, and across its two ends when the first and the last sample
// are 0 (a signal that starts and ends at rest; otherwise S' jumps there by s_0 / (2 ds), resp. s_{nsamp-1} / (2 ds)).
// Everything is evaluated in double for both scalar types of the library.
#ifndef FUS_SOURCE_SIGNAL_HPP
#define FUS_SOURCE_SIGNAL_HPP

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FUS_SIG_HD __host__ __device__
#else
#define FUS_SIG_HD
#endif

namespace fus
{
// What every entry of a sampled source shares: passed to the kernel by value.
struct SourceSignal
{
  double t_first;   // time of sample 0
  double ds;        // sample spacing, > 0
  int64_t nsamp;    // samples per channel, >= 2
  int64_t nchan;    // channels of the table = its row length
};

// nsamp >= 2, ds > 0 and finite, t_first finite
FUS_SIG_HD inline bool source_signal_ok(int64_t nsamp, double t_first, double ds)
{
  return nsamp >= 2 && ds > 0.0 && ds < INFINITY && t_first > -INFINITY && t_first < INFINITY;
}

// Segment index j in [-1, nsamp - 1] and local coordinate u in [0, 1) of time t; false outside the support (and for a
// NaN time), where the signal is exactly 0
FUS_SIG_HD inline bool signal_segment(const SourceSignal& p, double t, int64_t* j, double* u)
{
  const double x = (t - p.t_first) / p.ds;
  if (!(x >= -1.0) || !(x < (double)p.nsamp))
    return false;
  const double fl = floor(x);
  *j = (int64_t)fl, *u = x - fl;
  return true;
}

// The four weights of the samples j-1 .. j+2 at u, and their derivatives with respect to u
FUS_SIG_HD inline void signal_weights(double u, double w[4], double dw[4])
{
  const double u2 = u * u, u3 = u2 * u;
  w[0] = 0.5 * (-u + 2.0 * u2 - u3);
  w[1] = 0.5 * (2.0 - 5.0 * u2 + 3.0 * u3);
  w[2] = 0.5 * (u + 4.0 * u2 - 3.0 * u3);
  w[3] = 0.5 * (-u2 + u3);
  dw[0] = 0.5 * (-1.0 + 4.0 * u - 3.0 * u2);
  dw[1] = 0.5 * (-10.0 * u + 9.0 * u2);
  dw[2] = 0.5 * (1.0 + 8.0 * u - 9.0 * u2);
  dw[3] = 0.5 * (-2.0 * u + 3.0 * u2);
}

// g = a S_c(t) and dg = a S_c'(t) of channel c (0 <= c < p.nchan) of the time-major table; reads at most the four
// samples j-1 .. j+2 that lie in [0, nsamp), none outside the support
FUS_SIG_HD inline void source_signal(const SourceSignal& p, const double* table, int64_t c, double a, double t,
                                     double* g, double* dg)
{
  int64_t j;
  double u;
  *g = 0.0, *dg = 0.0;
  if (!signal_segment(p, t, &j, &u))
    return;
  double w[4], dw[4];
  signal_weights(u, w, dw);
  double s = 0.0, d = 0.0;
  for (int q = 0; q < 4; ++q)
  {
    const int64_t r = j - 1 + q;
    if (r >= 0 && r < p.nsamp)
    {
      const double v = table[r * p.nchan + c];
      s += w[q] * v, d += dw[q] * v;
    }
  }
  *g = a * s;
  *dg = a * (d / p.ds);
}
} // namespace fus

#endif
