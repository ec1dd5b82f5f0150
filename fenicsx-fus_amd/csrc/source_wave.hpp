// Source waveform of one boundary entry with its own amplitude, delay and (optional) burst duration
// (fus_model_set_source, fusmi.h).  Plain C++: no HIP header is needed, a host program may include this file; under
// hipcc the functions are __host__ __device__ and k_source_entries (wave_kernels.hpp) calls them per entry.
//
// For the local time s = t - tau, source frequency f, w0 = 2 pi f, ramp length Lr = 4 / f (the reference's
// window_length, Linear.hpp:185-192) and duration D (0 = continuous wave):
//   W(s)  = 0                                  s <= 0, or D > 0 and s >= D
//         = (1 - cos(pi f s / 4)) / 2          0 < s < Lr                         (the reference's onset ramp)
//         = (1 - cos(pi f (D - s) / 4)) / 2    D > 0 and D - Lr < s < D           (the same ramp, mirrored)
//         = 1                                  otherwise
//   g(s)  = a C W(s) cos(w0 s)
//   dg(s) = a C (W'(s) cos(w0 s) - W(s) w0 sin(w0 s))
// with C = scale p0 w0 / s0 as stage_scalars (wave.hip) has it.  A duration 0 < D < 2 Lr (the ramps would overlap) is
// refused by fus_source_duration_ok.  Everything is evaluated in double for both scalar types of the library.
#ifndef FUS_SOURCE_WAVE_HPP
#define FUS_SOURCE_WAVE_HPP

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FUS_SRC_HD __host__ __device__
#else
#define FUS_SRC_HD
#endif

namespace fus
{
// What every entry of a source shares: passed to the kernel by value.
struct SourceWave
{
  double f;    // source frequency
  double w0;   // 2 pi f
  double C;    // scale p0 w0 / s0
  double D;    // burst duration, 0 = continuous
};

FUS_SRC_HD inline SourceWave source_wave_make(double f, double p0, double s0, double scale, double D)
{
  const double w0 = 2.0 * 3.14159265358979323846 * f;
  return SourceWave{f, w0, scale * p0 * w0 / s0, D};
}

// D = 0, or D >= 2 Lr so that both ramps fit
FUS_SRC_HD inline bool source_duration_ok(double f, double D)
{
  return D == 0.0 || (D >= 8.0 / f && D < INFINITY);
}

// Window W(s) and its derivative dW(s)
FUS_SRC_HD inline void source_window(const SourceWave& p, double s, double* W, double* dW)
{
  const double Lr = 4.0 / p.f, q = 0.25 * 3.14159265358979323846 * p.f;   // ramp argument q x, x in (0, Lr)
  *W = 0.0, *dW = 0.0;
  if (!(s > 0.0) || (p.D > 0.0 && s >= p.D))
    return;
  if (s < Lr)
    *W = 0.5 * (1.0 - cos(q * s)), *dW = 0.5 * q * sin(q * s);
  else if (p.D > 0.0 && s > p.D - Lr)
    *W = 0.5 * (1.0 - cos(q * (p.D - s))), *dW = -0.5 * q * sin(q * (p.D - s));
  else
    *W = 1.0;
}

// g and dg of an entry with amplitude a at local time s = t - tau; both exactly 0 for s <= 0 and for s >= D > 0
FUS_SRC_HD inline void source_wave(const SourceWave& p, double a, double s, double* g, double* dg)
{
  double W, dW;
  source_window(p, s, &W, &dW);
  if (W == 0.0 && dW == 0.0)
  {
    *g = 0.0, *dg = 0.0;
    return;
  }
  const double c = cos(p.w0 * s), sn = sin(p.w0 * s);
  *g = a * p.C * W * c;
  *dg = a * p.C * (dW * c - W * p.w0 * sn);
}
} // namespace fus

#endif
