// Entry lists of the bioheat model's boundary conditions (fus_thermal_set_boundary, fusmi.h "bioheat").  Plain C++: no
// HIP header is needed, a host program may include this file (tests/cpp/thermal_bc_driver.cpp).
//
// The caller describes the boundary per DOF in its own numbering:
//   fixed[d] != 0        the DOF is held at the rise fixed_rise[d]                       (Dirichlet)
//   conv_diag[d] > 0     the DOF carries the surface term m_H[d] = sum_facets h_c |J_f| w_a w_b of a convective face
//                        whose coolant has the rise conv_rise[d]                         (Robin)
// Any array may be null (fixed: no fixed DOF; conv_diag: no convective DOF; fixed_rise / conv_rise: 0).  The kernels
// read sparse lists in INTERNAL numbering instead (dof_perm[d] = internal index of the caller's DOF d), ascending, so
// that neighbouring lanes hit neighbouring lines:
//   fix_idx, fix_val     theta[fix_idx[k]] = fix_val[k]
//   conv_idx, hw, r      b[conv_idx[k]] += r[k] - hw[k] x[conv_idx[k]],   r = hw theta_ext formed in double and rounded
//                        to T once
// A DOF that is both fixed and convective is fixed: it appears in the fixed list alone.  Zero entries of conv_diag are
// dropped.  Everything is validated before anything is written: *out is untouched when an error is returned.
#ifndef FUS_THERMAL_BC_HPP
#define FUS_THERMAL_BC_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

namespace fus
{
enum ThermalBcError
{
  TBC_OK = 0,
  TBC_CONV_DIAG = 1,        // a negative or non-finite conv_diag entry
  TBC_FIXED_RISE = 2,       // a non-finite fixed_rise where fixed is set
  TBC_CONV_RISE = 3,        // a non-finite conv_rise where conv_diag > 0
  TBC_CONV_RISE_ALONE = 4,  // conv_rise given without conv_diag
};

inline const char* thermal_bc_message(int err)
{
  switch (err)
  {
  case TBC_CONV_DIAG: return "conv_diag must be >= 0 and finite at every DOF";
  case TBC_FIXED_RISE: return "fixed_rise must be finite where fixed is set";
  case TBC_CONV_RISE: return "conv_rise must be finite where conv_diag > 0";
  case TBC_CONV_RISE_ALONE: return "conv_rise given without conv_diag";
  default: return "";
  }
}

template <typename T>
struct ThermalBcLists
{
  std::vector<int32_t> fix_idx, conv_idx;
  std::vector<T> fix_val, hw, r;
};

template <typename T>
inline int thermal_bc_lists(int64_t ndofs, const int32_t* dof_perm, const uint8_t* fixed, const T* fixed_rise,
                            const T* conv_diag, const T* conv_rise, ThermalBcLists<T>* out)
{
  if (conv_rise && !conv_diag)
    return TBC_CONV_RISE_ALONE;
  int64_t nf = 0, nc = 0;
  for (int64_t d = 0; d < ndofs; ++d)
  {
    const bool fx = fixed && fixed[d];
    if (conv_diag)
    {
      const double m = (double)conv_diag[d];
      if (!(m >= 0.0) || !std::isfinite(m))
        return TBC_CONV_DIAG;
      if (m > 0.0 && conv_rise && !std::isfinite((double)conv_rise[d]))
        return TBC_CONV_RISE;
      nc += (m > 0.0 && !fx);
    }
    if (fx && fixed_rise && !std::isfinite((double)fixed_rise[d]))
      return TBC_FIXED_RISE;
    nf += fx;
  }
  // (internal index, caller index), ascending by the internal index; dof_perm is injective, so the keys are unique
  std::vector<std::pair<int32_t, int64_t>> fx, cv;
  fx.reserve((size_t)nf), cv.reserve((size_t)nc);
  for (int64_t d = 0; d < ndofs; ++d)
  {
    if (fixed && fixed[d])
      fx.emplace_back(dof_perm[d], d);
    else if (conv_diag && (double)conv_diag[d] > 0.0)
      cv.emplace_back(dof_perm[d], d);
  }
  std::sort(fx.begin(), fx.end());
  std::sort(cv.begin(), cv.end());
  ThermalBcLists<T> L;
  L.fix_idx.resize(fx.size()), L.fix_val.resize(fx.size());
  for (size_t k = 0; k < fx.size(); ++k)
  {
    L.fix_idx[k] = fx[k].first;
    L.fix_val[k] = fixed_rise ? fixed_rise[fx[k].second] : T(0);
  }
  L.conv_idx.resize(cv.size()), L.hw.resize(cv.size()), L.r.resize(cv.size());
  for (size_t k = 0; k < cv.size(); ++k)
  {
    const int64_t d = cv[k].second;
    L.conv_idx[k] = cv[k].first;
    L.hw[k] = conv_diag[d];
    L.r[k] = conv_rise ? (T)((double)conv_diag[d] * (double)conv_rise[d]) : T(0);
  }
  *out = std::move(L);
  return TBC_OK;
}
} // namespace fus

#endif
