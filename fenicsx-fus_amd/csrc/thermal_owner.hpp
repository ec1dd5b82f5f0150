// Owner mask of the bioheat model's step rule on several ranks (fus_thermal_lambda_max, fusmi.h "bioheat").  Plain C++:
// no HIP header is needed, a host program may include this file (tests/cpp/thermal_owner_driver.cpp).
//
// The inner products of the power iteration run over the DOFs of all ranks and must count an interface DOF -- one that
// several ranks hold -- once.  The halo lists of fus_op_set_neighbours name, per interface DOF j of a rank,
//   uidx[j]                          its internal index, and
//   usrc[uptr[j] .. uptr[j + 1])     the addends of its ordered sum in ascending rank order: -1 for the rank's own
//                                    value, otherwise a slot of the receive buffer.
// A rank OWNS an interface DOF when its own value comes first in that list, that is when no sharer has a lower rank;
// every other DOF of a rank is its own.  Over all ranks every DOF is thus owned exactly once, by its lowest sharer.
#ifndef FUS_THERMAL_OWNER_HPP
#define FUS_THERMAL_OWNER_HPP

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace fus
{
enum ThermalOwnerError
{
  TOWN_OK = 0,
  TOWN_INDEX = 1,   // an entry of uidx outside [0, n_internal)
  TOWN_LIST = 2,    // uptr not ascending, an empty addend list, or a list without the rank's own value
};

// mask[i] = 1: this rank counts internal index i (padding slots included: the vectors are zero there); 0: a lower rank does
inline int thermal_owner_mask(int64_t n_internal, int64_t n_uidx, const int32_t* uidx, const int32_t* uptr,
                              const int32_t* usrc, std::vector<uint8_t>* mask)
{
  for (int64_t j = 0; j < n_uidx; ++j)
  {
    if (uidx[j] < 0 || uidx[j] >= n_internal)
      return TOWN_INDEX;
    if (uptr[j] < 0 || uptr[j + 1] <= uptr[j])
      return TOWN_LIST;
    bool own = false;
    for (int32_t k = uptr[j]; k < uptr[j + 1]; ++k)
      own = own || usrc[k] < 0;
    if (!own)
      return TOWN_LIST;
  }
  std::vector<uint8_t> m((size_t)n_internal, 1);
  for (int64_t j = 0; j < n_uidx; ++j)
    m[(size_t)uidx[j]] = usrc[uptr[j]] < 0 ? 1 : 0;
  *mask = std::move(m);
  return TOWN_OK;
}
} // namespace fus

#endif
