// Host side of every learner entry point: the status codes of include/deepmimic_hip.h and the check after the launches.
#ifndef DM_LAUNCH_H
#define DM_LAUNCH_H
#include <hip/hip_runtime.h>

#include "../../include/deepmimic_hip.h"

namespace {
// what an entry point returns after its launches: DM_OK, or DM_EHIP if one of them was refused
inline int dm_launch_status() { return hipGetLastError() == hipSuccess ? DM_OK : DM_EHIP; }
}  // namespace
#endif
