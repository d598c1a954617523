// The entry points an operator plugin had BEFORE the row form existed (no cgmres_hip_opplugin_plan), without a solver
// behind them: what cgmres_hip_register_operator sees of a plugin built by an older release of the glue.  Host-only;
// tests/test_user_gmres_row.py checks that such a plugin registers and is planned as the serial form.
#include <cstdint>

#include "cgmres_hip.h"

extern "C" {
int32_t cgmres_hip_opplugin_abi(void) { return CGMRES_HIP_ABI_VERSION; }
void cgmres_hip_opplugin_info(int32_t dims[2]) { dims[0] = 840, dims[1] = 2; }
int cgmres_hip_opplugin_solve(int32_t, int32_t, int32_t, double, const double*, double*, const double*, int32_t*, int32_t*) {
  return CGMRES_HIP_ERUNTIME;
}
const char* cgmres_hip_opplugin_last_error(void) { return "stub: no solver"; }
}
