// Kernel instantiations of cgmres_hip_horizon_device (horizon.hip.h) for the built-in models, both scalar types and both
// layouts of U / ptau.  A translation unit of its own: the code objects of the tick kernels (the other inst_*.hip) stay
// byte for byte what they were without this entry point, so no tick kernel moves in its code object.
#include "factory_impl.hip.h"

namespace cgm {
#define CGM_HORIZON_OF(NAME, MODEL, T)                                                         \
  int NAME(cgmres_hip_ctx* c, const void* x_dev, const cgmres_hip_horizon_out* out) {         \
    return horizon_variant<MODEL<T>, T>(c, x_dev, out);                                        \
  }
CGM_HORIZON_OF(horizon_pendulum_f64, PendulumDev, double)
CGM_HORIZON_OF(horizon_pendulum_f32, PendulumDev, float)
CGM_HORIZON_OF(horizon_msd_f64, MsdDev, double)
CGM_HORIZON_OF(horizon_msd_f32, MsdDev, float)
CGM_HORIZON_OF(horizon_semiactive_f64, SemiactiveDev, double)
CGM_HORIZON_OF(horizon_semiactive_f32, SemiactiveDev, float)
#undef CGM_HORIZON_OF
}  // namespace cgm
