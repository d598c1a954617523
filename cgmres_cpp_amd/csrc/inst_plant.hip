// Kernel instantiations of the plant of a closed loop (plant.hip.h) for the built-in models and both scalar types.  A
// translation unit of its own, like inst_horizon.hip and inst_record.hip: the code objects of the tick kernels (the other
// inst_*.hip) hold nothing of it.
#include "factory_impl.hip.h"

namespace cgm {
#define CGM_PLANT_OF(NAME, MODEL, T) \
  int NAME(cgmres_hip_ctx* c, const PlantCall& call) { return plant_variant<MODEL<T>, T>(c, call); }
CGM_PLANT_OF(plant_pendulum_f64, PendulumDev, double)
CGM_PLANT_OF(plant_pendulum_f32, PendulumDev, float)
CGM_PLANT_OF(plant_msd_f64, MsdDev, double)
CGM_PLANT_OF(plant_msd_f32, MsdDev, float)
CGM_PLANT_OF(plant_semiactive_f64, SemiactiveDev, double)
CGM_PLANT_OF(plant_semiactive_f32, SemiactiveDev, float)
#undef CGM_PLANT_OF
}  // namespace cgm
