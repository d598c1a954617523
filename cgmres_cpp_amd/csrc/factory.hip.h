// One factory per (model, scalar type): each lives in its own translation unit (inst_*.hip) so the kernel
// instantiations compile in parallel.  Returns nullptr when the requested variant cannot serve the sizes;
// *resolved receives the variant actually chosen (1 = lane, 2 = wg).
// Next to each factory, what works on the concrete type of the context it made and is no virtual of cgmres_hip_ctx:
// horizon_* = cgmres_hip_horizon_device (factory_impl.hip.h: horizon_variant), all six in inst_horizon.hip.
#pragma once
#include "ctx_common.hip.h"

namespace cgm {
using HorizonFn = int(cgmres_hip_ctx*, const void* x_dev, const cgmres_hip_horizon_out* out);
cgmres_hip_ctx* make_pendulum_f64(const cgmres_hip_config& cfg, int* resolved);
cgmres_hip_ctx* make_pendulum_f32(const cgmres_hip_config& cfg, int* resolved);
cgmres_hip_ctx* make_msd_f64(const cgmres_hip_config& cfg, int* resolved);
cgmres_hip_ctx* make_msd_f32(const cgmres_hip_config& cfg, int* resolved);
cgmres_hip_ctx* make_semiactive_f64(const cgmres_hip_config& cfg, int* resolved);
cgmres_hip_ctx* make_semiactive_f32(const cgmres_hip_config& cfg, int* resolved);
HorizonFn horizon_pendulum_f64, horizon_pendulum_f32, horizon_msd_f64, horizon_msd_f32, horizon_semiactive_f64,
    horizon_semiactive_f32;
// plant_* = one launch of the plant kernel (plant.hip.h, factory_impl.hip.h: plant_variant), all six in inst_plant.hip.
using PlantFn = int(cgmres_hip_ctx*, const PlantCall& call);
PlantFn plant_pendulum_f64, plant_pendulum_f32, plant_msd_f64, plant_msd_f32, plant_semiactive_f64, plant_semiactive_f32;
// One record of a closed loop / the ensemble of a batch (record.hip.h), on the context's stream: the log rows and the
// statistics of x [batch][nx], u [batch][nu] and the status arrays given; any destination may be null.  Independent of
// model and mapping, so there is one function, in inst_record.hip.
struct RecordOut {
  void *x_log, *u_log;
  int32_t *n_ax_log, *reason_log;
  const double* centre;
  double* moments;
  int32_t* counts;
};
int record_take(cgmres_hip_ctx* c, const void* x, const void* u, const int32_t* n_ax, const int32_t* reason, const RecordOut& o);
// The preview of a sampled reference signal (preview.hip.h), on the context's stream: preview_fill = one launch of the
// kernel (LoopSeqs::preview_fill), preview_export = rows [n_ticks][batch][dim_p*(dv+1)] from the handle's time on, without
// touching it.  Independent of model and mapping like record_take: both in inst_preview.hip.
int preview_fill(cgmres_hip_ctx* c, const PreviewCall& call);
int preview_export(cgmres_hip_ctx* c, const PreviewSig& s, int n_ticks, void* rows);
#ifdef CGM_STAMPS
long long* debug_stamps_ptr();  // diagnostic build only: stamp buffer of the last pendulum/f64 wg context
#endif
#ifdef CGM_AMAX
unsigned long long* debug_amax_ptr();  // diagnostic build only: rotation increments of the pendulum/f64 row-Newton kernel
#endif
}  // namespace cgm
