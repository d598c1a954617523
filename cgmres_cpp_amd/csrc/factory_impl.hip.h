// Included by the inst_*.hip translation units only.
#pragma once
#include "ctx_lane.hip.h"
#include "ctx_wg.hip.h"
#include "factory.hip.h"
#include "plant.hip.h"

namespace cgm {
template <class M, class T>
cgmres_hip_ctx* make_variant(const cgmres_hip_config& cfg, int* resolved) {
  WgPlanResult plan;
  plan_wg<M, T>(cfg, 0, &plan, nullptr);
  const bool wg_ok = plan.k.ipw != 0;  // (the sizes fit an LDS plan of the wg mapping; what else was asked for is init's to refuse)
  const int v = cfg.variant == 0 ? (wg_ok ? 2 : 1) : cfg.variant;
  *resolved = v;
  if (v == 2 || v == 3 || v == 4) return wg_ok ? new CtxWg<M, T>() : nullptr;  // (CtxWg::init picks / checks the LDS plan: 2 or 3)
  return new CtxLane<M, T>();
}
// cgmres_hip_horizon_device on a context make_variant<M, T> made: who made it knows its concrete type — the resolved
// variant 1 is CtxLane, everything else CtxWg — and CtxHost::horizon is no virtual
template <class M, class T>
int horizon_variant(cgmres_hip_ctx* c, const void* x_dev, const cgmres_hip_horizon_out* out) {
  if (c->cfg.variant == 1) return static_cast<CtxLane<M, T>*>(c)->horizon(x_dev, out);
  return static_cast<CtxWg<M, T>*>(c)->horizon(x_dev, out);
}
// One launch of plant_kernel<M, T> (plant.hip.h) on the stream of a context make_variant<M, T> made.  A call without p
// (cgmres_hip_plant_step_device) takes stage 0 of the handle's ptau, in the layout of the concrete context.
template <class M, class T>
int plant_variant(cgmres_hip_ctx* c, const PlantCall& call) {
  PlantArgs<T> A{};
  A.B = c->cfg.batch, A.steps = call.substeps, A.rk4 = call.integrator == CGMRES_HIP_PLANT_RK4;
  A.hh = call.substeps > 0 ? T(c->cfg.dt) / T(call.substeps) : T(0);
  A.x = static_cast<T*>(call.x), A.u = static_cast<const T*>(call.u);
  A.theta = static_cast<const T*>(call.theta), A.theta_inst = call.theta_inst;
  A.p = static_cast<const T*>(call.p), A.p_inst = call.p_inst, A.p_elem = call.p_elem;
  if (!A.p) {
    HorizonView<const T> U{}, ptau{};
    int rows = 0;
    if (c->cfg.variant == 1)
      static_cast<CtxLane<M, T>*>(c)->horizon_views(&U, &ptau, &rows);
    else
      static_cast<CtxWg<M, T>*>(c)->horizon_views(&U, &ptau, &rows);
    A.p = ptau.p, A.p_inst = ptau.sb, A.p_elem = ptau.se;
  }
  A.d = static_cast<const T*>(call.d), A.d_inst = call.d_inst;
  A.v = static_cast<const T*>(call.v), A.v_inst = call.v_inst;
  A.y = static_cast<T*>(call.y);
  plant_kernel<M, T><<<dim3((c->cfg.batch + kPlantBlock - 1) / kPlantBlock), kPlantBlock, 0, c->stream>>>(A);
  HIP_TRY(hipGetLastError());
  return 0;
}
}  // namespace cgm
