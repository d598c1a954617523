// Included by the inst_*.hip translation units only.
#pragma once
#include "ctx_lane.hip.h"
#include "ctx_wg.hip.h"
#include "factory.hip.h"

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
}  // namespace cgm
