// CPU probe of the wg planner (csrc/wg_plan.hip.h) and of the LDS carve-up it sizes (WgLds, csrc/wg_layout.hip.h) for USER
// models: plan_wg<UserDev<Model>, double> for the five aliases of tests/user_models/shape_models.hpp, keyed by the
// alias's index in cfg->model_id (0 Shape110, 1 Shape321, 2 Shape262, 3 Shape431, 4 Shape521).  Same entry points as
// tests/plan_probe.hip; built and loaded by tests/plan_probe.py.  UserDev is taken from csrc/user_model.hip.h for its
// traits only: no kernel is instantiated, no context is made and no HIP call is made, so it runs without a GPU.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#pragma clang force_cuda_host_device begin
#include "user_models/shape_models.hpp"
#pragma clang force_cuda_host_device end
#include "../cgmres_cpp_amd/csrc/user_model.hip.h"
#include "../cgmres_cpp_amd/csrc/wg_plan.hip.h"

namespace {
using namespace cgm;

template <class F>
int for_alias(int alias, F&& f) {
  if (alias == 0) return f(UserDev<Shape110>{});
  if (alias == 1) return f(UserDev<Shape321>{});
  if (alias == 2) return f(UserDev<Shape262>{});
  if (alias == 3) return f(UserDev<Shape431>{});
  if (alias == 4) return f(UserDev<Shape521>{});
  return -100;
}

template <class M, int IPW>
void walk(const cgmres_hip_config& c, int plan, long long* out) {
  using T = double;
  using Lds = WgLds<M, T, IPW, 0>;
  WgParams<T> P{};
  P.dv = c.dv, P.kmax = c.k_max, P.Lp = (M::NU * c.dv) | 1, P.Pp = (M::NP * (c.dv + 1)) | 1, P.Hp = WgTraits<M, T>::pitch_H(c.k_max);
  unsigned char* const base = reinterpret_cast<unsigned char*>(size_t(1) << 30);
  const Lds S(base, P, plan);
  const void* ptr[20] = {S.U,    S.Fh, S.W,  S.R,  S.p,    S.H,      S.rho, S.g,      S.hsub,  S.xs,
                         S.xh,   S.xT, S.u0, S.flag, S.reason, S.nax, S.ksolve, S.binst, S.binst + IPW, S.scan};
  for (int i = 0; i < 20; ++i) out[i] = static_cast<const unsigned char*>(ptr[i]) - base;
  out[20] = sizeof(T), out[21] = IPW, out[22] = Lds::NSTG, out[23] = M::NU, out[24] = (long long)(Lds::tab_count(c.dv) * sizeof(T));
  out[25] = (long long)(Lds::scan_count(c.dv) * sizeof(T)), out[26] = (long long)(Lds::scan2_count(3) * sizeof(T));
  out[27] = (long long)(Lds::scan2_count(4) * sizeof(T)), out[28] = M::TAB_PAD, out[29] = NWT_TABX;
  out[30] = 0, out[31] = 0;  // no row-Newton kernel for a user model (HAS_QUAD_SWEEP is false)
  static_assert(!WgTraits<M, T>::kRowNewton && !WgTraits<M, T>::kRowScan, "a row-parallel kernel became reachable for UserDev");
}
}  // namespace

extern "C" {
// as plan_probe.hip's; cfg->dtype must be CGMRES_HIP_F64 (the plugin glue refuses anything else before it plans)
int plan_probe(const cgmres_hip_config* cfg, int cus, long long* out, char* name, char* why) {
  if (cfg->dtype != CGMRES_HIP_F64) return -100;
  return for_alias(cfg->model_id, [&](auto m) {
    using M = decltype(m);
    WgPlanResult r;
    std::string w;
    const int rc = plan_wg<M, double>(*cfg, cus, &r, &w);
    const long long v[14] = {r.k.ipw, r.k.maxm, r.plan, r.k.par, r.cs_chunks, r.k.nwt, r.k.wave, r.variant, (long long)r.lds_bytes,
                             (long long)r.lds_bytes_hook, (long long)r.lds_bytes_tick, r.fh_hbm, r.fh_hbm_hook, r.binning};
    for (int i = 0; i < 14; ++i) out[i] = v[i];
    for (int i = 0; i < 8; ++i) out[14 + i] = r.base_off[i];
    std::strncpy(name, rc ? "" : wg_variant_name(r), 511);
    std::strncpy(why, w.c_str(), 511);
    return rc;
  });
}
int layout_probe(const cgmres_hip_config* cfg, int ipw, int tabx, int plan, long long* out) {
  if (cfg->dtype != CGMRES_HIP_F64 || tabx != 0) return -1;
  return for_alias(cfg->model_id, [&](auto m) {
    using M = decltype(m);
    if (ipw == 16) walk<M, 16>(*cfg, plan, out);
    else if (ipw == 8) walk<M, 8>(*cfg, plan, out);
    else return -1;
    return 0;
  });
}
long long lds_limit(int lean) { return (long long)(lean ? kLdsLimitLean : kLdsLimit); }
// dims of the alias: dim_x, dim_u, dim_p, NSTG, whether WaveOps::FITS holds
int alias_info(int alias, int* out) {
  return for_alias(alias, [&](auto m) {
    using M = decltype(m);
    out[0] = M::NX, out[1] = M::NU, out[2] = M::NP, out[3] = WgLds<M, double, 16>::NSTG, out[4] = WgTraits<M, double>::kWave;
    return 0;
  });
}
}
