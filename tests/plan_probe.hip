// CPU probe of the wg planner (csrc/wg_plan.hip.h) and of the LDS carve-up it sizes (WgLds, csrc/wg_layout.hip.h) for the
// six built-in (model, dtype) pairs; built and loaded by tests/plan_probe.py.  No kernel is instantiated and no HIP
// call is made: it runs on a machine without a GPU.
#include <cstring>

#include "../cgmres_cpp_amd/csrc/wg_plan.hip.h"

namespace {
using namespace cgm;

template <class M_, class T_>
struct Pair {
  using M = M_;
  using T = T_;
};
template <class F>
int for_pair(int model, int dtype, F&& f) {
  const int key = model * 2 + dtype;
  if (key == 0) return f(Pair<PendulumDev<double>, double>{});
  if (key == 1) return f(Pair<PendulumDev<float>, float>{});
  if (key == 2) return f(Pair<MsdDev<double>, double>{});
  if (key == 3) return f(Pair<MsdDev<float>, float>{});
  if (key == 4) return f(Pair<SemiactiveDev<double>, double>{});
  if (key == 5) return f(Pair<SemiactiveDev<float>, float>{});
  return -100;
}

template <class M, class T, int IPW, int TABX>
void walk(const cgmres_hip_config& c, int plan, long long* out) {
  using Lds = WgLds<M, T, IPW, TABX>;
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
  out[30] = 0, out[31] = 0;
  if constexpr (WgTraits<M, T>::kRowNewton) out[30] = (long long)wg_base_array_bytes<T>(16), out[31] = WG_ROW_NBASE;
}
}  // namespace

extern "C" {
// out: ipw, maxm, plan, par, cs_chunks, nwt, wave, variant, lds_bytes, lds_bytes_hook, lds_bytes_tick, fh_hbm, fh_hbm_hook,
// binning, base_off[8]; name / why: at least 512 bytes each.  Returns plan_wg's return value.
int plan_probe(const cgmres_hip_config* cfg, int cus, long long* out, char* name, char* why) {
  return for_pair(cfg->model_id, cfg->dtype, [&](auto pair) {
    using P = decltype(pair);
    WgPlanResult r;
    std::string w;
    const int rc = plan_wg<typename P::M, typename P::T>(*cfg, cus, &r, &w);
    const long long v[14] = {r.k.ipw, r.k.maxm, r.plan, r.k.par, r.cs_chunks, r.k.nwt, r.k.wave, r.variant, (long long)r.lds_bytes,
                             (long long)r.lds_bytes_hook, (long long)r.lds_bytes_tick, r.fh_hbm, r.fh_hbm_hook, r.binning};
    for (int i = 0; i < 14; ++i) out[i] = v[i];
    for (int i = 0; i < 8; ++i) out[14 + i] = r.base_off[i];
    std::strncpy(name, rc ? "" : wg_variant_name(r), 511);
    std::strncpy(why, w.c_str(), 511);
    return rc;
  });
}
// Byte offsets of the arrays of WgLds<M, T, ipw, tabx> on PLAN_* `plan`, in the constructor's own order: U Fh W R p H rho g
// hsub xs xh xT u0 flag reason nax ksolve binst, the end of binst, scan; then [20..31] sizeof(T), ipw, NSTG, NU, bytes of the
// stage table, of the LDS-scratch costate form, of the two-pass records (3, 4 chunks), TAB_PAD, NWT_TABX, bytes of one
// row-Newton base array and their number (0 where the model has no such kernel).
int layout_probe(const cgmres_hip_config* cfg, int ipw, int tabx, int plan, long long* out) {
  return for_pair(cfg->model_id, cfg->dtype, [&](auto pair) {
    using M = typename decltype(pair)::M;
    using T = typename decltype(pair)::T;
    if (ipw == 16 && tabx == 0) walk<M, T, 16, 0>(*cfg, plan, out);
    else if (ipw == 16 && tabx == NWT_TABX) walk<M, T, 16, NWT_TABX>(*cfg, plan, out);
    else if (ipw == 8 && tabx == 0) walk<M, T, 8, 0>(*cfg, plan, out);
    else return -1;
    return 0;
  });
}
long long lds_limit(int lean) { return (long long)(lean ? kLdsLimitLean : kLdsLimit); }
}
