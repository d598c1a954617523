// Which kernel of the "wg" family (tick_wg.hip.h, tick_wave.hip.h) a controller batch runs on, with how much LDS and
// where each array sits: plan_wg() decides all of it from the configuration, the CU count of the device and the
// model's compile-time traits.  It makes no HIP call and touches no global state, and it sees no kernel code — only the
// LDS layouts (wg_layout.hip.h, wave_ops.hip.h) and the model traits: tests/test_wg_plan.py runs it on the CPU.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/cgmres_hip.h"
#include "models.hip.h"
#include "tick_common.hip.h"  // DxdtUsesP
#include "wave_ops.hip.h"
#include "wg_layout.hip.h"

namespace cgm {

constexpr size_t kLdsLimit = 160 * 1024 - 1024;  // gfx950: 160 KiB per workgroup, minus the kernels' small static LDS
// Two workgroups share a CU when each allocates at most half of the 160 KiB (measured, tools/ubench_hwid.hip: 81408
// bytes of dynamic LDS co-reside, 81920 do not).
constexpr size_t kLdsLimitLean = 80 * 1024 - 512;

// which instantiation: tick_wg_kernel<M, T, ipw, maxm, lean, PAR, nwt>, or tick_wave_kernel when `wave`.  par is the
// form of the costate sweep whose scratch the plan holds (WgCtx::PAR: 0 serial, 1 LDS scratch, 2 two-pass); the
// row-parallel kernels exist in one form each (nwt = 1: PAR = 1, nwt = 2: PAR = 0) and use that scratch as they like
struct WgKernelId {
  int ipw, maxm;  // 16 or 8 instances per workgroup (0: the wg mapping cannot serve these sizes at all); vectors up to 16 * maxm
  bool lean;
  int par, nwt;
  bool wave;
};
struct WgPlanResult {
  WgKernelId k;
  int plan;                    // PLAN_* of the tick kernel
  int fh_hbm, fh_hbm_hook;     // F(U,x+hf,t+h) in HBM only: tick kernel / white-box hooks (which keep the full or fh_hbm plan)
  int cs_chunks;               // WgParams::cs_chunks (par = 2)
  int base_off[8];             // WgParams::base_off (nwt = 1)
  size_t lds_bytes;            // dynamic LDS of the wg tick kernel (the wg plan of the sizes also when `wave`)
  size_t lds_bytes_hook;       // ... of the hook kernel
  size_t lds_bytes_tick;       // what the tick kernel is launched with: lds_bytes, or the wave kernel's own
  bool binning;                // closed loop: bin the instances by their last Arnoldi count before every launch
  int variant;                 // resolved cgmres_hip_config.variant: 2 | 3 | 4
};

inline const char* wg_variant_name(const WgPlanResult& r) {
  if (r.k.wave) return "wave";
  if (r.k.nwt == 1) return "wg+row-newton";
  if (r.k.nwt == 2) return "wg+row-scan";
  static const char* const names[2][3] = {{"wg", "wg+parallel-costate", "wg+two-pass-costate"},
                                          {"wg-lean", "wg-lean", "wg-lean+two-pass-costate"}};
  return names[r.k.lean][r.k.par];
}

__attribute__((format(printf, 2, 3))) inline int plan_refuse(std::string* why, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (why) *why = buf;
  return CGMRES_HIP_EINVAL;
}

// Compile-time side of the decision: which kernels exist for (M, T).  CtxWg::pick guards its instantiations with these.
template <class M, class T>
struct WgTraits {
  static constexpr bool kF64 = std::is_same<T, double>::value;
  template <class MM, class = void>
  struct RowAffine : std::false_type {};
  template <class MM>
  struct RowAffine<MM, std::void_t<decltype(MM::ROW_AFFINE)>> : std::integral_constant<bool, MM::ROW_AFFINE> {};
  static constexpr bool kRowScan = RowAffine<M>::value && kF64;   // WgCtx::NWT = 2
  static constexpr bool kRowNewton = M::HAS_QUAD_SWEEP && kF64;  // WgCtx::NWT = 1
  // A Newton sweep costs the same whatever the horizon (four stages per lane, lanes beyond the horizon idle), the serial
  // sweep is proportional to it: measured at 4096 controllers, k_max = 10 — dv = 30: 103.6 vs 100.2 us per tick (serial
  // wins), 36: 105.3 vs 109.3, 40: 106.8 vs 114.6, 44: 99.6 vs 115.1, 50: 102.0 vs 125.1; dv = 25, k_max = 5: 59.7 vs 52.3.
  static constexpr int kRowNewtonMinDv = 33;
  // kernels with the chunk-parallel costate sweep: the form with per-stage LDS scratch (WgCtx::sweep_costate_par) exists for
  // the short-vector instantiations, the two-pass form (sweep_costate_2pass) for every 16-instance kernel
  static constexpr bool kPar2 = M::COSTATE_HOM && M::NX * 16 <= 64 && M::NX % 2 == 0;
  template <int MAXM>
  static constexpr bool kParCostate = kPar2 && MAXM == 10;
  // the wave mapping (tick_wave.hip.h).  User models (WaveOps<UserDev<Model>>): fp64, dim_x <= kUserWaveMaxNx,
  // dim_u <= kUserWaveMaxNu, and only on request (the library's choice never takes them)
  static constexpr int kWaveKmax = 10, kWaveWpb = 1;
  template <class MM, class = void>
  struct WaveFits : std::true_type {};
  template <class MM>
  struct WaveFits<MM, std::void_t<decltype(WaveOps<MM>::FITS)>> : std::integral_constant<bool, WaveOps<MM>::FITS> {};
  static constexpr bool kWave = WaveOps<M>::value && kF64 && WaveFits<M>::value;
  static constexpr bool kWaveDefault = kWave && !WaveSerialState<M>::value;
  static bool wave_supported(const cgmres_hip_config& c) {
    return kWave && c.dv >= 1 && c.dv <= 63 && c.k_max >= 1 && c.k_max <= kWaveKmax;
  }
  static size_t wave_lds_bytes(const cgmres_hip_config& c) {
    if constexpr (kWave) return WaveLds<M, T>::bytes(c.dv, c.k_max, kWaveWpb);
    return 0;
  }
  static int pitch_H(int k_max) { return ((k_max * (k_max + 1)) / 2 + 2) | 1; }  // (+2: hess_column's look-ahead past the last column)
  // scalars of one workgroup's slot in WgParams::scr: two parked stage tables of the widest kernel of that ipw
  static size_t scr_count(int ipw, int dv) {
    return 2 * (ipw == 16 ? WgLds<M, T, 16, NWT_TABX>::tab_count(dv) : WgLds<M, T, 8, NWT_TABX>::tab_count(dv));
  }
  // The costate sweep's look-ahead (WgCtx::costate_run) requests the coefficients of up to THREE stages below the first
  // stage of its range (the tail of the chunk-parallel form: `post` = 5) and the output words of those stages; the
  // values are never used, but the addresses must stay inside the workgroup's LDS allocation (an access outside it is
  // an aperture violation on this platform).  Below the stage table sit `rows` row arrays of pitch Lp (+ `front` small
  // words per instance in the lean plan): they must cover 3 stages of the table (3*NSTG words per instance, + the pair
  // offset), and the arrays in front of the first `out` row must cover 3*NU words.  Built-in models (NSTG <= 6) pass
  // from dv = 5 (lean) / any dv (full plans); a user model with many stage coefficients and a short horizon
  // (NX = 4, NU = 1: NSTG = 24, Lp = dv|1) does not — it then runs on the lane mapping.
  static bool lookahead_fits(int rows, int Lp, int front_words_per_inst) {
    constexpr int NSTG = WgLds<M, T, 16>::NSTG;
    return rows * Lp + front_words_per_inst >= 3 * NSTG + 2 && (rows - 1) * Lp + front_words_per_inst >= 3 * M::NU;
  }
};

// 0 and *out filled, or CGMRES_HIP_EINVAL and *why; out->k.ipw != 0 tells that the wg mapping can serve the sizes at all
// (what the library's choice between the lane and the wg mapping goes by).  Reads model_id-independent fields only:
// batch, dv, k_max, variant, flags, and tol (for `binning`).
template <class M, class T>
int plan_wg(const cgmres_hip_config& cfg, int cus, WgPlanResult* out, std::string* why) {
  using Tr = WgTraits<M, T>;
  using Lds16 = WgLds<M, T, 16>;
  WgPlanResult& r = *out;
  r = WgPlanResult{};
  const int L = M::NU * cfg.dv, Lp = L | 1, Pp = (M::NP * (cfg.dv + 1)) | 1, Hp = Tr::pitch_H(cfg.k_max);
  const bool big = L > 160;  // the long-vector kernels (MAXM = 20)

  // 1. Instances per workgroup and where F(U,x+hf,t+h) lives.  Preference: 16 instances with everything in LDS; 16 with
  //    F(U,x+hf,t+h) in HBM (long vectors only: the MAXM = 20 kernels are the ones that carry this mode); 8 instances.
  if (L > 320) return plan_refuse(why, "wg mapping: dim_u*dv = %d / LDS footprint not supported", L);
  {
    const size_t b16 = Lds16::bytes(cfg.dv, cfg.k_max, Lp, Pp, Hp), b16h = Lds16::bytes(cfg.dv, cfg.k_max, Lp, Pp, Hp, PLAN_FH_HBM);
    const size_t b8 = WgLds<M, T, 8>::bytes(cfg.dv, cfg.k_max, Lp, Pp, Hp);
    const bool full_ok = Tr::lookahead_fits(3, Lp, 0), fh_ok = Tr::lookahead_fits(2, Lp, 0);  // row arrays in front of the table
    const bool ok8 = b8 <= kLdsLimit && full_ok;
    if ((cfg.flags & CGMRES_HIP_FLAG_IPW8) && ok8) r.k.ipw = 8, r.lds_bytes = b8;
    else if (b16 <= kLdsLimit && full_ok) r.k.ipw = 16, r.lds_bytes = b16;
    else if (big && b16h <= kLdsLimit && fh_ok) r.k.ipw = 16, r.lds_bytes = b16h, r.fh_hbm = 1;
    else if (ok8) r.k.ipw = 8, r.lds_bytes = b8;
    else return plan_refuse(why, "wg mapping: dim_u*dv = %d / LDS footprint not supported", L);
  }
  const bool w16 = r.k.ipw == 16;
  r.k.maxm = big ? 20 : 10;
  r.plan = r.fh_hbm ? PLAN_FH_HBM : PLAN_FULL;
  r.lds_bytes_hook = r.lds_bytes, r.fh_hbm_hook = r.fh_hbm;  // the white-box hooks always run on this plan

  // 2. Lean plan: 16 instances per workgroup in at most half a CU's LDS (W is its only row array, see WgLds; a state
  //    equation that reads p wants the horizon in LDS).  variant 3 asks for it; the default takes it when the batch needs
  //    more 16-instance workgroups than the GPU has CUs (two workgroups per CU then run their serial phases side by side
  //    instead of in two rounds).
  const size_t lean_bytes = Lds16::bytes(cfg.dv, cfg.k_max, Lp, Pp, Hp, PLAN_LEAN);
  const bool lean_ok = w16 && !DxdtUsesP<M, T>::value && Tr::lookahead_fits(1, Lp, 4 * M::NX + M::NU) && lean_bytes <= kLdsLimitLean;
  if (cfg.variant == 3 && !lean_ok)
    return plan_refuse(why, "wg-lean mapping: LDS footprint of dim_u*dv = %d, k_max = %d not supported", L, cfg.k_max);
  r.k.lean = cfg.variant == 3 || (cfg.variant == 0 && lean_ok && (cfg.batch + 15) / 16 > cus);
  if (r.k.lean) r.plan = PLAN_LEAN, r.fh_hbm = 0, r.lds_bytes = lean_bytes;

  // 3. The latency mapping: asked for, or (library's choice) up to two controllers per SIMD.  One wave per SIMD runs a
  //    tick in ~43 us (wg: ~117 us whatever the batch); the kernel takes all 512 registers, so a batch beyond one
  //    controller per SIMD runs in rounds: two rounds (~88 us) still beat the wg mapping, three do not.  The handle
  //    stays a wg context of the same sizes (HBM state, white-box hooks), so everything below is decided for it too.
  if (cfg.variant == 4 && !Tr::wave_supported(cfg)) {
    if (WaveSerialState<M>::value)
      return plan_refuse(why,
                         "wave mapping for a user model: needs dim_x <= %d (has %d), dim_u <= %d (has %d), 1 <= dv <= 63 "
                         "(has %d), 1 <= k_max <= %d (has %d)",
                         kUserWaveMaxNx, M::NX, kUserWaveMaxNu, M::NU, cfg.dv, Tr::kWaveKmax, cfg.k_max);
    return plan_refuse(why, "wave mapping: model / dtype / dv = %d / k_max = %d not supported", cfg.dv, cfg.k_max);
  }
  r.k.wave = cfg.variant == 4 || (cfg.variant == 0 && Tr::kWaveDefault && Tr::wave_supported(cfg) && cfg.batch <= 8 * cus &&
                                  !(cfg.flags & CGMRES_HIP_FLAG_NO_WAVE));
  r.variant = r.k.wave ? 4 : (r.k.lean ? 3 : 2);

  // 4. Costate sweep.  Chunk-parallel with per-stage LDS scratch (WgCtx::sweep_costate_par): its own kernel instantiation on
  //    the full plan, taken when its scratch fits as well; otherwise the two-pass form: 4 chunks where their boundary
  //    records fit behind the plan's arrays, 3 otherwise (the lean plans).  (The white-box hooks keep the serial sweep.)
  const bool serial = cfg.flags & CGMRES_HIP_FLAG_SERIAL_COSTATE, two_pass = cfg.flags & CGMRES_HIP_FLAG_TWO_PASS_COSTATE;
  size_t scratch = 0;  // bytes of costate scratch behind the aligned `scan` pointer
  if (Tr::template kParCostate<10> && w16 && !big && !r.k.lean && cfg.dv >= 4 && !serial && !two_pass &&
      r.lds_bytes + Lds16::scan_count(cfg.dv) * sizeof(T) + 16 <= kLdsLimit)
    r.k.par = 1, scratch = Lds16::scan_count(cfg.dv) * sizeof(T);
  for (int chunks = 4; Tr::kPar2 && w16 && !serial && r.k.par == 0 && chunks >= 3; --chunks)
    if (cfg.dv >= 2 * chunks && r.lds_bytes + Lds16::scan2_count(chunks) * sizeof(T) + 16 <= (r.k.lean ? kLdsLimitLean : kLdsLimit))
      r.k.par = 2, r.cs_chunks = chunks, scratch = Lds16::scan2_count(chunks) * sizeof(T);
  if (scratch) r.lds_bytes += scratch + 16;

  // 5. Row-parallel sweeps in the Arnoldi loop (WgCtx::NWT): the full plan's 16-instance short-vector kernel, fp64.  (A
  //    flag that asks for a particular costate sweep asks for the kernel that has one.)  Their stage table has NWT_TABX
  //    spare scalars per stage, which moves everything behind it: the layout is WgLds<.., NWT_TABX>'s.
  if constexpr (Tr::kRowScan || Tr::kRowNewton)
  if (!(cfg.flags & CGMRES_HIP_FLAG_SERIAL_STATE_SWEEP) && !serial && !two_pass && !r.k.wave && w16 && !big && !r.k.lean &&
      !r.fh_hbm && cfg.dv <= 63 && cfg.k_max <= 12) {
    using LdsX = WgLds<M, T, 16, NWT_TABX>;
    const size_t bytes_x = LdsX::bytes(cfg.dv, cfg.k_max, Lp, Pp, Hp) + (scratch ? scratch + 16 : 0);
    if constexpr (Tr::kRowScan) {
      // a state equation that is affine in x: plain scans, no Newton
      if (bytes_x <= kLdsLimit) r.k.nwt = 2, r.lds_bytes = bytes_x;
    }
    if constexpr (Tr::kRowNewton) {
      // Newton state sweeps.  The base trajectory (WG_ROW_NBASE arrays of 8 KB) goes where LDS is idle during the Arnoldi
      // loop — the stage table, the scratch of the costate scan — and behind everything else for the rest; the kernel is
      // taken when all of that fits.
      const typename LdsX::Extent e = LdsX::extent(cfg.dv, cfg.k_max, Lp, Pp, Hp, PLAN_FULL);
      const size_t arr = wg_base_array_bytes<T>(16), tab_cap = LdsX::tab_count(cfg.dv) * sizeof(T);
      size_t end = (bytes_x + 15) & ~size_t(15), in_tab = 0, in_scan = 0;
      int off[WG_ROW_NBASE];
      for (int k = 0; k < WG_ROW_NBASE; ++k) {
        if ((in_tab + 1) * arr <= tab_cap) off[k] = int(e.tab_off + in_tab++ * arr);
        else if ((in_scan + 1) * arr <= scratch) off[k] = int(e.scan_off + in_scan++ * arr);
        else off[k] = int(end), end += arr;
      }
      if (cfg.dv >= Tr::kRowNewtonMinDv && end <= kLdsLimit) {
        r.k.nwt = 1, r.lds_bytes = end;
        for (int k = 0; k < WG_ROW_NBASE; ++k) r.base_off[k] = off[k];
      }
    }
  }
  r.lds_bytes_tick = r.k.wave ? Tr::wave_lds_bytes(cfg) : r.lds_bytes;

  // 6. Binning pays only when the batch needs more workgroups than the GPU holds at once (then the device works through
  //    a queue of workgroups and the sum of their times counts); with every workgroup resident the launch lasts as long
  //    as its slowest workgroup wherever the instances sit.  Early exits need tol > 0.
  r.binning = !r.k.wave && cfg.tol > 0 && !(cfg.flags & CGMRES_HIP_FLAG_NO_BINNING) &&
              (cfg.batch + r.k.ipw - 1) / r.k.ipw > cus * (r.k.lean ? 2 : 1);
  return 0;
}

}  // namespace cgm
