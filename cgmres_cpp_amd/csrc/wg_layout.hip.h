// What host and device agree on about the "wg" mapping (tick_wg.hip.h): the kernel-argument struct WgParams, the LDS
// carve-up WgLds and the constants the planner (wg_plan.hip.h) places arrays by.  No kernel code: everything here is
// __host__ __device__, makes no HIP call and is shared by the kernels, the host contexts and the CPU tests of the planner.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/cgmres_hip.h"

namespace cgm {

constexpr int CGM_FUSE_MAX = CGMRES_HIP_TICKS_PER_LAUNCH;
static_assert(CGM_FUSE_MAX == 10, "WgParams::dtau_tab");

enum WgMode { WG_TICK = 0, WG_HOOK_F = 1, WG_HOOK_PREPARE = 2, WG_HOOK_AX = 3, WG_HOOK_GMRES = 4 };

// Plant inputs of one fused launch, indexed like WgParams::ptau_seq with [NX] per instance, by the caller's instance index
// (never by the placement slot): dist = process disturbance d, x_{k+1} = (x_k + f(x_k, u_k) dt) + d_k; meas = measurement
// noise v, the controller is shown y_k = x_k + v_k.  Either may be null.  With meas the TRUE state x_k lives in the
// caller's x buffer (x_in == x_next, written every tick) and the on-chip copy holds y_k.
template <class T>
struct PlantSeqs {
  const T* dist;
  const T* meas;
  size_t dist_tick, meas_tick;  // elements per tick
  int dist_inst, meas_inst;     // elements per instance (0 = one row broadcast to every instance)
};

template <class T>
struct WgParams {
  int B, dv, kmax, L, Lp, Lg, Lv, Pp, Hp, fh_hbm, lds_bytes;  // fh_hbm: F(U,x+hf,t+h) is kept in HBM only (P.Fh), see WgLds
  int wave_dbg;   // wave mapping (tick_wave.hip.h): 1 = Newton with fresh sin/cos, 2 = serial state sweep in every mat-vec
  int cs_chunks;  // chunks of the two-pass costate sweep (WgCtx::sweep_costate_2pass): 3 or 4, what the LDS budget allows
  // row-parallel Newton kernel (WgCtx::NWT = 1): byte offsets, from the start of the workgroup's LDS, of the arrays that hold
  // the tick's base trajectory during the Arnoldi loop (plan_wg, wg_plan.hip.h, places them: in the stage table and in the scratch of
  // the chunk-parallel costate sweep, both idle then, and behind everything else where those do not suffice)
  int base_off[8];
   // Lp/Pp/Hp: odd LDS row pitches (Hp: the COMPACT Hessenberg, column k = rows 0..k at offset k(k+1)/2; h(k+1,k) of the
   // column in progress lives in WgLds::hsub);
   // Lg: global row pitch (multiple of 16); Lv = 16*MAXM (row-parallel Newton kernel: 16*12, stage_own.hip.h): pitch of
   // the Krylov rows (pads kept zero, no guards)
  T h, dt, tol, inv_h, one_m_zh, dtau_h, dtau_0;
  // closed loop on the device: up to CGM_FUSE_MAX consecutive ticks per launch, the controller state (U in LDS, dUdt
  // in registers, x in LDS) carried from tick to tick without going through HBM; dtau_tab[2*k], [2*k+1] = the two
  // horizon steps of tick k (cgmres.hpp:88,91), computed by the host exactly as for single launches
  int n_ticks;
  T dtau_tab[2 * 10];
  // time-varying reference (cgmres_hip_closed_loop_device_ptau): ptau of tick k of this launch =
  // ptau_seq[k*pseq_tick + b*pseq_inst + ...]; null = the handle's ptau for every tick
  const T* ptau_seq;
  size_t pseq_tick;
  int pseq_inst;
  // plant inputs of the fused loop (cgmres_hip_closed_loop_device_ex): null = none.  Behind ONE pointer to a device-resident
  // record, so that the kernels of the default path carry two more scalar registers and nothing else
  const PlantSeqs<T>* pin;
  // instance-major HBM state
  T *U, *dUdt, *Fh, *V, *xdxh, *ptau;  // [B][Lg], [B][Lg], [B][Lg], [B][kmax+1][Lv], [B][NX], [B][NP*(dv+1)]
  T* kry;                              // [B][KS]: H (k1*k1 col-major) | rho (k1) | g (3*kmax)
  T* scr;                              // [workgroups][2][(dv+TAB_PAD)*NSTG*IPW]: parked stage tables of the preamble sweeps
  T* pT;                               // lean plan: [workgroups][(dv+1)*NP][IPW] parameter horizon, transposed
  T* park;                             // [workgroups*IPW][Lv]: the solution vector during the Arnoldi loop (MAXM > 10 only)
  int *n_ax, *reason;
  // Placement: slot q = workgroup*IPW + row of the launch holds instance perm[q] (null = identity).  Instances never
  // exchange data; the closed loop of an oversubscribed batch bins instances by the Arnoldi count of their last tick so
  // that the rows of a workgroup leave the loop together (gmres.hpp:93-95 makes the count data-dependent;
  // util_kernels.hip.h: bin_by_count_kernel, a stable sort: the same counts give the same placement).  Where an
  // instance sits changes its bits in ONE case: the pendulum's quad sweep picks the form of its trig update (rotation /
  // fresh evaluation, sweep_state) per WAVE, i.e. for the 16 instances of a workgroup together, and the two forms round
  // differently (~1e-16) — in fast motion an instance's rounding depends on its workgroup mates.  Everything else of a
  // tick is independent of the placement bit for bit.
  const int* perm;
  const T* x_in;  // [B][NX]
  T* u_out;       // [B][NU]
  T* x_next;      // [B][NX] or null
  // hooks
  int mode;
  const T *hook_in0, *hook_in1;  // instance-major [B][L]
  T* hook_out;
  T hook_dtau;
};

// ---- LDS carve-up -------------------------------------------------------------------------------
// Three plans (WgParams::fh_hbm selects between the first two at run time, LEAN is a kernel template parameter):
//   full    U, F(U,x+hf,t+h) and the work vector W as rows, the stage table, ptau, the small Krylov arrays
//   fh_hbm  the row array of F(U,x+hf,t+h) is left out — the coefficient phase, its only reader after the preamble,
//           takes it from HBM (P.Fh).  Used when that is what lets 16 instances fit (MSD at N = 50: L = 300).
//   lean    only W, the stage table and the small arrays: U lives in the row lanes' REGISTERS (and is published into W
//           for the two unperturbed sweeps of the preamble), F(U,x+hf,t+h) and ptau are read from HBM/L2 by the
//           coefficient phase.  Half the footprint: TWO workgroups share a CU (<= 79.5 KB each), and the hardware
//           places their sweep waves on different SIMDs (tools/ubench_hwid.hip) — the serial phases of 32 instances
//           per CU overlap.  Chosen when a batch needs more workgroups than the GPU has CUs, or when controllers of
//           two models share the GPU (multiple_controller).
enum WgPlan { PLAN_FULL = 0, PLAN_FH_HBM = 1, PLAN_LEAN = 2 };
template <class M, class T, int IPW, int TABX = 0>  // TABX: spare scalars behind every stage of the stage table (WgCtx::NWT)
struct WgLds {
  // stage table: NSTG values per (stage, instance), layout [stage][slot][IPW], dv + TAB_PAD stages
  //   after phase 1: slots 0..NSLOT-1 = x(s), trig(s) (model's slot map);  after phase 2: slots 0..NBW-1 = costate coefficients
  static constexpr int NSTG = M::NSLOT > M::NBW ? M::NSLOT : M::NBW;
  static constexpr int TAB_PAD = M::TAB_PAD;
  T *U, *Fh, *W, *R, *p, *H, *rho, *g, *xs, *xh, *xT, *u0;  // xT: terminal states of the state sweeps in flight
  T* hsub;  // h(k+1,k) of the column in progress, per instance (the compact Hessenberg keeps rows 0..k of column k only)
  T* scan;  // scratch of the chunk-parallel costate sweep (WgCtx::sweep_costate_par), full plans only
  unsigned char* lds0;  // start of the workgroup's LDS (WgParams::base_off)
  int *flag, *reason, *nax, *ksolve;
  int* binst;  // global instance of every row of this workgroup (WgParams::perm applied)
  static __host__ __device__ size_t tab_count(int dv) {
    if constexpr (TABX != 0) return size_t(dv + TAB_PAD) * (NSTG * IPW + TABX);
    return size_t(dv + TAB_PAD) * NSTG * IPW;
  }
  // chunk-parallel costate sweep (WgCtx::sweep_costate_par): dF of the homogeneous lanes for the 3*(dv/4) stages of
  // chunks 1..3, then four boundary records per instance (k = 0..3): [NX*NX transfer matrix, row-major][NX vector]
  // [pad], read with 16-byte loads — SCAN_REC doubles apart so that the 16 instances of a read fall into distinct banks
  // (22 scalars = 44 banks for NX = 4: i*44 mod 64 are 16 distinct multiples of 4)
  static constexpr int SCAN_REC = M::NX * M::NX + M::NX + 2;
  static __host__ __device__ size_t scan_count(int dv) {
    return size_t(3 * (dv >> 2)) * M::NUL * M::NX * IPW + size_t(4) * IPW * SCAN_REC;
  }
  // two-pass costate sweep (WgCtx::sweep_costate_2pass), `chunks` of them: the end value of chunk 0 per instance, then one
  // boundary record per instance for each of the chunks 1 .. chunks-2
  static __host__ __device__ size_t scan2_count(int chunks) {
    return size_t(IPW) * M::NX + size_t(chunks - 2) * IPW * SCAN_REC;
  }
  // The constructor below is the one description of the carve-up: the host sizes the allocation by running it on a
  // made-up base address (extent) for the TABX the kernel is instantiated with.
  struct Extent {
    size_t tab_off, status_end, scan_off;  // bytes from the base: stage table, end of the status words, aligned `scan`
  };
  static Extent extent(int dv, int kmax, int Lp, int Pp, int Hp, int plan) {
    WgParams<T> P{};
    P.dv = dv, P.kmax = kmax, P.Lp = Lp, P.Pp = Pp, P.Hp = Hp;
    unsigned char* const base = reinterpret_cast<unsigned char*>(size_t(1) << 30);  // (never dereferenced)
    const WgLds S(base, P, plan);
    return {size_t(reinterpret_cast<unsigned char*>(S.R) - base), size_t(reinterpret_cast<unsigned char*>(S.binst + IPW) - base),
            size_t(reinterpret_cast<unsigned char*>(S.scan) - base)};
  }
  // bytes up to and including the status words; the + 16 absorbs the 16-byte alignment of `scan`, behind which the planner
  // (wg_plan.hip.h) adds the costate scratch
  static size_t bytes(int dv, int kmax, int Lp, int Pp, int Hp, int plan = PLAN_FULL) {
    return extent(dv, kmax, Lp, Pp, Hp, plan).status_end + 16;
  }
  __host__ __device__ __forceinline__ WgLds(unsigned char* base, const WgParams<T>& P, int plan) {
    T* q = reinterpret_cast<T*>(base);
    lds0 = base;
    const int k1 = P.kmax + 1;
    const bool lean = plan == PLAN_LEAN;
    // The costate sweep's look-ahead reads up to three stages BELOW the start of its operand arrays (values never used):
    // below the stage table that is a row array, below the first row of `out` it is whatever precedes the row arrays.
    // In the full plans U / Fh precede W; in the lean plan W would be the first array of the allocation, so the small
    // per-instance state arrays are placed in front of it (an access below the allocation is an aperture violation).
    if (lean) {
      xs = q, q += M::NX * IPW;
      xh = q, q += M::NX * IPW;
      xT = q, q += 2 * M::NX * IPW;  // lean: two concurrent preamble sweeps
      u0 = q, q += M::NU * IPW;      // lean: the control of the current tick for the plant step
    }
    U = q, q += lean ? 0 : IPW * P.Lp;                 // lean: U aliases W (never dereferenced as U)
    Fh = q, q += plan == PLAN_FULL ? IPW * P.Lp : 0;  // otherwise Fh aliases W (the preamble moves the result to HBM)
    W = q, q += IPW * P.Lp;
    R = q, q += tab_count(P.dv);
    p = q, q += lean ? 0 : IPW * P.Pp;
    H = q, q += IPW * P.Hp;
    rho = q, q += IPW * k1;
    g = q, q += IPW * 3 * P.kmax;
    hsub = q, q += IPW;
    if (!lean) {
      xs = q, q += M::NX * IPW;
      xh = q, q += M::NX * IPW;
      xT = q, q += 3 * M::NX * IPW;  // full plans: three concurrent preamble sweeps
      u0 = q;
    }
    int* z = reinterpret_cast<int*>(q);
    flag = z, reason = z + IPW, nax = z + 2 * IPW, ksolve = z + 3 * IPW, binst = z + 4 * IPW;
    // 16-byte aligned (records are read in pairs) — as an OFFSET from the base: a pointer-integer-pointer round trip
    // loses the LDS address space and every access through `scan` becomes a flat load behind s_waitcnt vmcnt(0)
    const unsigned scan_off = unsigned(reinterpret_cast<unsigned char*>(z + 5 * IPW) - base);
    scan = reinterpret_cast<T*>(base + ((scan_off + 15u) & ~15u));
  }
};

// Row-parallel kernels (WgCtx::NWT != 0): the stage table has NWT_TABX spare scalars per stage so that the 16 lanes of a row,
// which own four consecutive stages each, store into distinct banks.
constexpr int NWT_TABX = 1;
// Row-Newton kernel (WgCtx::NWT = 1): a lane owns WG_ROW_SPL stages (WgCtx::SPL); the tick's base trajectory is held in
// WG_ROW_NBASE arrays (WgCtx::RowBase) of one 16-byte pair per thread and stage pair, which plan_wg places
// (WgParams::base_off).
constexpr int WG_ROW_SPL = 4, WG_ROW_NBASE = 7;
template <class T>
constexpr size_t wg_base_array_bytes(int ipw) {  // one of the WG_ROW_NBASE arrays
  return size_t(WG_ROW_SPL) * ipw * 16 * sizeof(T);
}

}  // namespace cgm
