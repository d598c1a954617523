// Variants 2 and 3 ("wg", "wg-lean"): one workgroup owns IPW controller instances for a whole control tick.
//
// Mapping (gfx950, wave64):
//   * block = IPW*16 threads; thread (inst = tid/16, r = tid%16).  The 16 lanes of one DPP row own the
//     length-L vectors of one instance, lane r holding elements e = r + 16*m (m < MAXM) in registers.
//     Dot products / norms are lane partial sums + a 4-step DPP butterfly inside the row
//     (quad_perm, quad_perm, row_half_mirror, row_mirror): every lane of the row ends with the
//     bit-identical sum, so row-uniform branches (early exit, breakdown) never diverge inside a row.
//   * a horizon sweep (F_func, cgmres.hpp:113-162) has three phases:
//       1. state sweep  — serial in the stage index, on wave 0: four lanes (one DPP quad) per instance for the
//                         pendulum (PendulumDev::quad_stage), one lane per instance otherwise; x(s) and the
//                         reusable trig values go to the LDS stage table R;
//       2. coefficients — everything of the backward stage that does not involve the costate (dHdx and dHdu
//                         are affine in it, models.hip.h) for ALL (stage, instance) pairs at once; inside the
//                         Arnoldi loop waves 1..3 do this chunk by chunk BEHIND the state sweep (f_eval);
//       3. costate sweep — serial again, but only the short affine recurrence is left (pendulum: 12 fp64 ops
//                         per stage instead of 46), fused with the costate part of dH/du.
//     U, F(U,x+hf,t+h), the work vector, the stage table and ptau all sit in LDS (odd row pitches: conflict-free
//     for the sweep lanes); there is no HBM access inside the stage loops.  (Long vectors: WgParams::fh_hbm.)
//   * the Krylov basis V (IPW x (k_max+1) x L) does not fit in 160 KB of LDS at IPW = 16, it lives in
//     HBM/L2 as zero-padded, pair-interleaved rows of 16*MAXM scalars (16-byte accesses, no guards) and is
//     streamed once per Gram-Schmidt step through a register ring — the traffic SURVEY.md §8(d) prices.
//   * the serial phases run on ONE wave, which issues one instruction of any kind per ~4.4 cycles
//     (tools/ubench_issue.hip): the stage loops are written for instruction count.
//   * instances never exchange data: the only synchronisation is the workgroup barrier between phases.
//   * variant 3 ("wg-lean", template parameter LEAN): the same kernel on half the LDS — U in the row lanes' registers (or
//     re-read from its HBM row), F(U,x+hf,t+h) and ptau fetched from HBM/L2 a group of items ahead — so that two
//     workgroups share a CU and their serial phases run side by side on different SIMDs (WgLds).
//   * inside a chunk of stages the pendulum sweep advances its sin/cos values by rotation through the exact angle
//     increment instead of re-evaluating them (PendulumDev::quad_stage_rot), with per-chunk fallbacks; in fixed-k mode
//     (tol = 0) the Hessenberg column of an iteration is processed by an idle wave during the next sweep (gmres()).
//   * template parameter NWT = 1 (pendulum fp64, full plan; the library's choice for the headline batch): inside the
//     Arnoldi loop the three phases above give way to ROW-PARALLEL sweeps — every row of 16 lanes runs its instance's
//     state recurrence as Newton's method on the whole trajectory (four stages per lane, in-row DPP scans) and the
//     costate recurrence as three scans down the row, all in registers, with no workgroup barrier in the loop
//     (row_newton_sweep / row_costate); the serial state sweep remains in the preamble only.  This kernel
//     holds its solver vectors in STAGE OWNERSHIP (stage_own.hip.h: lane r has the 12 elements of its own four stages
//     instead of r + 16 m), so the sweeps take the direction from and leave the result in the registers of the vector
//     algebra: no work vector W, no row arrays U / Fh — their storage holds lane-private arrays of the owned stages.
//     NWT = 2 (a state equation affine in x: the semi-active damper): the same with plain scans — no Newton, no serial
//     sweep and no stage table anywhere in the tick (row_affine_sweep).
// Statement order inside each instance follows cgmres.hpp:78-175 / gmres.hpp:28-112; what differs from the
// reference is the association order of sums (16 partial sums + butterfly; affine regrouping of the costate step).
#pragma once
#include "wg_ctx.hip.h"
#include "wg_gmres.hip.h"
#include "wg_sweep_rows.hip.h"
#include "wg_sweep_serial.hip.h"

namespace cgm {

// the one-thread kernel that fills the device-resident record behind WgParams::pin
template <class T>
__global__ void set_plant_seqs_kernel(PlantSeqs<T>* dst, PlantSeqs<T> v) {
  *dst = v;
}

// ---- the tick kernel: cgmres.hpp:78-110 for IPW instances ----------------------------------------
template <class M, class T, int IPW, int MAXM, bool LEAN = false, int PAR = 0, int NWT = 0>
__global__ __launch_bounds__(IPW * 16) __attribute__((amdgpu_waves_per_eu(LEAN ? 2 : 1, LEAN ? 2 : 1))) void tick_wg_kernel(
    WgParams<T> P) {
  extern __shared__ __align__(16) unsigned char smem[];
  WgCtx<M, T, IPW, MAXM, LEAN, PAR, NWT> C(P, smem);
  using Ctx = decltype(C);
  constexpr bool SO = Ctx::ROW_NEWTON;  // solver vectors in stage ownership (stage_own.hip.h)
  constexpr int NVEC = Ctx::NVEC;
  T du[NVEC], bb[NVEC];
  C.load_common(P.U);
  if constexpr (SO)
    C.so_load_row(du, P.dUdt);
  else
    C.load_row_to_reg(du, P.dUdt, P.Lg);
  const int nt = P.n_ticks;
  for (int tk = 0; tk < nt; ++tk) {
    const bool last = tk + 1 == nt;
    C.dtau_h = P.dtau_tab[2 * tk], C.dtau_0 = P.dtau_tab[2 * tk + 1];
    // H region zeroed so the exported Hessenberg has no stale entries
    for (int q = C.r; q < P.Hp; q += 16) C.S.H[C.inst * P.Hp + q] = T(0);
    if (M::NP > 0 && P.ptau_seq) C.load_ptau_tick(P.ptau_seq + size_t(tk) * P.pseq_tick);
    __syncthreads();  // (also drains the prologue's / load_ptau_tick's HBM stores of the lean parameter table)
    CGM_STAMP(C, 0);
    if constexpr (!LEAN && !SO) C.publish_direction(du);  // direction of the first mat-vec: x0 = dUdt (warm start, cgmres.hpp:99)
    T ax0[NVEC];
    if constexpr (NWT == 2) {
      C.preamble_affine(bb, ax0);
    } else if constexpr (NWT == 1) {
      C.preamble_rows(bb, ax0, du);
      C.store_base();
    } else {
      C.template preamble<true>(bb, ax0, du);  // Fh in LDS (or HBM); b and A*dUdt in registers
    }
    CGM_STAMP(C, 1);
    C.gmres(du, bb, ax0);
    CGM_STAMP(C, 12);
    // U += dUdt*dt, u = U[0:dim_u]  (cgmres.hpp:102-109)
    T un[NVEC];
    if constexpr (SO) {
      C.so_load(0, un, C.tid);  // (lanes without a stage hold another lane's words here: never stored)
    } else if constexpr (LEAN) {
      C.get_urow(un);
    } else {
      C.lds_to_reg(un, C.S.U);
    }
#pragma unroll
    for (int m = 0; m < NVEC; ++m) un[m] = un[m] + du[m] * P.dt;
    constexpr bool U_ROW_IS_HBM = LEAN && !decltype(C)::U_IN_REGS;  // then every tick writes its U row
    if constexpr (SO) {
      if (last) {
        C.so_store_row(P.U, un);
        C.so_store_row(P.dUdt, du);
        if (C.valid && C.r == 0) {  // u = the controls of stage 0: slots 0 .. NU-1 of lane 0
#pragma unroll
          for (int j = 0; j < M::NU; ++j) P.u_out[size_t(C.b) * M::NU + j] = un[j];
        }
      }
    } else {
      if (last || U_ROW_IS_HBM) C.reg_to_row(P.U, P.Lg, un);
    }
    if (last) {  // the rest of the controller state goes back to HBM with the last tick of the launch only
      if constexpr (!SO) {
        C.reg_to_row(P.dUdt, P.Lg, du);
        if (C.valid && C.r < M::NU) P.u_out[size_t(C.b) * M::NU + C.r] = un[0];  // element e = r (m = 0), r < NU <= 16
      }
      C.store_status();
      // x_dxh and F_dxh_h of this tick stay with the controller like the reference's members (cgmres.hpp:198-201):
      // a white-box Ax_func after control() evaluates with them (with fh_hbm the preamble has stored the row already)
      if constexpr (SO) {
        T fh[NVEC];
        C.so_load(1, fh, C.tid);
        C.so_store_row(P.Fh, fh);
      } else if (!C.fh_hbm()) {
        T fh[MAXM];
        C.lds_to_reg(fh, C.S.Fh);
        C.reg_to_row(P.Fh, P.Lg, fh);
      }
      if (C.valid && C.r < M::NX) P.xdxh[size_t(C.b) * M::NX + C.r] = C.S.xh[C.r * IPW + C.inst];
    }
    // the plant step and the next tick read the new U: from LDS, or (lean) from the row registers + a small u array
    if constexpr (LEAN) {
      if constexpr (decltype(C)::U_IN_REGS) {
#pragma unroll
        for (int m = 0; m < MAXM; ++m) C.ureg[m] = un[m];
      }
      if (C.valid && C.r < M::NU) C.S.u0[C.r * IPW + C.inst] = un[0];
    } else if constexpr (SO) {
      if (C.valid) C.so_put_U(un);
    } else {
      C.reg_to_lds(C.S.U, un);
    }
    if (P.x_next) {  // plant step of the example main loop (<example>/main.cpp:71-73)
      __syncthreads();
      // Plant inputs of cgmres_hip_closed_loop_device_ex (d, v): two cold blocks around the plant step, which itself stays
      // statement for statement what it is without them.  They talk to it through S.xs alone, each sweep lane reading
      // back what it wrote itself, so that a kernel that is given neither input keeps (within a few registers,
      // tools/isa_summary.py) the allocation it has without the feature.  A shared block with selects did not.
      const bool inputs = __builtin_expect(P.pin != nullptr, 0) && C.sweep_lane;
      if (inputs && P.pin->meas) {
        // S.xs holds y = x + v: the plant moves the TRUE state, which is in the caller's buffer, last written by this lane
        const T* xt = P.x_next + size_t(C.bi) * M::NX;
#pragma unroll
        for (int c = 0; c < M::NX; ++c) C.S.xs[c * IPW + C.tid] = xt[c];
      }
      if (C.sweep_lane) {
        const int i = C.tid;
        T x[M::NX], u[M::NU], f[M::NX], tr[M::NC > 0 ? M::NC : 1];
#pragma unroll
        for (int c = 0; c < M::NX; ++c) x[c] = C.S.xs[c * IPW + i];
#pragma unroll
        for (int j = 0; j < M::NU; ++j) u[j] = LEAN ? C.S.u0[j * IPW + i] : (SO ? C.so_unow()[j * IPW + i] : C.S.U[i * P.Lp + j]);
        C.model_dxdt(f, x, u, tr, i, 0);  // the example's plant = the model's own state equation (p of stage 0)
#pragma unroll
        for (int c = 0; c < M::NX; ++c) {
          const T xn = x[c] + f[c] * P.dt;
          if (last) P.x_next[size_t(C.bi) * M::NX + c] = xn;
          C.S.xs[c * IPW + i] = xn;
        }
      }
      if (inputs) {  // x_{k+1} = (x_k + f dt) + d_k, kept in the caller's buffer every tick when v is given; S.xs = x_{k+1} + v_{k+1}
        const int i = C.tid;
        const PlantSeqs<T> q = *P.pin;
        const T* dk = q.dist ? q.dist + size_t(tk) * q.dist_tick + size_t(C.bi) * q.dist_inst : nullptr;
        const T* vk = q.meas && !last ? q.meas + size_t(tk + 1) * q.meas_tick + size_t(C.bi) * q.meas_inst : nullptr;
#pragma unroll
        for (int c = 0; c < M::NX; ++c) {
          T xn = C.S.xs[c * IPW + i];
          if (dk) xn = xn + dk[c];
          if (last || q.meas) P.x_next[size_t(C.bi) * M::NX + c] = xn;
          if (vk) xn = xn + vk[c];
          C.S.xs[c * IPW + i] = xn;  // what the next tick's controller sees
        }
      }
    }
    if (!last) {
      if (C.r == 0) C.S.flag[C.inst] = 0, C.S.reason[C.inst] = 0, C.S.nax[C.inst] = 0, C.S.ksolve[C.inst] = 0;
      __syncthreads();  // U, x and the cleared status words are in place for the next tick
    }
  }
  CGM_STAMP(C, 13);
#ifdef CGM_STAMPS
  cgm_stamp_flush();
#endif
}

// ---- white-box hooks on the same device code -------------------------------------------------------
template <class M, class T, int IPW, int MAXM>
__global__ __launch_bounds__(IPW * 16) __attribute__((amdgpu_waves_per_eu(1, 1))) void hook_wg_kernel(WgParams<T> P) {
  extern __shared__ __align__(16) unsigned char smem[];
  WgCtx<M, T, IPW, MAXM> C(P, smem);
  T a[MAXM], c2[MAXM];
  const size_t Lrow = P.L;
  auto load_im = [&](T* reg, const T* src) {  // instance-major [B][L] (no padding) -> registers
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
      const int e = C.elem(m);
      reg[m] = (C.valid && e < P.L) ? src[size_t(C.b) * Lrow + e] : T(0);
    }
  };
  auto store_im = [&](T* dst, const T* reg) {
    if (!C.valid) return;
#pragma unroll
    for (int m = 0; m < MAXM; ++m) {
      const int e = C.elem(m);
      if (e < P.L) dst[size_t(C.b) * Lrow + e] = reg[m];
    }
  };
  if (P.mode == WG_HOOK_F) {  // F_func(ret, U, x, t)
    C.load_common(P.U);
    __syncthreads();
    load_im(a, P.hook_in0);
    C.reg_to_lds(C.S.U, a);
    __syncthreads();
    C.template f_eval<false, F_PLAIN>(C.S.xs, P.hook_dtau, C.S.W, false);
    __syncthreads();
    C.lds_to_reg(a, C.S.W);
    store_im(P.hook_out, a);
    return;
  }
  if (P.mode == WG_HOOK_PREPARE) {  // cgmres.hpp:83-96
    C.load_common(P.U);
    __syncthreads();
    C.template preamble<false>(a, c2);
    if (P.hook_out) store_im(P.hook_out, a);
    if (!C.fh_hbm()) {  // (with fh_hbm the preamble has already stored the row)
      C.lds_to_reg(a, C.S.Fh);
      C.reg_to_row(P.Fh, P.Lg, a);
    }
    if (C.valid && C.r < M::NX) P.xdxh[size_t(C.b) * M::NX + C.r] = C.S.xh[C.r * IPW + C.inst];
    return;
  }
  // AX / GMRES: state left by PREPARE
  C.load_common(P.U);
  if (!C.fh_hbm()) C.load_row_to_lds(C.S.Fh, P.Fh);
  if (C.valid && C.r < M::NX) C.S.xh[C.r * IPW + C.inst] = P.xdxh[size_t(C.b) * M::NX + C.r];
  for (int q = C.r; q < P.Hp; q += 16) C.S.H[C.inst * P.Hp + q] = T(0);
  load_im(a, P.hook_in0);
  C.publish_direction(a);
  __syncthreads();
  C.ax(false);
  if (P.mode == WG_HOOK_AX) {
    C.lds_to_reg(a, C.S.W);
    store_im(P.hook_out, a);
    return;
  }
  load_im(c2, P.hook_in1);
  T ax0h[MAXM];
  C.lds_to_reg(ax0h, C.S.W);
  C.gmres(a, c2, ax0h);
  store_im(P.hook_out, a);
  C.store_status();
}

}  // namespace cgm
