// The row-parallel sweeps of the "wg" kernels — row-Newton (NWT = 1) and row-scan (NWT = 2): members of WgCtx
// (wg_ctx.hip.h).
#pragma once
#include "wg_ctx.hip.h"

namespace cgm {

// ---- NWT = 1: the perturbed state sweeps as Newton on the whole trajectory, row-parallel ----------------------------
// The serial state sweep (sweep_state) keeps ONE wave busy for ~12 k cycles per mat-vec while the others mostly wait
// (profiles/r04_wg_serial_instruction_counters.json: 23 % of the VALU issue slots used).  Here every row of 16 lanes solves its
// own instance's recurrence cgmres.hpp:132-140 for ALL stages at once, on all four waves:
//   * lane r of the row owns the stages 4r .. 4r+3 (dv <= 63);
//   * x0 / x2 (model.hpp:38,40: linear, no trig) as the DIFFERENCE to the unperturbed trajectory — a scan of the
//     control differences with powers of the constant 2 x 2 matrix, four in-row DPP steps;
//   * x1 / x3 by Newton's method on the stage equations, started from the unperturbed trajectory (the direction is
//     scaled by h = 1e-3..: the perturbed trajectory is close): per iteration the stage residuals, the local
//     composition of the lane's four linearised stage maps, one in-row scan of 2 x 2 affine maps (wave_scan.hip.h),
//     and the local expansion; sin / cos carried from iteration to iteration by rotation (fresh evaluation when an
//     angle moved too far).  Quadratic convergence: the loop ends when a correction is below 1e-10 relative, i.e. the next one would
//     be below rounding; measured two iterations per mat-vec.
// The base trajectory (x0, x1, x2, sin/cos per owned stage: 28 values per lane) is taken from the stage table of the tick's
// first unperturbed sweep (preamble), which stays the serial quad sweep.  The result differs from the serial sweep's
// by rounding only (tests/test_gpu_parity.py bounds it against the oracle like every other mapping).
// During the Arnoldi loop the base lives in LDS — in the stage table, which only the preamble's state sweeps use, in
// the scratch of the serial-sweep kernel's costate scan, which this kernel does not use at all, and behind everything
// else where those two are too small (plan_wg places the arrays: WgParams::base_off) — as pairs [q / 2][thread] per
// array: every lane reads back
// exactly what it wrote (no barrier), 16 bytes per access, conflict-free.  Call after the preamble's last barrier.
CGM_WGCTX_T
__device__ __forceinline__ typename CGM_WGCTX::Pair* CGM_WGCTX::base_pairs(int k, int thread) const {
  return reinterpret_cast<Pair*>(S.lds0 + P.base_off[k]) + thread;
}
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::store_base() {
  const T* src[NBASE] = {nb.x0, nb.x1, nb.x2, nb.sd, nb.cd, nb.s1, nb.c1};
#pragma unroll
  for (int k = 0; k < NBASE; ++k) {
    Pair* d = base_pairs(k, tid);
#pragma unroll
    for (int q = 0; q < SPL; q += 2) d[(q / 2) * IPW * 16] = Pair{src[k][q], src[k][q + 1]};
  }
  inv_dtau_nb = T(1) / dtau_h;
}
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::load_base(int k, T* dst, int thread) const {
  const Pair* d = base_pairs(k, thread);
#pragma unroll
  for (int q = 0; q < SPL; q += 2) {
    const Pair t = d[(q / 2) * IPW * 16];
    dst[q] = t.a, dst[q + 1] = t.b;
  }
}
// ---- stage ownership (stage_own.hip.h): this kernel's solver vectors are held by the lanes that own their stages, so
// the sweeps take the direction from, and leave the result in, the registers of the vector algebra.  What the sweeps
// need besides — U and F(U,x+hf,t+h) of the owned stages — sits in two lane-private LDS arrays in the format of the base
// arrays: slot pair p of (instance, lane) at pair index (p*IPW + instance)*lanes + lane, lanes = the ceil(dv/4) lanes
// that own a stage; 16 bytes per access, the lanes of a workgroup contiguous, every lane reads back what it wrote itself
// (no barrier).  Lanes without a stage read the last owning lane's words (finite, masked by their zero step sizes)
// and store nothing.  The arrays live in the storage of the row arrays U / Fh / W, which this kernel does not use;
// behind them the first controls of U and of U + h dUdt by stage for the preamble's serial sweeps, and the controls of
// stage 0 per instance [j*IPW + i] for x + h f and the plant step (StageOwn::lds_scalars).
CGM_WGCTX_T
__device__ __forceinline__ int CGM_WGCTX::so_lanes() const { return StageOwn::lanes(P.dv); }
CGM_WGCTX_T
__device__ __forceinline__ typename CGM_WGCTX::Pair* CGM_WGCTX::so_pairs(int which, int thread) const {
  const int n = so_lanes(), rr = thread & 15, ii = thread >> 4;
  return reinterpret_cast<Pair*>(S.lds0) + which * (NV / 2) * IPW * n + ii * n + (rr < n ? rr : n - 1);
}
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::so_load(int which, T* dst, int thread) const {
  const Pair* d = so_pairs(which, thread);
  const int step = IPW * so_lanes();
#pragma unroll
  for (int i = 0; i < NV; i += 2) {
    const Pair t = d[(i / 2) * step];
    dst[i] = t.a, dst[i + 1] = t.b;
  }
}
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::so_store(int which, const T* src, int thread) const {
  if ((thread & 15) >= so_lanes()) return;
  Pair* d = so_pairs(which, thread);
  const int step = IPW * so_lanes();
#pragma unroll
  for (int i = 0; i < NV; i += 2) d[(i / 2) * step] = Pair{src[i], src[i + 1]};
}
CGM_WGCTX_T
__device__ __forceinline__ T* CGM_WGCTX::so_stage(int which) const {  // 0: first controls of U, 1: of U + h dUdt; [instance][stage]
  return reinterpret_cast<T*>(S.lds0) + 2 * NV * IPW * so_lanes() + which * IPW * StageOwn::stage_pitch(P.dv);
}
CGM_WGCTX_T
__device__ __forceinline__ T* CGM_WGCTX::so_unow() const { return so_stage(2); }
// the row's new U: private array + the controls of stage 0
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::so_put_U(const T* u) const {
  so_store(0, u, tid);
  if (r == 0) {
#pragma unroll
    for (int j = 0; j < M::NU; ++j) so_unow()[j * IPW + inst] = u[j];
  }
}
// HBM rows [B][Lg] in the ABI's natural order: a lane moves its 12 contiguous elements, every one behind its e < L guard
// (the last owning lane reaches beyond L, at dv = 53 beyond the row's pitch: the next instance's row, or the end of
// the allocation).  Once per launch.
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::so_load_row(T* reg, const T* g) const {
  const T* src = g + size_t(b) * P.Lg;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int e = StageOwn::elem(r, i);
    reg[i] = (valid && e < P.L) ? src[e] : T(0);
  }
}
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::so_store_row(T* g, const T* reg) const {
  if (!valid) return;
  T* dst = g + size_t(b) * P.Lg;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int e = StageOwn::elem(r, i);
    if (e < P.L) dst[e] = reg[i];
  }
}
// the first controls of every owned stage, of U and of U + h d, for the serial sweeps of the preamble (sweep_state);
// call in front of the barrier the sweeps start behind
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::so_publish_u0(const T* d) const {
  if (!valid) return;
  T us[NV];
  so_load(0, us, tid);
  T* row = so_stage(0) + inst * StageOwn::stage_pitch(P.dv) + SPL * r;
  const int step = IPW * StageOwn::stage_pitch(P.dv);
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    if (SPL * r + q < P.dv) {
      row[q] = us[M::NU * q];
      row[step + q] = d[M::NU * q] * P.h + us[M::NU * q];
    }
  }
}
// The rotation of the Newton sweep's trig pairs, for the increments that sweep hands it (newton_rot.hip.h): sin dl and
// cos dl - 1 from the short polynomials of |dl| <= 2^CGM_NEWTON_ROT_LOG2_R, and the turn of a pair (sin, cos) of a base
// angle by the angle those two values belong to.  The turn by -dl takes (-sn, cm1) — the same bits as the polynomials
// of -dl would give: z is even in dl and every other operation odd.
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::newton_rot_step(T dl, T* sn_out, T* cm1_out) {
  constexpr double S[] = CGM_NEWTON_ROT_SIN, C[] = CGM_NEWTON_ROT_COS;
  constexpr int NS = sizeof(S) / sizeof(S[0]), NC = sizeof(C) / sizeof(C[0]);
  const T z = dl * dl;
  T ps = T(S[NS - 1]), pc = T(C[NC - 1]);
#pragma unroll
  for (int i = NS - 2; i >= 0; --i) ps = fma_t(z, ps, T(S[i]));
#pragma unroll
  for (int i = NC - 2; i >= 0; --i) pc = fma_t(z, pc, T(C[i]));
  *sn_out = fma_t(z * dl, ps, dl);
  *cm1_out = z * pc;
}
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::turn(T* s, T* c, T sn, T cm1) {
  const T sb = *s, cb = *c;
  *s = sb + fma_t(sb, cm1, cb * sn);
  *c = cb + fma_t(cb, cm1, -(sb * sn));
}
// Costate recurrence (cgmres.hpp:145-153) and dH/du (:156-161) of the row's instance from the states x(s) and trig
// values of the owned stages (x of "stage dv" = the terminal state), in registers:
//   MODE F_PLAIN: out = F        F_RHS: out = (F*(1-zeta h) - Fh)/h  (:91-96)        F_AX: out = (F - Fh)/h  (:173-174)
// PendulumDev::costate_step is affine in the costate with (l1, l3) closed in themselves, l0 a running sum over l3 and
// l2 a geometric recurrence over l0 / l3 — three scans DOWN the row (partner = the lane above), each as local fold,
// in-row scan, local expansion.  The terminal costate (cgmres.hpp:143) is the starting value of the lane that holds
// stage dv (nothing above it but identities).  u: the controls the owned stages were run with (U, or U + h d), out: the
// result, both in the stage ownership of the vector algebra (slot 3 q + j = control j of the lane's stage q); stages
// beyond the horizon deliver exact zeros, the pads of every solver vector.
CGM_WGCTX_T
template <int MODE>
__device__ __forceinline__ void CGM_WGCTX::row_costate(const T* x0f, const T* y1, const T* x2f, const T* y3, const T* sd, const T* cd,
                                                       const T* c1, const T* u, T dtau, T* out, int tid_o) {
  constexpr int NU = M::NU, NP = M::NP, NBW = M::NBW;
  static_assert(NU == 3 && NP == 2 && M::NUL == 1 && NV == SPL * NU, "written for the pendulum's stage");
  const int r = tid_o & 15, inst = tid_o >> 4;
  const int dv = P.dv, s_0 = SPL * r;
  const T ee = -dtau * M::C22, a = T(1) - dtau * M::As;
  const T sc_phi = MODE == F_RHS ? P.one_m_zh : T(1.0);
  const T sc = MODE == F_PLAIN ? T(1.0) : (MODE == F_RHS ? P.one_m_zh * P.inv_h : P.inv_h);
  bool tr[SPL];
  T dq[SPL], eq[SPL];
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    tr[q] = s_0 + q < dv;
    dq[q] = tr[q] ? dtau : T(0), eq[q] = tr[q] ? ee : T(0);
  }
  const int q_term = dv - s_0;
  const bool has_term = q_term >= 0 && q_term < SPL;
  T bw[SPL][NBW], phi0[SPL];
  T lT[M::NX] = {T(0), T(0), T(0), T(0)};
  CGM_STAMP(*this, 24);
  {
    T pp[SPL][NP], fh[NV];
    // every LDS operand first (parameter addresses clamped into the horizon: no branch, one wait): F(U,x+hf,t+h) of the
    // owned stages from the lane's private array, the parameters from the instance's row
    if constexpr (MODE != F_PLAIN) {
      so_load(1, fh, tid_o);
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) fh[i] = T(0);
    }
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      const int s = s_0 + q, sp = s < dv ? s : dv;
#pragma unroll
      for (int j = 0; j < NP; ++j) pp[q][j] = get_p(inst, sp * NP + j);
    }
    CGM_STAMP_LDS(*this, 27);
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      const T x[M::NX] = {x0f[q], y1[q], x2f[q], y3[q]};
      const T tg[3] = {sd[q], cd[q], c1[q]};
      const T* uq = u + NU * q;
      T phi[NU], bq[NBW];
      // (with the stage's own step size: every coefficient that enters the recurrences carries it as a factor and is
      // zero beyond the horizon; bw[3], which does not, is only used where the stage exists)
      M::stage_coeffs(bq, phi, x, uq, pp[q], tg, dq[q]);
#pragma unroll
      for (int cc = 0; cc < NBW; ++cc) bw[q][cc] = bq[cc];
      phi0[q] = MODE == F_PLAIN ? phi[0] : (phi[0] * sc_phi - fh[NU * q]) * P.inv_h;
      const T o1 = MODE == F_PLAIN ? phi[1] : (phi[1] * sc_phi - fh[NU * q + 1]) * P.inv_h;
      const T o2 = MODE == F_PLAIN ? phi[2] : (phi[2] * sc_phi - fh[NU * q + 2]) * P.inv_h;
      out[NU * q + 1] = tr[q] ? o1 : T(0), out[NU * q + 2] = tr[q] ? o2 : T(0);
      if (q == q_term) M::dPhidx(lT, x, pp[q]);
    }
  }
  CGM_STAMP(*this, 24);
  T L0[SPL], L2[SPL], L3[SPL];  // costate components ENTERING the owned stages (lambda of stage s + 1)
  {
    // (l1, l3): n1 = l1 + bw1 l3 + bw5,  n3 = l3 + dq l1 + eq l3; the lane with stage dv starts from the constant map
    T D[4] = {has_term ? T(-1) : T(0), T(0), T(0), has_term ? T(-1) : T(0)};
    T c[2] = {has_term ? lT[1] : T(0), has_term ? lT[3] : T(0)};
#pragma unroll
    for (int q = SPL - 1; q >= 0; --q) {
      const T b1 = bw[q][1];
      const T n00 = fma_t(b1, D[2], D[0]);
      const T n01 = fma_t(b1, D[3], D[1] + b1);
      const T n10 = fma_t(eq[q], D[2], fma_t(dq[q], D[0], D[2] + dq[q]));
      const T n11 = fma_t(eq[q], D[3], fma_t(dq[q], D[1], D[3] + eq[q]));
      const T m0 = fma_t(b1, c[1], c[0] + bw[q][5]);
      const T m1 = fma_t(eq[q], c[1], fma_t(dq[q], c[0], c[1]));
      D[0] = n00, D[1] = n01, D[2] = n10, D[3] = n11, c[0] = m0, c[1] = m1;
    }
    aff2_step_vec<0, true>(c, D), aff2_step_mat<0, true>(D);
    aff2_step_vec<1, true>(c, D), aff2_step_mat<1, true>(D);
    aff2_step_vec<2, true>(c, D), aff2_step_mat<2, true>(D);
    aff2_step_vec<3, true>(c, D);
    // costate entering the lane's last stage (the lanes above the one with stage dv deliver zeros)
    T l1 = scan_partner<0, true>(c[0]), l3 = scan_partner<0, true>(c[1]);
    l1 = has_term ? lT[1] : l1, l3 = has_term ? lT[3] : l3;
    T l0s = has_term ? lT[0] : T(0);  // l0 relative to the lane's entry: n0 = l0 + (bw4 + bw0 l3)
#pragma unroll
    for (int q = SPL - 1; q >= 0; --q) {
      L3[q] = l3, L0[q] = l0s;
      l0s += fma_t(bw[q][0], l3, bw[q][4]);
      const T n1 = fma_t(bw[q][1], l3, l1 + bw[q][5]);
      const T n3 = fma_t(eq[q], l3, fma_t(dq[q], l1, l3));
      l1 = n1, l3 = n3;
    }
    T t0 = l0s;
    t0 += scan_partner<0, true>(t0);
    t0 += scan_partner<1, true>(t0);
    t0 += scan_partner<2, true>(t0);
    t0 += scan_partner<3, true>(t0);
    const T in0 = scan_partner<0, true>(t0);
    // l2: n2 = aq l2 + (bw2 l3 + dq l0), aq = 1 - dq As
    T e2 = has_term ? lT[2] : T(0);
#pragma unroll
    for (int q = SPL - 1; q >= 0; --q) {
      L0[q] += in0;
      e2 = fma_t(fma_t(-M::As, dq[q], T(1)), e2, fma_t(bw[q][2], L3[q], dq[q] * L0[q]));
    }
    {
      const T a2 = a * a;
      T m = a2 * a2;  // (a lane with fewer than four stages has nothing but zeros above it: its multiplier is not used)
      e2 = fma_t(m, scan_partner<0, true>(e2), e2), m = m * m;
      e2 = fma_t(m, scan_partner<1, true>(e2), e2), m = m * m;
      e2 = fma_t(m, scan_partner<2, true>(e2), e2), m = m * m;
      e2 = fma_t(m, scan_partner<3, true>(e2), e2);
    }
    T l2 = scan_partner<0, true>(e2);
    l2 = has_term ? lT[2] : l2;
#pragma unroll
    for (int q = SPL - 1; q >= 0; --q) {
      L2[q] = l2;
      l2 = fma_t(fma_t(-M::As, dq[q], T(1)), l2, fma_t(bw[q][2], L3[q], dq[q] * L0[q]));
    }
  }
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    const T dF = fma_t(bw[q][3], L3[q], L2[q] * M::Bs);  // B^T lambda, costate_step
    out[NU * q] = tr[q] ? fma_t(dF, sc, phi0[q]) : T(0);
  }
  CGM_STAMP(*this, 23);
}

// ---- NWT = 2: a model whose state equation is AFFINE in x for given controls (semiactive_damper/model.hpp:36-39:
//      x0' = x1, x1' = a x0 + b u0 x1).  One evaluation of F (cgmres.hpp:113-162) is then two scans over the row and
//      nothing else — the state recurrence :132-140 as a scan of 2 x 2 maps UP the row (lane 0 starts from the constant
//      map "x(0)"), the costate recurrence :145-153 as one DOWN the row (the lane with stage dv starts from the terminal
//      costate, :143), four stages per lane folded locally on either side — exact up to rounding, no iteration, no stage
//      table, no serial sweep anywhere in the tick.
//      MODE as in row_costate; x0c: the initial state [c*IPW + i]; urow: the row of controls (may be `out`'s row).
CGM_WGCTX_T
template <int MODE>
__device__ __forceinline__ void CGM_WGCTX::row_affine_sweep(const T* x0c, T dtau, const T* urow, T* out, bool run) {
  constexpr int NU = M::NU, NBW = M::NBW;
  static_assert(M::NX == 2 && NU == 3 && M::NP == 0 && M::NUL == 1 && M::NC == 0 && NBW == 4,
                "written for the semi-active damper's stage");
  int tid_o = tid;  // (see row_newton_sweep)
  asm volatile("" : "+v"(tid_o));
  const int r = tid_o & 15, inst = tid_o >> 4;
  const int dv = P.dv, s_0 = SPL * r;
  const T sc_phi = MODE == F_RHS ? P.one_m_zh : T(1.0);
  const T sc = MODE == F_PLAIN ? T(1.0) : (MODE == F_RHS ? P.one_m_zh * P.inv_h : P.inv_h);
  bool tr[SPL];
  T dq[SPL], u0[SPL], u1[SPL], u2[SPL], fh[SPL][NU];
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    const int s = s_0 + q, sk = s < dv ? s : dv - 1;
    tr[q] = s < dv;
    dq[q] = tr[q] ? dtau : T(0);  // (stages beyond the horizon: identity maps)
    u0[q] = urow[sk * NU], u1[q] = urow[sk * NU + 1], u2[q] = urow[sk * NU + 2];
#pragma unroll
    for (int j = 0; j < NU; ++j) fh[q][j] = MODE == F_PLAIN ? T(0) : S.Fh[inst * P.Lp + sk * NU + j];
  }
  const int q_term = dv - s_0;
  const bool has_term = q_term >= 0 && q_term < SPL, first = r == 0;
  const T xi0 = x0c[0 * IPW + inst], xi1 = x0c[1 * IPW + inst];
  // ---- states: x(s+1) = x(s) + [[0, dq], [dq a, dq b u0]] x(s)
  T X0[SPL], X1[SPL], d2[SPL], d3[SPL];
  {
    T D[4] = {first ? T(-1) : T(0), T(0), T(0), first ? T(-1) : T(0)}, c[2] = {first ? xi0 : T(0), first ? xi1 : T(0)};
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      d2[q] = dq[q] * M::a, d3[q] = dq[q] * (M::b * u0[q]);
      const T n00 = fma_t(dq[q], D[2], D[0]);
      const T n01 = fma_t(dq[q], D[3], D[1] + dq[q]);
      const T n10 = fma_t(d3[q], D[2], fma_t(d2[q], D[0], D[2] + d2[q]));
      const T n11 = fma_t(d3[q], D[3], fma_t(d2[q], D[1], D[3] + d3[q]));
      const T m0 = fma_t(dq[q], c[1], c[0]);
      const T m1 = fma_t(d3[q], c[1], fma_t(d2[q], c[0], c[1]));
      D[0] = n00, D[1] = n01, D[2] = n10, D[3] = n11, c[0] = m0, c[1] = m1;
    }
    aff2_step_vec<0>(c, D), aff2_step_mat<0>(D);
    aff2_step_vec<1>(c, D), aff2_step_mat<1>(D);
    aff2_step_vec<2>(c, D), aff2_step_mat<2>(D);
    aff2_step_vec<3>(c, D);
    T e0 = scan_partner<0>(c[0]), e1 = scan_partner<0>(c[1]);  // the state the lane's first stage starts from
    e0 = first ? xi0 : e0, e1 = first ? xi1 : e1;
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      X0[q] = e0, X1[q] = e1;
      const T n0 = fma_t(dq[q], e1, e0);
      const T n1 = fma_t(d3[q], e1, fma_t(d2[q], e0, e1));
      e0 = n0, e1 = n1;
    }
  }
  // ---- stage coefficients, costate: n0 = l0 + bw2 + dq a l1,  n1 = l1 + bw3 + dq l0 + bw0 l1  (costate_step)
  T bw[SPL][NBW], phi0[SPL], L1[SPL];
  T lT[M::NX] = {T(0), T(0)};
#pragma unroll
  for (int q = 0; q < SPL; ++q) {
    const int s = s_0 + q;
    const T x[M::NX] = {X0[q], X1[q]}, u[NU] = {u0[q], u1[q], u2[q]};
    T phi[NU];
    M::stage_coeffs(bw[q], phi, x, u, nullptr, nullptr, dq[q]);  // (bw[1], which carries no step size, is only used where the stage exists)
    phi0[q] = MODE == F_PLAIN ? phi[0] : (phi[0] * sc_phi - fh[q][0]) * P.inv_h;
    if (run && tr[q]) {
      out[inst * P.Lp + s * NU + 1] = MODE == F_PLAIN ? phi[1] : (phi[1] * sc_phi - fh[q][1]) * P.inv_h;
      out[inst * P.Lp + s * NU + 2] = MODE == F_PLAIN ? phi[2] : (phi[2] * sc_phi - fh[q][2]) * P.inv_h;
    }
    if (q == q_term) M::dPhidx(lT, x, nullptr);
  }
  {
    T D[4] = {has_term ? T(-1) : T(0), T(0), T(0), has_term ? T(-1) : T(0)};
    T c[2] = {has_term ? lT[0] : T(0), has_term ? lT[1] : T(0)};
#pragma unroll
    for (int q = SPL - 1; q >= 0; --q) {
      const T b0 = bw[q][0];
      const T n00 = fma_t(d2[q], D[2], D[0]);
      const T n01 = fma_t(d2[q], D[3], D[1] + d2[q]);
      const T n10 = fma_t(b0, D[2], fma_t(dq[q], D[0], D[2] + dq[q]));
      const T n11 = fma_t(b0, D[3], fma_t(dq[q], D[1], D[3] + b0));
      const T m0 = fma_t(d2[q], c[1], c[0] + bw[q][2]);
      const T m1 = fma_t(b0, c[1], fma_t(dq[q], c[0], c[1] + bw[q][3]));
      D[0] = n00, D[1] = n01, D[2] = n10, D[3] = n11, c[0] = m0, c[1] = m1;
    }
    aff2_step_vec<0, true>(c, D), aff2_step_mat<0, true>(D);
    aff2_step_vec<1, true>(c, D), aff2_step_mat<1, true>(D);
    aff2_step_vec<2, true>(c, D), aff2_step_mat<2, true>(D);
    aff2_step_vec<3, true>(c, D);
    T l0 = scan_partner<0, true>(c[0]), l1 = scan_partner<0, true>(c[1]);  // costate entering the lane's last stage
    l0 = has_term ? lT[0] : l0, l1 = has_term ? lT[1] : l1;
#pragma unroll
    for (int q = SPL - 1; q >= 0; --q) {
      L1[q] = l1;
      const T n0 = fma_t(d2[q], l1, l0 + bw[q][2]);
      const T n1 = fma_t(bw[q][0], l1, fma_t(dq[q], l0, l1 + bw[q][3]));
      l0 = n0, l1 = n1;
    }
  }
  if (run) {
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      if (tr[q]) out[inst * P.Lp + (s_0 + q) * NU] = fma_t(bw[q][1] * L1[q], sc, phi0[q]);  // B^T lambda, costate_step
    }
  }
}
// the preamble of a tick with it: the three evaluations of cgmres.hpp:88-99 one after the other, every row for itself
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::preamble_affine(T* bb, T* ax0) {
  make_xh();
  __syncthreads();  // (x + h f of every instance is formed by the sweep lanes of wave 0)
  int tid_o = tid;
  asm volatile("" : "+v"(tid_o));
  const int inst = tid_o >> 4;
  const T* Urow = S.U + inst * P.Lp;
  row_affine_sweep<F_PLAIN>(S.xh, dtau_h, Urow, S.Fh, valid);
  row_affine_sweep<F_AX>(S.xh, dtau_h, S.W + inst * P.Lp, S.W, valid);
  lds_to_reg(ax0, S.W);
  row_affine_sweep<F_RHS>(S.xs, dtau_0, Urow, S.W, valid);
  lds_to_reg(bb, S.W);
}

// The preamble of a tick (see preamble()) for the row-parallel kernel: the three state sweeps stay the serial quad
// sweeps, side by side on waves 0-2 (#1 leaves its stage table in LDS, #2 / #3 park theirs in HBM); everything behind
// them — stage coefficients, costate recurrence, dH/du — every row does for itself in registers (row_costate), one
// sweep after the other with no workgroup barrier in between: F(U,x+hf,t+h) -> the lanes' private array, A*dUdt and b
// straight into the registers of the vector algebra.  The stage states of sweep #1, with freshly evaluated sin / cos, become the base of the
// Newton sweeps (nb; moved to LDS by store_base once every lane is done with the stage table).
// du: dUdt, the direction of the first mat-vec (warm start, cgmres.hpp:99).  Neither b nor A*dUdt passes through LDS.
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::preamble_rows(T* bb, T* ax0, const T* du) {
  so_publish_u0(du);
  make_xh();
  __syncthreads();
  const size_t tab_n = Lds::tab_count(P.dv);
  T* tab0 = P.scr + size_t(blockIdx.x) * 2 * tab_n;
  T* tab1 = tab0 + tab_n;
  T* xT0 = S.xT, *xT1 = S.xT + M::NX * IPW, *xT2 = S.xT + 2 * M::NX * IPW;
  sweep_state<false, false>(0, S.xh, dtau_h, S.R, xT0, false);
  sweep_state<false, false>(64, S.xs, dtau_0, tab0, xT1, false);
  sweep_state<true, false>(128, S.xh, dtau_h, tab1, xT2, false);
  __threadfence_block();
  __syncthreads();  // drains vmcnt: the HBM tables are complete and visible to the other waves of this CU
  CGM_STAMP(*this, 4);
  int tid_o = tid;
  asm volatile("" : "+v"(tid_o));
  const int r = tid_o & 15, inst = tid_o >> 4, dv = P.dv;
  struct Stages {
    T x0[SPL], x1[SPL], x2[SPL], x3[SPL], sd[SPL], cd[SPL], c1[SPL];
  };
  // x and trig of the owned stages from a stage table (slot map: PendulumDev::quad_stage), x(dv) from xT
  auto read_stages = [&](Stages& g, const T* tab, const T* xT) {
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      const int s = SPL * r + q, sk = s < dv ? s : 0;
      const T* e = tab + tab_off(sk) + inst;
      g.x0[q] = e[M::QSLOT_XA * IPW], g.x1[q] = e[1 * IPW], g.x2[q] = e[M::QSLOT_XB * IPW], g.x3[q] = T(0);
      g.sd[q] = e[M::TRIG_SLOT0 * IPW], g.cd[q] = e[(M::TRIG_SLOT0 + 1) * IPW], g.c1[q] = e[(M::TRIG_SLOT0 + 2) * IPW];
    }
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      const int s = SPL * r + q;
      if (s == dv) g.x0[q] = xT[0 * IPW + inst], g.x1[q] = xT[1 * IPW + inst], g.x2[q] = xT[2 * IPW + inst], g.x3[q] = xT[3 * IPW + inst];
      // (x1 beyond the horizon repeats the terminal value: the Newton sweep then finds zero residuals there without a
      // select, see row_newton_sweep; row_costate sees it through bw[5] alone, which carries the stage's zero step size)
      if (s > dv) g.x0[q] = T(0), g.x1[q] = xT[1 * IPW + inst], g.x2[q] = T(0);
    }
  };
  T us[NV];  // U of the owned stages
  so_load(0, us, tid_o);
  {
    Stages g;
    read_stages(g, S.R, xT0);
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      nb.x0[q] = g.x0[q], nb.x1[q] = g.x1[q], nb.x2[q] = g.x2[q];
      mc.sincos_pair(g.x0[q] - g.x1[q], g.x1[q], &nb.sd[q], &nb.cd[q], &nb.s1[q], &nb.c1[q]);
    }
    T fh[NV];
    row_costate<F_PLAIN>(g.x0, g.x1, g.x2, g.x3, g.sd, g.cd, g.c1, us, dtau_h, fh, tid_o);
    so_store(1, fh, tid_o);  // (read back by this same lane only)
  }
  {
    Stages g;
    read_stages(g, tab1, xT2);
    T uw[NV];  // the controls sweep #3 ran with (the same expression as so_publish_u0)
#pragma unroll
    for (int i = 0; i < NV; ++i) uw[i] = du[i] * P.h + us[i];
    row_costate<F_AX>(g.x0, g.x1, g.x2, g.x3, g.sd, g.cd, g.c1, uw, dtau_h, ax0, tid_o);
  }
  {
    Stages g;
    read_stages(g, tab0, xT1);
    row_costate<F_RHS>(g.x0, g.x1, g.x2, g.x3, g.sd, g.cd, g.c1, us, dtau_0, bb, tid_o);
  }
  __syncthreads();  // every lane is done with the stage table: the base may move in (store_base)
}

// F(U + h d, x + h f, t + h) - F(U, x + h f, t + h), / h, for the row's instance: state recurrence, costate recurrence
// and dH/du all in the registers of the row's 16 lanes — no stage table, no workgroup barrier; the only LDS traffic is
// reads of the lanes' own operands (U and F(U,x+hf,t+h) of the owned stages, the base trajectory, ptau).
// COLLECTIVE over the wave (wave-uniform branches on __any).
// Stages outside the horizon (s >= dv; the last lanes of the row) are IDENTITY maps by construction — their step
// sizes and coefficients are zeroed once per sweep — so the folds and expansions below carry no per-stage selects.
// v: the direction d, out: the result, both in the stage ownership of the vector algebra (NV elements per lane).  Also
// sets row_moved: did the direction change any control of this row?  One that the rounding of U + h*d absorbs completely
// leaves F unchanged bit for bit in the serial sweeps — A*d = 0 exactly, the reference's breakdown case
// (gmres.hpp:63-65) — while Newton's fixed point agrees with the serial trajectory up to rounding only: gmres()
// answers that case from this flag.
CGM_WGCTX_T
template <int MODE>
__device__ __forceinline__ void CGM_WGCTX::row_newton_sweep(T dtau, const T* v, T* out, bool run) {
  constexpr int NU = M::NU;
  static_assert(MODE == F_AX, "only the mat-vec of the Arnoldi loop");
  // (everything below derives from the thread index and is invariant over sweeps and ticks: left visible, the compiler
  // hoists it to the top of the kernel and keeps dozens of values alive across the Gram-Schmidt rounds — in scratch,
  // reloaded behind s_waitcnt vmcnt(0), i.e. behind the basis rows in flight)
  int tid_o = tid;
  asm volatile("" : "+v"(tid_o));
  const int r = tid_o & 15;
  const int dv = P.dv, s_0 = SPL * r;
  const T ee = -dtau * M::C22;
  bool tr[SPL];            // stage s_0 + q has a transition (s < dv)
  T dq[SPL], eq[SPL];      // its step sizes: dtau, -dtau C22, or 0
  T u[NV], u0[SPL], du[SPL];
  so_load(0, u, tid_o);  // U of the owned stages
  {
    bool moved = false;
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      tr[q] = s_0 + q < dv;
      dq[q] = tr[q] ? dtau : T(0), eq[q] = tr[q] ? ee : T(0);
      const T ub = u[NU * q];
#pragma unroll
      for (int j = 0; j < NU; ++j) {  // U + h d (cgmres.hpp:166-168); the pads of d and of U are zeros
        const T uv = v[NU * q + j] * P.h + u[NU * q + j];
        moved = moved || uv != u[NU * q + j];
        u[NU * q + j] = uv;
      }
      u0[q] = u[NU * q];
      du[q] = tr[q] ? u0[q] - ub : T(0);
    }
    row_moved = ((__ballot(moved) >> (16 * ((tid_o >> 4) & 3))) & 0xffffull) != 0;
  }
  CGM_STAMP_LDS(*this, 26);
  // (the base trajectory is requested with the controls: one LDS round trip for both)
  T b0[SPL], b2[SPL], y1[SPL], sd[SPL], cd[SPL], s1[SPL], c1[SPL];
  load_base(0, b0, tid_o), load_base(2, b2, tid_o), load_base(1, y1, tid_o);
  load_base(3, sd, tid_o), load_base(4, cd, tid_o), load_base(5, s1, tid_o), load_base(6, c1, tid_o);
  // ---- x0, x2: difference to the base trajectory (zero initial difference)
  const T a = T(1) - dtau * M::As, bs = dtau * M::Bs;
  T dx0[SPL], dx2[SPL];
  {
    // (the first two stages written out — from a zero difference the first leaves (0, bs du), and the second still
    // finds e0 = 0: left in the loop, their operations on literal zeros stay in the instruction stream, there being
    // no fast-math to fold them)
    static_assert(SPL >= 2, "two stages of the fold are written out");
    const T e2_0 = bs * du[0];
    T e0 = dtau * e2_0, e2 = fma_t(a, e2_0, bs * du[1]);
#pragma unroll
    for (int q = 2; q < SPL; ++q) {
      const T n0 = fma_t(dtau, e2, e0);
      e2 = fma_t(a, e2, bs * du[q]);
      e0 = n0;
    }
    const T a2 = a * a;
    T m11 = a2 * a2, m01 = dtau * ((T(1) + a) + (a2 + a * a2));  // the lane's four stages: [[1, m01], [0, m11]]
    auto step = [&](auto tc) {
      constexpr int t = decltype(tc)::value;
      const T p0 = scan_partner<t>(e0), p2 = scan_partner<t>(e2);
      e0 = (e0 + p0) + m01 * p2;
      e2 = fma_t(m11, p2, e2);
      m01 = fma_t(m01, m11, m01);
      m11 = m11 * m11;
    };
    step(std::integral_constant<int, 0>{}), step(std::integral_constant<int, 1>{});
    step(std::integral_constant<int, 2>{}), step(std::integral_constant<int, 3>{});
    T x0 = scan_partner<0>(e0), x2 = scan_partner<0>(e2);  // the state the lane's first stage starts from
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      dx0[q] = x0, dx2[q] = x2;
      const T n0 = fma_t(dtau, x2, x0);
      x2 = fma_t(a, x2, bs * du[q]);
      x0 = n0;
    }
  }
  CGM_STAMP(*this, 21);
  // ---- x1, x3: Newton.  The trig values are carried from iteration to iteration by rotation: first by the change of
  //      x0 (y1 starts at the base value), then by the corrections of y1.
  T x0f[SPL], x2f[SPL], Pq[SPL], Qq[SPL], y3[SPL];
  {
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      x0f[q] = b0[q] + dx0[q], x2f[q] = b2[q] + dx2[q];
      Pq[q] = M::A32 * x2f[q] * x2f[q];
      Qq[q] = M::A32a * x2f[q] - M::A32b * u0[q];
    }
    // x3 is not part of the base: x3(s) = (x1(s+1) - x1(s)) / dtau of the base trajectory (a starting value only)
    const T yb = dpp_row_zero_fill<0x101>(y1[0]);  // row_shl:1
#pragma unroll
    for (int q = 0; q < SPL; ++q)
      y3[q] = tr[q] ? ((q + 1 < SPL ? y1[q + 1 < SPL ? q + 1 : 0] : yb) - y1[q]) * inv_dtau_nb : T(0);
  }
  // angle increment of x0 - x1 since the trig values were last brought up to date: the change of x0 in the first
  // iteration, where x1 still is the base's, then minus the correction of x1 — whose own increment is that correction,
  // so from the second iteration on one pair (sin, cos - 1) turns (sd, cd) one way and (s1, c1) the other
  T ad[SPL];
#pragma unroll
  for (int q = 0; q < SPL; ++q) ad[q] = dx0[q];
  const T rmax = T(1) / T(1ll << -(CGM_NEWTON_ROT_LOG2_R));
  for (int it = 0; it < NEWTON_MAX; ++it) {
    T jq[SPL], c0q[SPL], c1q[SPL];
    T amax = T(0);  // (stages outside the horizon carry harmless finite values)
#pragma unroll
    for (int q = 0; q < SPL; ++q) amax = __builtin_fmax(amax, abs_t(ad[q]));
#ifdef CGM_AMAX
    cgm_amax_record(run, amax, it);
#endif
    if (__builtin_expect((P.wave_dbg & 1) || __any(run && !(amax <= rmax)), 0)) {
#pragma unroll
      for (int q = 0; q < SPL; ++q) mc.sincos_pair(x0f[q] - y1[q], y1[q], &sd[q], &cd[q], &s1[q], &c1[q]);
    } else {
#pragma unroll
      for (int q = 0; q < SPL; ++q) {
        T sn, cm1;
        newton_rot_step(ad[q], &sn, &cm1);
        turn(&sd[q], &cd[q], sn, cm1);
        if (it > 0) turn(&s1[q], &c1[q], -sn, cm1);
      }
    }
    // defects of the stage equations (the stage after the lane's last one belongs to the next lane) and the local
    // composition of the linearised stage maps  D -> D + [[0, dq], [j, eq]] (I + D)  in the D-form of wave_scan.hip.h
    const T yn1 = dpp_row_zero_fill<0x101>(y1[0]), yn3 = dpp_row_zero_fill<0x101>(y3[0]);  // row_shl:1
    // (from D = 0, c = 0 the first stage leaves its own map, and the second still finds D[0] = 0: written out, like
    // the first stages of the x0/x2 fold)
    T D[4], c[2];
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      // model.hpp:41 and its derivative in x1
      const T g = fma_t(Pq[q], sd[q], fma_t(M::A52, s1[q], fma_t(Qq[q], cd[q], M::C22 * (x2f[q] - y3[q]))));
      const T J1 = fma_t(Qq[q], sd[q], fma_t(M::A52, c1[q], -(Pq[q] * cd[q])));
      // Beyond the horizon (s >= dv) the residuals vanish by DATA, not by a select: the step there is dq = 0, so t1
      // and t3 are y1 and y3 of the stage themselves (where the stage exists dq IS dtau: the same bits); the base
      // holds x1(dv) in every such stage, y3 starts from 0 there, and both receive the correction that the identity
      // maps carry on.  Inside a lane that correction is the same bits from stage to stage and the residual an exact
      // zero.  Across a lane boundary it arrives through the scan, whose rounding is not that of the lane's own
      // expansion: y1 can differ from its neighbour by an ulp there, which the next iteration sees as a residual of
      // that size and corrects — among stages that feed nothing (the folds run up the row, and nothing beyond stage dv
      // is read by row_costate except through zero coefficients).  The last stage of lane 15 has the zero fill of
      // row_shl for a neighbour: its residual enters lane 15's own fold only, which no lane reads.
      const T t1 = fma_t(dq[q], y3[q], y1[q]), t3 = fma_t(dq[q], g, y3[q]);
      jq[q] = dq[q] * J1;
      c0q[q] = t1 - (q + 1 < SPL ? y1[q + 1 < SPL ? q + 1 : 0] : yn1);
      c1q[q] = t3 - (q + 1 < SPL ? y3[q + 1 < SPL ? q + 1 : 0] : yn3);
      if (q == 0) {
        D[0] = T(0), D[1] = dq[0], D[2] = jq[0], D[3] = eq[0], c[0] = c0q[0], c[1] = c1q[0];
        continue;
      }
      const bool z = q == 1;  // D[0] is the first stage's zero
      const T n00 = z ? dq[q] * D[2] : fma_t(dq[q], D[2], D[0]);
      const T n01 = fma_t(dq[q], D[3], D[1] + dq[q]);
      const T n10 = fma_t(eq[q], D[2], z ? D[2] + jq[q] : fma_t(jq[q], D[0], D[2] + jq[q]));
      const T n11 = fma_t(eq[q], D[3], fma_t(jq[q], D[1], D[3] + eq[q]));
      const T m0 = fma_t(dq[q], c[1], c[0] + c0q[q]);
      const T m1 = fma_t(eq[q], c[1], fma_t(jq[q], c[0], c[1] + c1q[q]));
      D[0] = n00, D[1] = n01, D[2] = n10, D[3] = n11, c[0] = m0, c[1] = m1;
    }
    aff2_step_vec<0>(c, D), aff2_step_mat<0>(D);
    aff2_step_vec<1>(c, D), aff2_step_mat<1>(D);
    aff2_step_vec<2>(c, D), aff2_step_mat<2>(D);
    aff2_step_vec<3>(c, D);
    T e1 = scan_partner<0>(c[0]), e3 = scan_partner<0>(c[1]);  // correction of the lane's first stage
    T viol = T(-1);
    T dl1[SPL];
    const T th = T(1e-10);
#pragma unroll
    for (int q = 0; q < SPL; ++q) {
      y1[q] += e1, y3[q] += e3;
      dl1[q] = e1, ad[q] = -e1;
      // |e| - th (1 + |y|) > 0 ?  (the "- th" is taken off once, after the loop)
      const T vq = __builtin_fmax(fma_t(-th, abs_t(y1[q]), abs_t(e1)), fma_t(-th, abs_t(y3[q]), abs_t(e3)));
      // (beyond stage dv its correction is carried on — up to the ulp-sized residuals above, which are 1e-6 of the
      // threshold: without this select one termination decision in a million falls the other way, and the bench,
      // which takes 2.6e7 of them, ends 7e-12 away in dUdt — profiles/r10_iter_diet_ab.json.  The select stays.)
      viol = s_0 + q <= dv ? __builtin_fmax(viol, vq) : viol;
      const T n1 = fma_t(dq[q], e3, e1 + c0q[q]);
      const T n3 = fma_t(eq[q], e3, fma_t(jq[q], e1, e3 + c1q[q]));
      e1 = n1, e3 = n3;
    }
    CGM_STAMP(*this, 22);
    if (!__any(run && viol > th)) {
      // the correction is below the square root of the rounding level: trig values to first order, done
#pragma unroll
      for (int q = 0; q < SPL; ++q) {
        const T nsd = fma_t(cd[q], -dl1[q], sd[q]), ncd = fma_t(sd[q], dl1[q], cd[q]);
        const T ns1 = fma_t(c1[q], dl1[q], s1[q]), nc1 = fma_t(s1[q], -dl1[q], c1[q]);
        sd[q] = nsd, cd[q] = ncd, s1[q] = ns1, c1[q] = nc1;
      }
      break;
    }
  }
  row_costate<MODE>(x0f, y1, x2f, y3, sd, cd, c1, u, dtau, out, tid_o);
}

}  // namespace cgm
