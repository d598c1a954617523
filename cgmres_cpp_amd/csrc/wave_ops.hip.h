// What a model brings to the "wave" mapping (tick_wave.hip.h): the scans of its horizon recurrences over the lanes of a
// wave (WaveOps), and the LDS layout of one wave (WaveLds).  No kernel: the planner (wg_plan.hip.h) reads the traits and
// the layout from here.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "models.hip.h"
#include "wave_scan.hip.h"

namespace cgm {

// what a model's scans need to know about the lane
struct WaveLane {
  int lane, dv, msrc;  // msrc: the mirrored lane of the costate scans (stage dv-1-m on lane m; an involution on [0, dv))
  bool in_hor;         // the lane has a stage with controls
};

// which models have the scans above, and how.  NONLINEAR: the state equation is not affine in x — Newton on the trajectory
// from a base trajectory, serial sweeps in front of the solve (the code in the kernel); otherwise the model supplies
//   state_scan  (L, u, xinit, dtau, x)            x(s) of every lane's stage from the lane's controls: ONE scan, exact
//   costate_scan(L, x, u, p, dtau, phi, dF)       costate recurrence + dH/du pieces from the lane's stage
// or, with SERIAL_STATE (user models), state_sweeps<NS>(L, u, xinit, dtau, p, x): NS serial sweeps side by side
template <class M>
struct WaveOps : std::false_type {  // (no wave scans: whatever is not specialised below)
  static constexpr bool NONLINEAR = false;
  static constexpr int LDS_EXTRA = 0;
};

template <class T>
struct WaveOps<PendulumDev<T>> : std::true_type {
  using M = PendulumDev<T>;
  static constexpr bool NONLINEAR = true;
  using TickConsts = GeoPowers<T>;  // powers of 1 - dtau As (x2 and l2 are geometric recurrences)
  static constexpr int LDS_EXTRA = 0;
  static __device__ __forceinline__ void make_consts(TickConsts& G, T dtau, const WaveLane&, T*) { G.make(T(1) - dtau * M::As); }
  // sin/cos of (base angle + dl) from the base pair, |dl| <= sqrt(rot_zmax) (Taylor polynomials of the wg mapping's
  // rotation stage, MathCtx::rot_sin / rot_cos)
  template <class MC>
  static __device__ __forceinline__ void rotate(T sb, T cb, T dl, T* s, T* c, const MC& mc) {
    constexpr int NRS = MC::NRS, NRC = MC::NRC;
    const T z = dl * dl;
    T ps = mc.rot_sin(NRS - 1), pc = mc.rot_cos(NRC - 1);
#pragma unroll
    for (int i = NRS - 2; i >= 0; --i) ps = fma_t(z, ps, mc.rot_sin(i));
#pragma unroll
    for (int i = NRC - 2; i >= 0; --i) pc = fma_t(z, pc, mc.rot_cos(i));
    const T sn = fma_t(z * dl, ps, dl);  // sin dl
    const T cm1 = z * pc;                // cos dl - 1
    *s = sb + fma_t(sb, cm1, cb * sn);
    *c = cb + fma_t(cb, cm1, -(sb * sn));
  }
};

// semiactive_damper/model.hpp:36-55: x0' = x1, x1' = a x0 + b u0 x1 — affine in x for given controls: the state sweep IS
// one scan of 2 x 2 affine maps (exact up to rounding, no iteration, no serial sweep anywhere), and so is the costate
// recurrence (SemiactiveDev::costate_step).
template <class T>
struct WaveOps<SemiactiveDev<T>> : std::true_type {
  using M = SemiactiveDev<T>;
  static constexpr bool NONLINEAR = false;
  struct TickConsts {};
  static constexpr int LDS_EXTRA = 0;
  static __device__ __forceinline__ void make_consts(TickConsts&, T, const WaveLane&, T*) {}
  static __device__ __forceinline__ void state_scan(const WaveLane& L, const T* u, const T* xinit, T dtau, const TickConsts&,
                                                    T* x) {
    // y' = y + D y,  D = [[0, dtau], [dtau a, dtau b u0]]; lane 0 applies its map to the initial state
    T D[4] = {T(0), dtau, dtau * M::a, dtau * M::b * u[0]};
    const bool first = L.lane == 0;
    const T y0 = first ? xinit[0] : T(0), y1 = first ? xinit[1] : T(0);
    T c[2] = {y0 + D[1] * y1, y1 + fma_t(D[2], y0, D[3] * y1)};
    scan_aff2(D, c);
    x[0] = wave_shift_up(c[0], xinit[0]);
    x[1] = wave_shift_up(c[1], xinit[1]);
  }
  static __device__ __forceinline__ void costate_scan(const WaveLane& L, const T* x, const T* u, const T*, T dtau,
                                                      const TickConsts&, T* phi, T* dF) {
    T bw[M::NBW], trig[1] = {T(0)};
    M::stage_coeffs(bw, phi, x, u, nullptr, trig, dtau);
    T xT[M::NX], lT[M::NX];
#pragma unroll
    for (int c = 0; c < M::NX; ++c) xT[c] = wave_bcast(x[c], L.dv);
    M::dPhidx(lT, xT, nullptr);
    T mb[M::NBW];
#pragma unroll
    for (int c = 0; c < M::NBW; ++c) mb[c] = wave_gather(bw[c], L.msrc);
    const bool first = L.lane == 0;
    const T i0 = first ? lT[0] : T(0), i1 = first ? lT[1] : T(0);
    // n0 = l0 + bw2 + dtau a l1,  n1 = l1 + bw3 + dtau l0 + bw0 l1
    T D[4] = {T(0), dtau * M::a, dtau, mb[0]};
    T c[2] = {mb[2] + i0 + D[1] * i1, mb[3] + i1 + fma_t(D[2], i0, D[3] * i1)};
    scan_aff2(D, c);
    const T in1 = wave_shift_up(c[1], lT[1]);  // costate ENTERING the lane's stage
    dF[0] = wave_gather(mb[1] * in1, L.msrc);  // B^T l of the stage (model.hpp:52)
  }
};

// mass_spring_damper/model.hpp:36-64: linear and time-invariant — x' = x + dtau (A x + B u), l' = l + bw + dtau (Al l) with
// CONSTANT 4 x 4 matrices (A from dxdt :36-41, Al from dHdx :50-55 — not each other's transpose: the reference's
// k1*k2 / k1+k2 quirk).  Every composed matrix of a scan is a power of I + dtau A (resp. Al): one table of powers per
// horizon step and recurrence in LDS (power_table4, built once per tick), then a sweep is two VECTOR-only scans.
template <class T>
struct WaveOps<MsdDev<T>> : std::true_type {
  using M = MsdDev<T>;
  static constexpr bool NONLINEAR = false;
  static constexpr int TABLE = 32 * 16;              // scalars of one power table
  static constexpr int LDS_EXTRA = 4 * TABLE;        // state + costate tables for dtau_h and for dtau_0
  struct TickConsts {
    const T *st, *co;
  };
  static __device__ __forceinline__ void make_consts(TickConsts& G, T dtau, const WaveLane& L, T* lds) {
    const T A[16] = {T(0), T(0), T(1), T(0),                                                           // model.hpp:37
                     T(0), T(0), T(0), T(1),                                                           // :38
                     -(M::k1 * M::k2) / M::m1, M::k2 / M::m1, -(M::d1 + M::d2) / M::m1, M::d2 / M::m1,  // :39
                     M::k2 / M::m2, -M::k2 / M::m2, M::d2 / M::m2, -M::d2 / M::m2};                    // :40
    const T Al[16] = {T(0), T(0), -(M::k1 + M::k2) / M::m1, M::k2 / M::m2,    // :51
                      T(0), T(0), M::k2 / M::m1, -M::k2 / M::m2,              // :52
                      T(1), T(0), -(M::d1 + M::d2) / M::m1, M::d2 / M::m2,    // :53
                      T(0), T(1), M::d2 / M::m1, -M::d2 / M::m2};             // :54
    T D[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) D[e] = dtau * A[e];
    power_table4(lds, D, L.lane);
#pragma unroll
    for (int e = 0; e < 16; ++e) D[e] = dtau * Al[e];
    power_table4(lds + TABLE, D, L.lane);
    G.st = lds, G.co = lds + TABLE;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  static __device__ __forceinline__ void state_scan(const WaveLane& L, const T* u, const T* xinit, T dtau, const TickConsts& G,
                                                    T* x) {
    const bool first = L.lane == 0;
    T y[4], c[4] = {T(0), T(0), L.in_hor ? dtau * (u[0] / M::m1) : T(0), L.in_hor ? dtau * (u[1] / M::m2) : T(0)};
#pragma unroll
    for (int r = 0; r < 4; ++r) y[r] = first ? xinit[r] : T(0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // lane 0 applies its map to the initial state: c += (I + D) x(0)
      T a = c[r] + y[r];
#pragma unroll
      for (int k = 0; k < 4; ++k) a = fma_t(G.st[4 * r + k], y[k], a);
      c[r] = a;
    }
    scan_const4(c, G.st, L.lane);
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = wave_shift_up(c[r], xinit[r]);
  }
  static __device__ __forceinline__ void costate_scan(const WaveLane& L, const T* x, const T* u, const T* p, T dtau,
                                                      const TickConsts& G, T* phi, T* dF) {
    T bw[M::NBW], trig[1] = {T(0)};
    M::stage_coeffs(bw, phi, x, u, p, trig, dtau);
    T xT[M::NX], pT[M::NP], lT[M::NX];
#pragma unroll
    for (int c = 0; c < M::NX; ++c) xT[c] = wave_bcast(x[c], L.dv);
#pragma unroll
    for (int j = 0; j < M::NP; ++j) pT[j] = wave_bcast(p[j], L.dv);
    M::dPhidx(lT, xT, pT);
    const bool first = L.lane == 0;
    T c[4], y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = wave_gather(bw[r], L.msrc), y[r] = first ? lT[r] : T(0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T a = c[r] + y[r];
#pragma unroll
      for (int k = 0; k < 4; ++k) a = fma_t(G.co[4 * r + k], y[k], a);
      c[r] = a;
    }
    scan_const4(c, G.co, L.lane);
    const T in2 = wave_shift_up(c[2], lT[2]), in3 = wave_shift_up(c[3], lT[3]);  // costate ENTERING the lane's stage
    dF[0] = wave_gather(in2 / M::m1, L.msrc);  // model.hpp:58-59
    dF[1] = wave_gather(in3 / M::m2, L.msrc);
  }
};

// USER models (user_model.hip.h), fp64.  Nothing is known about the state equation, so the state recurrence
// x(s+1) = x(s) + dxdt(x(s), U(s), p(s)) dtau (cgmres.hpp:131-140) is walked SERIALLY inside the wave: a wave-uniform
// loop over the stages, stage s's controls and parameters fetched with readlane, the model's dxdt on wave-uniform values,
// x(s+1) kept by lane s+1.  No LDS.  state_sweeps<NS> runs NS independent sweeps in one loop so that their dependency
// chains overlap (the three sweeps in front of the solve).  The costate recurrence is affine in the costate with the
// coefficients UserDev::stage_coeffs generates by probing the user's dHdx / dHdu (checked on the device,
// user_affinity_kernel): lambda(s) = (I + dtau J(s)^T) lambda(s+1) + dtau q(s) — one scan of NX x NX affine maps on
// the mirrored lanes (scan_affn), and dF(s) = B(s)^T lambda(s+1) on the lane of stage s.
// Limits (WgTraits::wave_supported, wg_plan.hip.h): NX <= kUserWaveMaxNx — the scan keeps a map and its DPP partner (2 NX^2 + 2 NX
// doubles) next to the register-resident Krylov basis; NU <= kUserWaveMaxNu (the basis is (k_max + 1) NU doubles per lane).
constexpr int kUserWaveMaxNx = 4, kUserWaveMaxNu = 6;
template <class Model>
struct UserDev;
template <class Model>
struct WaveOps<UserDev<Model>> : std::true_type {
  using M = UserDev<Model>;
  using T = double;
  static constexpr bool NONLINEAR = false;
  static constexpr bool SERIAL_STATE = true;  // state_sweeps instead of state_scan; p of stage 0 in x_dxh and the plant
  static constexpr bool FITS = M::NX <= kUserWaveMaxNx && M::NU <= kUserWaveMaxNu;
  struct TickConsts {};
  static constexpr int LDS_EXTRA = 0;
  static __device__ __forceinline__ void make_consts(TickConsts&, T, const WaveLane&, T*) {}
  // x[q] of every lane's stage (lane 0: xinit[q]; lanes beyond dv keep xinit[q]) for the controls u[q] on the lanes
  template <int NS>
  static __device__ __forceinline__ void state_sweeps(const WaveLane& L, const T (&u)[NS][M::NU], const T (&xinit)[NS][M::NX],
                                                      const T (&dtau)[NS], const T* p, T (&x)[NS][M::NX]) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    T y[NS][NX];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
#pragma unroll
      for (int c = 0; c < NX; ++c) y[q][c] = xinit[q][c], x[q][c] = xinit[q][c];
    }
    for (int s = 0; s < L.dv; ++s) {  // (wave-uniform)
      T ps[NP > 0 ? NP : 1];
      ps[0] = T(0);
#pragma unroll
      for (int j = 0; j < NP; ++j) ps[j] = wave_bcast(p[j], s);
      const bool mine = L.lane == s + 1;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        T us[NU], f[NX];
#pragma unroll
        for (int j = 0; j < NU; ++j) us[j] = wave_bcast(u[q][j], s);
        M::dxdt_p(f, y[q], us, ps);
#pragma unroll
        for (int c = 0; c < NX; ++c) {
          y[q][c] = f[c] * dtau[q] + y[q][c];
          x[q][c] = mine ? y[q][c] : x[q][c];
        }
      }
    }
  }
  static __device__ __forceinline__ void costate_scan(const WaveLane& L, const T* x, const T* u, const T* p, T dtau,
                                                      const TickConsts&, T* phi, T* dF) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    T bw[M::NBW];
    M::stage_coeffs(bw, phi, x, u, p, nullptr, dtau);
    // terminal costate from the terminal stage (lane dv), wave-uniform (cgmres.hpp:146)
    T xT[NX], pT[NP > 0 ? NP : 1], lT[NX];
    pT[0] = T(0);
#pragma unroll
    for (int c = 0; c < NX; ++c) xT[c] = wave_bcast(x[c], L.dv);
#pragma unroll
    for (int j = 0; j < NP; ++j) pT[j] = wave_bcast(p[j], L.dv);
    M::dPhidx(lT, xT, pT);
    // the map of stage dv-1-m on lane m: l -> l + D l + c with D = dtau J^T, c = dtau q; lane 0 applies its map to the
    // terminal costate (c += (I + D) lT)
    T D[NX * NX], c[NX];
#pragma unroll
    for (int e = 0; e < NX * NX; ++e) D[e] = wave_gather(bw[e], L.msrc);
#pragma unroll
    for (int r = 0; r < NX; ++r) c[r] = wave_gather(bw[M::NBW_LIN + r], L.msrc);
    const bool first = L.lane == 0;
    T y[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) y[r] = first ? lT[r] : T(0);
#pragma unroll
    for (int r = 0; r < NX; ++r) {
      T a = c[r] + y[r];
#pragma unroll
      for (int k = 0; k < NX; ++k) a = fma_t(D[NX * r + k], y[k], a);
      c[r] = a;
    }
    scan_affn<NX>(D, c);
    // the costate ENTERING the stage, back on the stage's own lane: dF = B^T lambda(s+1) (cgmres.hpp:155-161)
    T l[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) l[r] = wave_gather(wave_shift_up(c[r], lT[r]), L.msrc);
#pragma unroll
    for (int j = 0; j < NU; ++j) {
      T a = T(0);
#pragma unroll
      for (int k = 0; k < NX; ++k) a = fma_t(bw[NX * NX + j * NX + k], l[k], a);
      dF[j] = a;
    }
  }
};
template <class M, class = void>
struct WaveSerialState : std::false_type {};
template <class M>
struct WaveSerialState<M, std::void_t<decltype(WaveOps<M>::SERIAL_STATE)>> : std::integral_constant<bool, WaveOps<M>::SERIAL_STATE> {};

// LDS of one wave: the table of the serial sweeps and two control rows for them (nothing else lives in memory)
template <class M, class T>
struct WaveLds {
  static constexpr int TAB_W = 2 * M::NX;  // per (sweep, stage): one pair (state component, trig value) per quad lane
  static __host__ __device__ int row_len(int dv) { return (dv * M::NU + 2) & ~1; }
  static __host__ __device__ int tab_len(int dv) { return (dv + 1) * TAB_W; }  // one sweep's table
  // region A: the tables of sweeps #1 / #2 — dead once the solve starts — and, over them, the Krylov basis of the kernels
  // that keep it in LDS ([vector][component][stage]); then the table of sweep #3 / of the serial fall-back, the two rows
  static __host__ __device__ int region_a(int dv, int kmax) {
    const int t = 2 * tab_len(dv), v = (kmax + 1) * M::NU * dv;
    return ((t > v ? t : v) + 1) & ~1;
  }
  // (models that are affine in x have no serial sweep and keep the basis in registers: only their own tables are in LDS)
  static __host__ __device__ size_t count_T(int dv, int kmax) {
    const size_t sweeps = WaveOps<M>::NONLINEAR ? size_t(region_a(dv, kmax)) + tab_len(dv) + 2 * row_len(dv) + 2 : 0;
    return sweeps + WaveOps<M>::LDS_EXTRA + 2;
  }
  static __host__ __device__ size_t bytes(int dv, int kmax, int waves) {
    return ((count_T(dv, kmax) * sizeof(T) + 15) & ~size_t(15)) * waves;
  }
};

}  // namespace cgm
