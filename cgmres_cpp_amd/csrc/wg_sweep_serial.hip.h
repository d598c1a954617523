// The horizon sweep of the serial-sweep "wg" kernels (full, fh_hbm and lean plans; also the preamble of the row-Newton
// kernel): members of WgCtx (wg_ctx.hip.h).
#pragma once
#include "wg_ctx.hip.h"

namespace cgm {

// ---- horizon sweep (cgmres.hpp:113-162; with PERT also :168-169, with MODE the post-processing) ------------
//   MODE F_PLAIN: out = F        F_RHS: out = (F*(1-zeta h) - Fh)/h  (:91-96)        F_AX: out = (F - Fh)/h  (:173-174)
//   PERT: u = U + h*W.  `out` may be W itself: every (stage, instance) entry of W is read for the last time in
//   phase 2 by the thread that then overwrites it.
// Three phases (see the header comment).  A stage table is dv*NSTG*IPW scalars indexed [(stage*NSTG + slot)*IPW + i];
// phase 1 writes x(s), trig(s) to `tab` — the LDS table S.R or, for the concurrent preamble sweeps, a per-workgroup
// table in HBM — phase 2 reads `tab` and leaves the costate coefficients in S.R, phase 3 consumes S.R.

// The Fh-in-HBM mode only exists in the long-vector instantiations (L > 160 is where LDS gets tight); the short ones
// compile it out, so the headline kernel carries none of its branches.
CGM_WGCTX_T
__device__ __forceinline__ bool CGM_WGCTX::fh_hbm() const { return LEAN || (MAXM > 10 && P.fh_hbm); }
// value of lane `src` (a lane of this wave) through the LDS crossbar
CGM_WGCTX_T
__device__ __forceinline__ double CGM_WGCTX::row_bcast(double v, int src) {
  const int lo = __builtin_amdgcn_ds_bpermute(src * 4, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(src * 4, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
CGM_WGCTX_T
__device__ __forceinline__ float CGM_WGCTX::row_bcast(float v, int src) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src * 4, __float_as_int(v)));
}
// Workgroup barrier that orders LDS only.  __syncthreads() also drains the wave's outstanding HBM traffic
// (s_waitcnt vmcnt(0)); inside a sweep nothing another wave needs travels through HBM.
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::lds_barrier() const {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// Phases 1 and 2 are pipelined in chunks of stages (f_eval): the sweep wave publishes a chunk of the stage table
// and goes on with the next one while the other waves turn the published chunk into costate coefficients.
// Chunks of ~25 stages measured best (round 2, after the coefficient phase moved to stage pairs: 2 chunks at dv = 50 —
// 1: -5 %, 3: -1.2 %, 4: -2.5 %, 5: -4 % — and 4 at dv = 100; round 1 had 4 at dv = 50): a barrier costs the sweep
// wave ~300 cycles, and only the processing of the last chunk stays on the critical path.
// SPLIT_TAIL (full plans with the quad sweep, 16 instances): the LAST pipeline chunk is what the costate sweep waits
// for after the state sweep, so it is kept at SPLIT_N = 12 stages — 192 (stage, instance) items, ONE per lane of the
// three coefficient waves (coeffs_chunked) instead of a stage pair per lane — and the first chunk takes the rest
// (its coefficients are computed in the shadow of the sweep's last chunk either way).
CGM_WGCTX_T
__device__ __forceinline__ int CGM_WGCTX::chunk_len() const {  // even: stages go in pairs
  if (SPLIT_TAIL && P.dv <= 64 && P.dv >= 2 * SPLIT_N) return (P.dv - SPLIT_N + 1) & ~1;
  const int chunks = P.dv <= 64 ? 2 : 4;
  return 2 * ((P.dv + 2 * chunks - 1) / (2 * chunks));
}

// phase 1: state sweep, cgmres.hpp:132-140, on the lanes [lane0, lane0 + 64) of one wave; x(dv) -> xT[c*IPW + i].
// PIPE: one lds_barrier() after every chunk (the caller's other waves run coeffs_chunked, which has the matching ones).
// ALT (quad sweep, pipelined only): x0 / x2 are stored at the first stage of every pair only (see M::x02_step)
CGM_WGCTX_T
template <bool PERT, bool PIPE, bool ALT>
__device__ __forceinline__ void CGM_WGCTX::sweep_state(int lane0, const T* x0c, T dtau, T* tab, T* xT, bool only_active) {
  constexpr int NX = M::NX, NU = M::NU, NC = M::NC;
  constexpr int STEP = TAB_STEP;
  const int dv = P.dv, lt = tid - lane0, CH = chunk_len();
  if (lt < 0 || lt >= 64) return;
  if constexpr (M::HAS_QUAD_SWEEP) {
    // four lanes (one DPP quad) per instance — see PendulumDev::quad_stage
    const int qi = lt >> 2;
    int rho = lt & 3;
    // Lean plan (256 registers per wave): keep the per-lane kernel coefficients from being hoisted to the kernel
    // entry — live across the whole tick they get spilled and every chunk of every sweep starts by waiting for
    // their scratch reloads (+5 k cycles per sweep); made opaque here they are ~12 selects per sweep call.
    if constexpr (LEAN) asm volatile("" : "+v"(rho));
    const bool goq = lt < 4 * IPW && blockIdx.x * IPW + qi < P.B && (!only_active || act_q);
    typename M::QuadLane Q;
    Q.init(rho, mc);
    // PERT: W holds U + h*direction (publish_direction).  Row-parallel Newton kernel: the first controls of every stage,
    // staged by the stage-owning lanes (so_publish_u0), one word per stage
    constexpr int US = ROW_NEWTON ? 1 : NU;
    const T* __restrict__ U = ROW_NEWTON ? so_stage(PERT ? 1 : 0) + qi * StageOwn::stage_pitch(P.dv)
                                         : (PERT || LEAN ? S.W : S.U) + qi * P.Lp;
    const T dtau1 = Q.sg * dtau;
    T x[NX], v = T(0), amax = T(0);
    if (goq) {
#pragma unroll
      for (int c = 0; c < NX; ++c) x[c] = x0c[c * IPW + qi];
      v = M::template quad_begin<false>(x, Q, mc, &amax);
    }
    // Branch-free stages, two per loop trip: all lanes store (see the slot map in models.hip.h), u0 of the next
    // stage is fetched one stage ahead (index dv*NU is the pad word of the odd-pitch row), and every table
    // pointer advances by the same constant so the second stage of a trip addresses with immediates.
    // table/control pointers and the prefetched u0 persist across chunks (only the slow redo rewinds them)
    T* pa = tab + qi;
    // the lane that holds +x1 stores it in the place of its own trig value (sin x1, which no later phase reads): one
    // select (2 instructions) instead of a second 8-byte LDS store (14.6 cycles) per stage
    const bool x1_lane = rho == M::QLANE_TRUE_X;
    T* pv = pa + Q.slot_v * IPW;
    const T* pu = U;
    T ua = T(0);
    if (goq) ua = pu[0];
    // Stage modes: 0 = trig value rotated from the previous stage (PendulumDev::quad_stage_rot), 1 = fresh evaluation
    // per stage (fast kernel), 2 = fresh evaluation with the library sin/cos.  A chunk runs at the
    // sweep's LEVEL (0: rotation, 1: fresh evaluations) and is redone one level up when an angle increment left the
    // rotation's range, in mode 2 when an argument left the fast kernel's range.  The level is kept from sweep to
    // sweep (rot_level: the perturbed sweeps of a tick and the ticks that follow see nearly the same increments —
    // without that memory a batch in fast motion paid for a failed rotation pass in EVERY sweep: 176 instead of 145
    // us/tick at tick 5500 of the seeded scenario, where the swing-up reaches 10 rad/s) and rotation is tried again
    // every ROT_HOLD sweeps.  (A third form — rotation with one more Taylor term per polynomial, good to 0.145 rad per
    // stage — was built and measured: its extra copy of the stage loop cost the slow regime 3.6 %; dropped.)
    constexpr int ROT_HOLD = 64;
    T argp = T(0);
    int zmax = 0;
    int lvl = __builtin_amdgcn_readfirstlane(rot_level);  // wave-uniform (kept in a scalar register)
    if (rot_hold == 0 && lvl > 0) lvl = 0, rot_hold = ROT_HOLD;
    auto run = [&](auto mode_tag, int n) {
      constexpr int MODE = decltype(mode_tag)::value;
      auto stage = [&](int o, T u0) {
        if (!ALT || (o & 1) == 0) {  // (o is a literal at every call site)
          pa[o * STEP + M::QSLOT_XA * IPW] = x[0];
          pa[o * STEP + M::QSLOT_XB * IPW] = x[2];
        }
        pv[o * STEP] = x1_lane ? x[1] : v;
        if constexpr (MODE == 0)
          M::quad_stage_rot(x, v, argp, u0, dtau, dtau1, Q, mc, &zmax);
        else
          M::template quad_stage<MODE == 2>(x, v, u0, dtau, dtau1, Q, mc, &amax);
      };
      int k = 0;
      if constexpr (MODE == 0) {  // rotation mode: four stages per trip (a taken branch costs ~30 cycles)
        for (; k + 4 <= n; k += 4) {
          const T ub = pu[US];
          stage(0, ua);
          const T uc = pu[2 * US];
          stage(1, ub);
          const T ud = pu[3 * US];
          stage(2, uc);
          ua = pu[4 * US];
          stage(3, ud);
          pa += 4 * STEP, pv += 4 * STEP, pu += 4 * US;
        }
      }
      for (; k + 2 <= n; k += 2) {
        const T ub = pu[US];
        stage(0, ua);
        ua = pu[2 * US];
        stage(1, ub);
        pa += 2 * STEP, pv += 2 * STEP, pu += 2 * US;
      }
      if (k < n) {  // odd tail: only the last chunk can have one (chunk_len() is even)
        stage(0, ua);
        pa += STEP, pv += STEP, pu += US;
      }
    };
    for (int s0 = 0; s0 < dv; s0 += CH) {
      const int n = dv - s0 < CH ? dv - s0 : CH;
      // (the level decisions are taken by ALL lanes of the wave, also those without an instance: the level stays
      // wave-uniform and the stage loops never run under a divergent branch)
      T xs[NX];
#pragma unroll
      for (int c = 0; c < NX; ++c) xs[c] = x[c];
      auto rewind = [&]() {
#pragma unroll
        for (int c = 0; c < NX; ++c) x[c] = xs[c];
        pa = tab + qi + s0 * STEP, pv = pa + Q.slot_v * IPW;
        pu = U + s0 * US;
        if (goq) ua = pu[0];
      };
      // v (and with it the rotation) is carried from the previous chunk / quad_begin; only a redo starts from a fresh
      // evaluation.  (Re-evaluating at every chunk start bounded the rotation's drift to one chunk — 26 stages at
      // dv = 50 — at ~40 instructions per chunk; over the whole horizon the drift stays five orders below the parity
      // bound, tests/test_gpu_parity.py.  126.8 -> 125.6 us/tick.)
      bool stale_v = false;
      bool done = false;
      if (lvl == 0) {
        if (goq) {
          if (stale_v) v = M::template quad_trig<false>(M::quad_arg(x, Q), Q, mc, &amax);
          argp = M::quad_arg(x, Q);
          run(std::integral_constant<int, 0>{}, n);
        }
        if (__builtin_expect(__any(goq && M::quad_rot_bad(zmax)), 0)) {  // an angle moved too far in one stage
          lvl = 1, rot_hold = ROT_HOLD, stale_v = true;
          rewind();
        } else {
          done = true;
        }
        zmax = 0;
      }
      if (__builtin_expect(!done, 0)) {
        if (goq) {
          if (stale_v) v = M::template quad_trig<false>(M::quad_arg(x, Q), Q, mc, &amax);
          run(std::integral_constant<int, 1>{}, n);
          if (n & 1) ua = pu[0];
        }
      }
      // an argument outside the fast range of the trig kernel: redo this chunk with the library sin/cos
      if (__builtin_expect(__any(goq && M::quad_arg_bad(amax)), 0)) {
        rewind();
        if (goq) {
          v = M::template quad_trig<true>(M::quad_arg(x, Q), Q, mc, &amax);
          run(std::integral_constant<int, 2>{}, n);
          if (n & 1) ua = pu[0];
        }
        amax = T(0);
      }
      if (PIPE) lds_barrier();
    }
    rot_level = lvl;
    if (rot_hold > 0) --rot_hold;
    if (goq && rho == M::QLANE_TRUE_X) {
#pragma unroll
      for (int c = 0; c < NX; ++c) xT[c * IPW + qi] = x[c];
    }
  } else {
    const int i = lt;
    const bool go = i < IPW && blockIdx.x * IPW + i < P.B && (!only_active || act_i);
    const T* __restrict__ U = (PERT || LEAN ? S.W : S.U) + i * P.Lp;  // (lean: W holds U for the unperturbed sweeps)
    T* __restrict__ R = tab + i;
    T xs[NX];
    if (go) {
#pragma unroll
      for (int c = 0; c < NX; ++c) xs[c] = x0c[c * IPW + i];
    }
    // Same loop shape as the quad sweep: two stages per trip, the controls of the next stage fetched one stage
    // ahead (the words after the last stage belong to the row's pad / the next row: in-bounds, unused), walking
    // pointers so the second stage of a trip addresses with immediates.
    struct Uc {
      T v[M::NU_DYN];
    };
    T* pr = R;
    const T* pu = U;
    auto fetch = [&](Uc& a, const T* q) {
#pragma unroll
      for (int j = 0; j < M::NU_DYN; ++j) a.v[j] = q[j];
    };
    auto stage = [&](const Uc& a, T* q, int sidx) {
      T f[NX], tr[NC > 0 ? NC : 1];
#pragma unroll
      for (int c = 0; c < NX; ++c) q[c * IPW] = xs[c];
      model_dxdt(f, xs, a.v, tr, i, sidx);
#pragma unroll
      for (int c = 0; c < NC; ++c) q[(M::TRIG_SLOT0 + c) * IPW] = tr[c];
#pragma unroll
      for (int c = 0; c < NX; ++c) xs[c] = f[c] * dtau + xs[c];
    };
    Uc ua, ub;
    if (go) fetch(ua, pu);
    for (int s0 = 0; s0 < dv; s0 += CH) {
      const int n = dv - s0 < CH ? dv - s0 : CH;
      if (go) {
        int k = 0;
        for (; k + 2 <= n; k += 2) {
          fetch(ub, pu + NU);
          stage(ua, pr, s0 + k);
          fetch(ua, pu + 2 * NU);
          stage(ub, pr + STEP, s0 + k + 1);
          pr += 2 * STEP, pu += 2 * NU;
        }
        if (k < n) {  // odd tail (last chunk only)
          stage(ua, pr, s0 + k);
          pr += STEP, pu += NU;
        }
      }
      if (PIPE) lds_barrier();
    }
    if (go) {
#pragma unroll
      for (int c = 0; c < NX; ++c) xT[c * IPW + i] = xs[c];
    }
  }
}

// phase 2: costate-free part of one backward stage of one instance.
// Reads x/trig from `tab`, writes the coefficients to S.R and the costate-free part of the result to `out`.
// Operands of an item that live in HBM/L2 — the parameter horizon in the lean plan, F(U,x+hf,t+h) with fh_hbm —
// are fetched for a whole group of items BEFORE the group is processed (and, behind the state sweep, before the
// barrier that releases the chunk): an item-by-item fetch exposes two dependent HBM/L2 round trips per item and
// the coefficient waves then fall behind the sweep wave (measured: +20 % on every sweep).
CGM_WGCTX_T
template <int MODE>
__device__ __forceinline__ void CGM_WGCTX::coeff_prefetch(CoeffPre& c, int s, int i) const {
  if constexpr (LEAN) {
#pragma unroll
    for (int j = 0; j < M::NP; ++j) c.p[j] = pTw[size_t(s * M::NP + j) * IPW + i];
  }
  if (MODE != F_PLAIN && fh_hbm()) {
    // explicitly global: left generic, hipcc merges this pointer with an LDS one and trips over the flat
    // aperture cast ("Illegal instruction detected ... $src_shared_base", ROCm 7.2)
    typedef const T __attribute__((address_space(1))) * GPtr;
    const GPtr row = reinterpret_cast<GPtr>(reinterpret_cast<uintptr_t>(P.Fh)) + size_t(S.binst[i]) * P.Lg + s * M::NU;
#pragma unroll
    for (int j = 0; j < M::NU; ++j) c.fh[j] = row[j];
  }
}
// x02: x0 and x2 of this stage when the table does not hold them (second stage of a pair, ALT_X02)
CGM_WGCTX_T
template <bool PERT, int MODE>
__device__ __forceinline__ void CGM_WGCTX::coeff_item(int s, int i, T dtau, const T* tab, T* out, const CoeffPre* pre,
                                                      const T* x02) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NC = M::NC, NBW = M::NBW;
  const T sc_phi = MODE == F_RHS ? P.one_m_zh : T(1.0);
  T x[NX], tr[NC > 0 ? NC : 1], u[NU], p[NP > 0 ? NP : 1], bw[NBW], phi[NU];
  const T* Rs = tab + tab_off(s) + i;
#pragma unroll
  for (int c = 0; c < NX; ++c) x[c] = Rs[c * IPW];
  if constexpr (ALT_X02) {
    if (x02) x[0] = x02[0], x[2] = x02[1];
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) tr[c] = Rs[(M::TRIG_SLOT0 + c) * IPW];
#pragma unroll
  for (int j = 0; j < NU; ++j) u[j] = (PERT || LEAN ? S.W : S.U)[i * P.Lp + s * NU + j];
#pragma unroll
  for (int j = 0; j < NP; ++j) p[j] = (LEAN && pre) ? pre->p[j] : get_p(i, s * NP + j);
  M::stage_coeffs(bw, phi, x, u, p, tr, dtau);
  // coefficients go back pair-interleaved — pair c of instance i at [(c*IPW + i)*2, +1] of the stage's region —
  // so the costate sweep fetches them with 16-byte LDS reads (ds_read_b128: 8 cycles; ds_read2_b64: 16).  In place
  // is safe: the 16 instances of a stage are 16 adjacent lanes of ONE wave in ONE pass, and all their reads of
  // x/trig precede these writes in program order.
  static_assert(NBW % 2 == 0 && (IPW * 16) % 64 == 0, "pair-interleaved costate coefficients");
  {
    Pair* Rp = reinterpret_cast<Pair*>(S.R + tab_off(s)) + i;
#pragma unroll
    for (int c = 0; c < NBW; c += 2) Rp[(c / 2) * IPW] = Pair{bw[c], bw[c + 1]};
  }
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    T rj = phi[j];
    if (MODE != F_PLAIN) {
      // two loads from two address spaces, selected by VALUE (a select of the pointers would have to go through
      // the flat aperture); with fh_hbm the LDS word read is a word of W and is not used
      T fh;
      if constexpr (LEAN) {
        fh = pre->fh[j];
      } else {
        fh = S.Fh[i * P.Lp + s * NU + j];
        if (fh_hbm()) fh = pre->fh[j];
      }
      rj = (rj * sc_phi - fh) * P.inv_h;
    }
    out[i * P.Lp + s * NU + j] = rj;
  }
}
// all threads, items (s, i) with i fastest
// (i = tid mod IPW at every call site: the instance index of an item advances in steps that are multiples of IPW)
CGM_WGCTX_T
__device__ __forceinline__ bool CGM_WGCTX::item_on(int i, bool only_active) const {
  return blockIdx.x * IPW + i < P.B && (!only_active || act_i);
}
// items q0, q0 + stride, ... (COEFF_GROUP of them) of the range [0, n_items), stage offset s0: fetch, `between`, compute
CGM_WGCTX_T
template <bool PERT, int MODE, class Between>
__device__ __forceinline__ void CGM_WGCTX::coeff_group(int q0, int stride, int n_items, int s0, T dtau, const T* tab, T* out,
                                                       bool only_active, Between&& between) {
  CoeffPre pre[COEFF_GROUP];
#pragma unroll
  for (int g = 0; g < COEFF_GROUP; ++g) {
    const int q = q0 + g * stride, i = q & (IPW - 1);
    if (q < n_items && item_on(i, only_active)) coeff_prefetch<MODE>(pre[g], s0 + q / IPW, i);
  }
  between();
#pragma unroll
  for (int g = 0; g < COEFF_GROUP; ++g) {
    const int q = q0 + g * stride, i = q & (IPW - 1);
    if (q < n_items && item_on(i, only_active)) coeff_item<PERT, MODE>(s0 + q / IPW, i, dtau, tab, out, &pre[g]);
  }
}
// the same for items = (stage pair, instance) of the stages [s0, s_end) of the LDS table (ALT_X02): the second stage
// of a pair takes x0 / x2 from M::x02_step instead of the table
CGM_WGCTX_T
template <bool PERT, int MODE, class Between>
__device__ __forceinline__ void CGM_WGCTX::coeff_group_pairs(int q0, int stride, int s0, int s_end, T dtau, T* out,
                                                             bool only_active, Between&& between) {
  const int n_items = ((s_end - s0 + 1) >> 1) * IPW;
  CoeffPre pre[COEFF_GROUP][2];
#pragma unroll
  for (int g = 0; g < COEFF_GROUP; ++g) {
    const int q = q0 + g * stride, i = q & (IPW - 1), s = s0 + 2 * (q / IPW);
    if (q < n_items && item_on(i, only_active)) {
      coeff_prefetch<MODE>(pre[g][0], s, i);
      if (s + 1 < s_end) coeff_prefetch<MODE>(pre[g][1], s + 1, i);
    }
  }
  between();
#pragma unroll
  for (int g = 0; g < COEFF_GROUP; ++g) {
    const int q = q0 + g * stride, i = q & (IPW - 1), s = s0 + 2 * (q / IPW);
    if (q < n_items && item_on(i, only_active)) {
      T x02[2] = {S.R[tab_off(s, M::QSLOT_XA) + i], S.R[tab_off(s, M::QSLOT_XB) + i]};
      const T u0 = (PERT || LEAN ? S.W : S.U)[i * P.Lp + s * M::NU];
      coeff_item<PERT, MODE>(s, i, dtau, S.R, out, &pre[g][0]);
      if (s + 1 < s_end) {
        M::x02_step(x02[0], x02[1], u0, dtau);
        coeff_item<PERT, MODE>(s + 1, i, dtau, S.R, out, &pre[g][1], x02);
      }
    }
  }
}
CGM_WGCTX_T
template <bool PERT, int MODE>
__device__ __forceinline__ void CGM_WGCTX::sweep_coeffs(T dtau, const T* tab, T* out, bool only_active) {
  if constexpr (HBM_OPERANDS) {
    for (int q0 = tid; q0 < P.dv * IPW; q0 += IPW * 16 * COEFF_GROUP)
      coeff_group<PERT, MODE>(q0, IPW * 16, P.dv * IPW, 0, dtau, tab, out, only_active, [] {});
  } else {
    for (int q = tid; q < P.dv * IPW; q += IPW * 16) {
      const int i = q & (IPW - 1), s = q / IPW;
      if (!item_on(i, only_active)) continue;
      coeff_item<PERT, MODE>(s, i, dtau, tab, out);
    }
  }
}
// the waves other than wave 0, chunk by chunk behind sweep_state<PERT, true> (one lds_barrier() before every chunk)
CGM_WGCTX_T
template <bool PERT, int MODE>
__device__ __forceinline__ void CGM_WGCTX::coeffs_chunked(T dtau, T* out, bool only_active) {
  constexpr int NL = IPW * 16 - 64;
  const int dv = P.dv, CH = chunk_len(), lt = tid - 64;
  for (int s0 = 0; s0 < dv; s0 += CH) {
    const int n = dv - s0 < CH ? dv - s0 : CH;
    if constexpr (HBM_OPERANDS && ALT_X02) {
      coeff_group_pairs<PERT, MODE>(lt, NL, s0, s0 + n, dtau, out, only_active, [&] { lds_barrier(); });
      for (int q0 = lt + NL * COEFF_GROUP; q0 < ((n + 1) >> 1) * IPW; q0 += NL * COEFF_GROUP)
        coeff_group_pairs<PERT, MODE>(q0, NL, s0, s0 + n, dtau, out, only_active, [] {});
    } else if constexpr (HBM_OPERANDS) {
      // the first group's HBM operands are requested BEFORE the barrier, i.e. while the sweep wave still works on
      // this chunk (every thread reaches the barrier exactly once per chunk, with or without items)
      coeff_group<PERT, MODE>(lt, NL, n * IPW, s0, dtau, S.R, out, only_active, [&] { lds_barrier(); });
      for (int q0 = lt + NL * COEFF_GROUP; q0 < n * IPW; q0 += NL * COEFF_GROUP)
        coeff_group<PERT, MODE>(q0, NL, n * IPW, s0, dtau, S.R, out, only_active, [] {});
    } else if constexpr (ALT_X02) {
      lds_barrier();
      if (SPLIT_TAIL && n <= SPLIT_N) {
        // One STAGE per lane: lanes 0-31 of a wave take the first stages of two pairs, lanes 32-63 their second stages
        // (which re-derive x0 / x2 from the pair's first stage like the pair items do).  The coefficients of a stage
        // overwrite its slots in place, and a second-stage lane reads two slots of the FIRST stage: both lanes sit in
        // the same wave and every read below precedes every write in program order (straight-line code, no branch
        // between the halves; a wave's LDS operations complete in order).
        const int l = lt & 63, i = l & (IPW - 1), half = l >> 5;
        const int ps = s0 + 2 * (2 * (lt >> 6) + ((l >> 4) & 1)), st = ps + half;
        if (st < s0 + n && item_on(i, only_active)) {
          T x02[2] = {S.R[tab_off(ps, M::QSLOT_XA) + i], S.R[tab_off(ps, M::QSLOT_XB) + i]};
          const T u0 = (PERT || LEAN ? S.W : S.U)[i * P.Lp + ps * M::NU];
          T x0n = x02[0], x2n = x02[1];
          M::x02_step(x0n, x2n, u0, dtau);
          if (half) x02[0] = x0n, x02[1] = x2n;
          coeff_item<PERT, MODE>(st, i, dtau, S.R, out, nullptr, x02);
        }
        continue;
      }
      for (int q = lt; q < ((n + 1) >> 1) * IPW; q += NL) {  // items = (stage pair, instance)
        const int i = q & (IPW - 1), s = s0 + 2 * (q / IPW);
        if (!item_on(i, only_active)) continue;
        T x02[2] = {S.R[tab_off(s, M::QSLOT_XA) + i], S.R[tab_off(s, M::QSLOT_XB) + i]};
        const T u0 = (PERT || LEAN ? S.W : S.U)[i * P.Lp + s * M::NU];
        coeff_item<PERT, MODE>(s, i, dtau, S.R, out);
        if (s + 1 < s0 + n) {
          M::x02_step(x02[0], x02[1], u0, dtau);
          coeff_item<PERT, MODE>(s + 1, i, dtau, S.R, out, nullptr, x02);
        }
      }
    } else {
      lds_barrier();
      for (int q = lt; q < n * IPW; q += NL) {
        const int i = q & (IPW - 1), s = s0 + q / IPW;
        if (!item_on(i, only_active)) continue;
        coeff_item<PERT, MODE>(s, i, dtau, S.R, out);
      }
    }
  }
}

// phase 3: costate sweep (cgmres.hpp:145-153) + the costate part of dH/du (:156-161).  COLLECTIVE (every thread
// calls it); the caller adds the barrier that publishes `out`.
CGM_WGCTX_T
template <int MODE>
__device__ __forceinline__ void CGM_WGCTX::sweep_costate(T dtau, const T* xT, T* out, bool only_active) {
  if constexpr (PAR_COSTATE) {
    sweep_costate_par<MODE>(dtau, xT, out, only_active);
  } else if constexpr (PAR_2PASS) {
    sweep_costate_2pass<MODE>(dtau, xT, out, only_active);
  } else {
    if (!(sweep_lane && (!only_active || act_i))) return;
    T l[M::NX];
    costate_run<MODE, false, true>(l, tid, P.dv - 1, P.dv, dtau, S.R + 2 * tid, out + tid * P.Lp,
                             [&](T* l0) { costate_terminal(l0, xT, tid); });
  }
}
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::costate_terminal(T* l, const T* xT, int i) const {
  T xs[M::NX], p[M::NP > 0 ? M::NP : 1];
#pragma unroll
  for (int c = 0; c < M::NX; ++c) xs[c] = xT[c * IPW + i];
#pragma unroll
  for (int j = 0; j < M::NP; ++j) p[j] = get_p(i, P.dv * M::NP + j);
  M::dPhidx(l, xs, p);
}
// `count` (workgroup-uniform) stages hi, hi-1, ... of the recurrence on this lane, from l.
//   HOM = false: the affine stage; coefficients from `coef` (this instance's pairs of stage 0), the costate part of
//                dH/du is added to the row `orow`: orow[s*NU + j] += sc*dF[j]
//   HOM = true:  the bias-free stage on the first NBW_LIN coefficients; dF itself goes to orow[(s*NUL + j)*HL]
// One wave issues one instruction per ~4.4 cycles whatever it is (tools/ubench_issue.hip), so the loop is written
// for instruction count: moving pointers with immediate offsets, no branch inside a trip, unconditional look-ahead
// fetches.
//   After the `count` common stages, lanes with `more` set go on for `extra` (workgroup-uniform, 0..3) stages; the
//   first two of those use operands the look-ahead has fetched anyway.  `init` fills l; it is called after the first
//   operand requests have been issued so that its own LDS reads share their round trip.
//   WRITE = false: only the end value of l is wanted (first pass of sweep_costate_2pass): no output traffic at all.
CGM_WGCTX_T
template <int MODE, bool HOM, bool WRITE, class Init>
__device__ __forceinline__ void CGM_WGCTX::costate_run(T* l, int i, int hi, int count, T dtau, const T* coef, T* orow, Init&& init,
                                                       int extra, bool more) {
  constexpr int NU = M::NU, NBW = M::NBW, NUL = M::NUL;
  constexpr int NLOAD = HOM ? M::NBW_LIN : NBW;  // coefficients fetched per stage
  constexpr int OJ = HOM ? HL : 1;               // distance between the NUL outputs of a stage
  constexpr int opitch = HOM ? NUL * HL : NU;    // and between stages
  static_assert(NLOAD % 2 == 0, "coefficients are fetched in pairs");
  const T sc = MODE == F_PLAIN ? T(1.0) : (MODE == F_RHS ? P.one_m_zh * P.inv_h : P.inv_h);
  constexpr int STEP = TAB_STEP;
  struct Ops {
    T bw[NBW], o[NUL];
  };
  auto fetch = [&](Ops& a, const T* pr, const T* po) {
    const Pair* pp = reinterpret_cast<const Pair*>(pr);
#pragma unroll
    for (int c = 0; c < NLOAD; c += 2) {
      const Pair t = pp[(c / 2) * IPW];
      a.bw[c] = t.a, a.bw[c + 1] = t.b;
    }
    if constexpr (!HOM && WRITE) {
#pragma unroll
      for (int j = 0; j < NUL; ++j) a.o[j] = po[j * OJ];
    }
  };
  auto stage = [&](const Ops& a, T* po) {
    T dF[NUL];
    M::template costate_step<HOM>(l, dF, a.bw, dtau);
    if constexpr (WRITE) {
#pragma unroll
      for (int j = 0; j < NUL; ++j) po[j * OJ] = HOM ? dF[j] : a.o[j] + dF[j] * sc;
    }
  };
  // Three register sets, three stages per trip: the operands of stage t-2 are requested while stage t computes
  // (two LDS latencies of slack).  q/o sit on stage s-4 of the trip that starts with stage s: every access is
  // pointer + non-negative immediate.  Below stage 0 the look-ahead reads words of the preceding LDS arrays
  // (at most 3 stages = 3*STEP scalars — the `post` tail below — which WgTraits::lookahead_fits (wg_plan.hip.h) guarantees to lie
  // inside the row arrays in front of the table), never used.  LDS accesses outside the workgroup's allocation
  // FAULT on this platform (aperture violation): -DCGM_DEBUG_LDS checks every address here.
#ifdef CGM_DEBUG_LDS
  auto chk = [&](const void* ptr, int what) {  // (a flag, not a printf: 40 printf sites made this build take 20 minutes)
    const long off = static_cast<const char*>(ptr) - reinterpret_cast<const char*>(LEAN ? S.xs : S.U);
    if (off < 0 || off + 16 > long(P.lds_bytes)) g_cgm_lds_oob = 0x10000 | (what << 12) | (tid & 0xfff);
  };
#else
  auto chk = [&](const void*, int) {};
#endif
  auto fetch3 = [&](Ops& a, const T* pr3, const T* po3) {
    if (NLOAD) chk(pr3, 1), chk(pr3 + (NLOAD / 2 - 1) * 2 * IPW, 2);
    if (!HOM && WRITE) chk(po3, 3);
    fetch(a, pr3, po3);
  };
  auto stage3 = [&](const Ops& a, T* po3) {
    if (WRITE) chk(po3, 4);
    stage(a, po3);
  };
  Ops A, B, C;
  int rem = count;
  const T* q = coef + (hi - 4) * STEP;  // pair-interleaved coefficients, see coeff_item
  T* o = orow + (hi - 4) * opitch;
  fetch3(A, q + 4 * STEP, o + 4 * opitch);  // stage hi
  fetch3(B, q + 3 * STEP, o + 3 * opitch);  // stage hi-1
  init(l);
  if (!HOM && WRITE && PAR_COSTATE) CGM_STAMP(*this, 18);
  for (; rem >= 3; rem -= 3) {
    fetch3(C, q + 2 * STEP, o + 2 * opitch);
    stage3(A, o + 4 * opitch);
    fetch3(A, q + STEP, o + opitch);
    stage3(B, o + 3 * opitch);
    fetch3(B, q, o);
    stage3(C, o + 2 * opitch);
    q -= 3 * STEP, o -= 3 * opitch;
  }
  if (!HOM && WRITE && PAR_COSTATE) CGM_STAMP(*this, 19);
  // the last rem (0..2) common stages, then the extra ones of the lanes with `more`: A and B hold the next two
  const int post = rem + extra;  // <= 5
  if (post > 2) fetch3(C, q + 2 * STEP, o + 2 * opitch);
  if (post >= 1 && (rem >= 1 || more)) stage3(A, o + 4 * opitch);
  if (post > 3) fetch3(A, q + STEP, o + opitch);
  if (post >= 2 && (rem >= 2 || more)) stage3(B, o + 3 * opitch);
  if (post > 4) fetch3(B, q, o);
  if (post >= 3 && more) stage3(C, o + 2 * opitch);
  if (post >= 4 && more) stage3(A, o + opitch);
  if (post >= 5 && more) stage3(B, o);
  if (!HOM && WRITE && PAR_COSTATE) CGM_STAMP(*this, 20);
}

// The costate recurrence is AFFINE in l once the stage coefficients are stored (l' = M_s l + b_s, dF_s = B_s l), so
// the horizon is cut into four chunks that run SIDE BY SIDE on the four waves instead of one lane per instance
// walking all dv stages:
//   chunk 0 (the last stages: its start value, the terminal costate, is known) is run directly;
//   chunks 1..3 are run from l = 0 WITH the bias (particular solution; wave 0, one lane per instance and chunk — it
//   writes o + sc*dF_particular to `out` like the direct lane) and from the NX unit vectors WITHOUT it (wave k:
//   column c of the chunk's transfer matrix on lane c*IPW + i, its dF per stage into the scratch Hd);
//   then l at the chunk boundaries follows from two small matrix-vector products (wave 0) and the homogeneous part
//   of dF, sum_c l_c(start of chunk) * Hd[stage][c], is added to `out` by all threads (one (stage, instance) each).
// dv stage-times of one wave become dv/4 + the remainder + ~2 short parallel phases; the result differs from the
// sequential recurrence by rounding only (~1e-16 relative to |l|; tests/test_gpu_parity.py bounds it against the oracle).
CGM_WGCTX_T
template <int MODE>
__device__ __forceinline__ void CGM_WGCTX::sweep_costate_par(T dtau, const T* xT, T* out, bool only_active) {
  constexpr int NX = M::NX, NU = M::NU, NUL = M::NUL;
  static_assert(NX % 2 == 0, "boundary records are read in pairs");
  const int dv = P.dv, n = dv >> 2, n0 = dv - 3 * n;  // chunk k >= 1: stages [(3-k)n, (4-k)n); chunk 0: [3n, dv)
  const T sc = MODE == F_PLAIN ? T(1.0) : (MODE == F_RHS ? P.one_m_zh * P.inv_h : P.inv_h);
  T* Hd = S.scan;                             // [stage < 3n][j < NUL][c*IPW + i]
  T* Rec = Hd + 3 * n * NUL * HL;             // boundary records [k < 3][i][REC], see scan_count
  constexpr int REC = Lds::SCAN_REC;
  // every address below derives from the thread index and is invariant over ticks and Arnoldi iterations: left
  // visible, the compiler hoists those computations to the top of the kernel and keeps ~20 more values alive over the
  // whole tick loop (they end up in scratch, reloaded behind s_waitcnt vmcnt(0))
  int tid_o = tid;
  asm volatile("" : "+v"(tid_o));
  const int wave = tid_o >> 6, lane = tid_o & 63;
  // --- phase A: all chunks side by side
  if (wave == 0) {
    const int i = lane & (IPW - 1), k = lane >> 4;
    if (item_on(i, only_active)) {
      T l[NX];
      const int hi = k == 0 ? dv - 1 : (4 - k) * n - 1;
      costate_run<MODE, false, true>(l, i, hi, n, dtau, S.R + 2 * i, out + i * P.Lp,
                               [&](T* l0) {
                                 costate_terminal(l0, xT, i);
                                 if (k != 0) {
#pragma unroll
                                   for (int c = 0; c < NX; ++c) l0[c] = T(0);
                                 }
                               },
                               n0 - n, k == 0);
      // chunk 0: its end value = the start value of chunk 1, record 0; chunk k >= 1: particular end value, record k
      // (chunk 3's is never read and goes to the spare record)
      T* dst = Rec + (k * IPW + i) * REC + NX * NX;
#pragma unroll
      for (int c = 0; c < NX; ++c) dst[c] = l[c];
    }
  } else if (lane < HL) {
    const int i = lane & (IPW - 1), c0 = lane / IPW, k = wave;
    if (item_on(i, only_active)) {
      T l[NX];
      costate_run<MODE, true, true>(l, i, (4 - k) * n - 1, n, dtau, S.R + 2 * i, Hd + lane, [&](T* l0) {
#pragma unroll
        for (int c = 0; c < NX; ++c) l0[c] = c == c0 ? T(1) : T(0);
      });
#pragma unroll
      for (int r = 0; r < NX; ++r) Rec[(k * IPW + i) * REC + r * NX + c0] = l[r];  // column c0 of the transfer matrix
    }
  }
  CGM_STAMP(*this, 16);
  lds_barrier();
  CGM_STAMP(*this, 17);
  // --- phase B, all threads, no further barrier.  Every LDS instruction costs its issuing wave 7..16 cycles (tools/
  //     ubench_lds.hip), so the work is dealt by WAVE such that nobody reads a boundary record it does not need:
  //       wave 0: the stages of chunk 1 — start value = record 0, no product;
  //       wave 1: chunk 2 — one NX x NX product, l(start of chunk 2) = p_1 + M_1 l(start of chunk 1);
  //       waves 2, 3: chunk 3 — two products, l(start of chunk 3) = p_2 + M_2 l(start of chunk 2);
  //     (redundantly in every thread of the wave, which is cheaper than a third barrier), then
  //     out[stage] += sc * sum_c l_c(start of the chunk) * Hd[stage][c] for the thread's stages j, j + stride, ...
  {
    const int w = __builtin_amdgcn_readfirstlane(wave);  // (scalar: the branches below are wave-uniform)
    const int k = w < 2 ? w + 1 : 3;
    const int i = lane & (IPW - 1);
    const int j0 = w < 3 ? lane >> 4 : 4 + (lane >> 4), stride = w < 2 ? 4 : 8;
    const Pair* rec = reinterpret_cast<const Pair*>(Rec + i * REC);  // (REC is even: records are 16-byte aligned)
    constexpr int RP = REC / 2, KP = IPW * RP;                      // pairs per record, per chunk
    T al[NX];
#pragma unroll
    for (int c = 0; c < NX; c += 2) {
      const Pair t = rec[(NX * NX + c) / 2];
      al[c] = t.a, al[c + 1] = t.b;
    }
    auto advance = [&](int kk) {  // al <- p_kk + M_kk al
      T m[NX * NX], nx[NX];
#pragma unroll
      for (int e = 0; e < NX * NX; e += 2) {
        const Pair t = rec[kk * KP + e / 2];
        m[e] = t.a, m[e + 1] = t.b;
      }
#pragma unroll
      for (int c = 0; c < NX; c += 2) {
        const Pair t = rec[kk * KP + (NX * NX + c) / 2];
        nx[c] = t.a, nx[c + 1] = t.b;
      }
#pragma unroll
      for (int rr = 0; rr < NX; ++rr) {
#pragma unroll
        for (int c = 0; c < NX; ++c) nx[rr] = fma_t(m[rr * NX + c], al[c], nx[rr]);
      }
#pragma unroll
      for (int c = 0; c < NX; ++c) al[c] = nx[c];
    };
    if (k >= 2) advance(1);
    // one record in registers at a time: with both in flight the allocation of the Arnoldi loop tips into scratch
    __builtin_amdgcn_sched_barrier(0);
    if (k >= 3) advance(2);
    if (item_on(i, only_active)) {
      const int base = (3 - k) * n;
      for (int j = j0; j < n; j += stride) {
        const int s = base + j;
#pragma unroll
        for (int jj = 0; jj < NUL; ++jj) {
          T acc = T(0);
#pragma unroll
          for (int c = 0; c < NX; ++c) acc = fma_t(al[c], Hd[(s * NUL + jj) * HL + c * IPW + i], acc);
          T* po = out + i * P.Lp + s * NU + jj;
          *po = fma_t(acc, sc, *po);
        }
      }
    }
  }
}

// The chunk-parallel sweep WITHOUT per-stage scratch, for the plans whose LDS has no room for it (lean, long vectors):
// the horizon is cut into C = P.cs_chunks (3 or 4) chunks of n = dv/C stages (chunk 0, the LAST part of the horizon,
// takes the remainder) and walked twice —
//   pass 1 (no output traffic at all): wave 0, lane (k, i): chunk 0 from the terminal costate — its end value is the
//          start value of chunk 1 — and chunks 1 .. C-2 from l = 0 with the bias (particular end value p_k); waves 1..:
//          chunks 1 .. C-2 from the NX unit vectors without the bias (transfer matrix M_k).  The last chunk of the walk
//          (the first stages) needs neither: nobody continues from its end;
//   one barrier;
//   pass 2: wave 0, lane (k, i): l(start of chunk k) = p_(k-1) + M_(k-1) l(start of chunk k-1) (at most two small
//          products, redundantly per lane), then the chunk for real: o + sc*dF to `out` like the serial sweep.
// One wave walks 2n instead of dv stages, both times alone at the LDS pipe; the scratch is 4 + (C-2)*22 scalars per
// instance.  Same arithmetic per stage as the serial sweep; what differs is that l enters a chunk as p + M l_start
// instead of through the stages before it (rounding level, bounded against the oracle by the tests).
CGM_WGCTX_T
template <int MODE>
__device__ __forceinline__ void CGM_WGCTX::sweep_costate_2pass(T dtau, const T* xT, T* out, bool only_active) {
  constexpr int NX = M::NX;
  constexpr int REC = Lds::SCAN_REC;
  static_assert(NX % 2 == 0, "boundary records are read in pairs");
  const int C = P.cs_chunks, dv = P.dv, n = dv / C, n0 = dv - (C - 1) * n;  // chunk k >= 1: stages [(C-1-k)n, (C-k)n)
  T* Vec0 = S.scan;              // [i][NX]
  T* Rec = Vec0 + IPW * NX;      // [k-1][i][REC], k = 1 .. C-2
  int tid_o = tid;               // (opaque: see sweep_costate_par)
  asm volatile("" : "+v"(tid_o));
  const int wave = tid_o >> 6, lane = tid_o & 63;
  // ---- pass 1
  if (wave == 0) {
    const int i = lane & (IPW - 1), k = lane >> 4;
    if (k < C - 1 && item_on(i, only_active)) {
      T l[NX];
      costate_run<MODE, false, false>(l, i, k == 0 ? dv - 1 : (C - k) * n - 1, n, dtau, S.R + 2 * i, out + i * P.Lp,
                                      [&](T* l0) {
                                        costate_terminal(l0, xT, i);
                                        if (k != 0) {
#pragma unroll
                                          for (int c = 0; c < NX; ++c) l0[c] = T(0);
                                        }
                                      },
                                      n0 - n, k == 0);
      T* dst = k == 0 ? Vec0 + i * NX : Rec + ((k - 1) * IPW + i) * REC + NX * NX;
#pragma unroll
      for (int c = 0; c < NX; ++c) dst[c] = l[c];
    }
  } else {
    const int q = tid_o - 64, g = q / HL, ql = q - g * HL, i = ql & (IPW - 1), c0 = ql / IPW;  // chunk g + 1, column c0
    if (g < C - 2 && item_on(i, only_active)) {
      T l[NX];
      costate_run<MODE, true, false>(l, i, (C - 1 - g) * n - 1, n, dtau, S.R + 2 * i, out, [&](T* l0) {
#pragma unroll
        for (int c = 0; c < NX; ++c) l0[c] = c == c0 ? T(1) : T(0);
      });
#pragma unroll
      for (int r = 0; r < NX; ++r) Rec[(g * IPW + i) * REC + r * NX + c0] = l[r];
    }
  }
  CGM_STAMP(*this, 16);
  lds_barrier();
  CGM_STAMP(*this, 17);
  // ---- pass 2
  if (wave == 0) {
    const int i = lane & (IPW - 1), k = lane >> 4;
    if (k < C && item_on(i, only_active)) {
      T l[NX];
      costate_run<MODE, false, true>(l, i, k == 0 ? dv - 1 : (C - k) * n - 1, n, dtau, S.R + 2 * i, out + i * P.Lp,
                                     [&](T* l0) {
                                       if (k == 0) {
                                         costate_terminal(l0, xT, i);
                                       } else {
                                         const Pair* v0 = reinterpret_cast<const Pair*>(Vec0 + i * NX);
#pragma unroll
                                         for (int c = 0; c < NX; c += 2) {
                                           const Pair t = v0[c / 2];
                                           l0[c] = t.a, l0[c + 1] = t.b;
                                         }
                                         for (int kk = 1; kk < k; ++kk) {  // l0 <- p_kk + M_kk l0
                                           const Pair* rec = reinterpret_cast<const Pair*>(Rec + ((kk - 1) * IPW + i) * REC);
                                           T m[NX * NX], nx[NX];
#pragma unroll
                                           for (int e = 0; e < NX * NX; e += 2) {
                                             const Pair t = rec[e / 2];
                                             m[e] = t.a, m[e + 1] = t.b;
                                           }
#pragma unroll
                                           for (int c = 0; c < NX; c += 2) {
                                             const Pair t = rec[(NX * NX + c) / 2];
                                             nx[c] = t.a, nx[c + 1] = t.b;
                                           }
#pragma unroll
                                           for (int rr = 0; rr < NX; ++rr) {
#pragma unroll
                                             for (int c = 0; c < NX; ++c) nx[rr] = fma_t(m[rr * NX + c], l0[c], nx[rr]);
                                           }
#pragma unroll
                                           for (int c = 0; c < NX; ++c) l0[c] = nx[c];
                                         }
                                       }
                                     },
                                     n0 - n, k == 0);
    }
  }
}

// One complete sweep on the LDS table.  COLLECTIVE: every thread of the block must call it (two workgroup barriers
// inside); the caller adds the barrier that publishes `out`.  x0c = initial state, component-major LDS [c*IPW + i].
// `after_sweep` runs on the sweep wave right after its state sweep, i.e. while it would otherwise wait for the other
// waves to finish the last coefficient chunk (gmres() requests its basis rows there); the barrier that follows
// orders LDS only so those loads stay in flight during the costate sweep.
// `idle_work` runs on the other waves BEFORE their first chunk barrier, i.e. while they would wait for the sweep wave
// to finish the first chunk of stages (gmres() does the previous iteration's Hessenberg column there).
CGM_WGCTX_T
template <bool PERT, int MODE, class After, class Idle>
__device__ __forceinline__ void CGM_WGCTX::f_eval(const T* x0c, T dtau, T* out, bool only_active, After&& after_sweep,
                                                  Idle&& idle_work) {
  if constexpr (IPW * 16 >= 128) {
    if (tid < 64) {
      sweep_state<PERT, true, ALT_X02>(0, x0c, dtau, S.R, S.xT, only_active);
      after_sweep();
    } else {
      idle_work();
      coeffs_chunked<PERT, MODE>(dtau, out, only_active);
    }
    CGM_STAMP(*this, 4);
    lds_barrier();
    CGM_STAMP(*this, 5);
    sweep_costate<MODE>(dtau, S.xT, out, only_active);
  } else {
    idle_work();
    f_eval<PERT, MODE>(x0c, dtau, out, only_active);
    if (tid < 64) after_sweep();
  }
}
CGM_WGCTX_T
template <bool PERT, int MODE>
__device__ __forceinline__ void CGM_WGCTX::f_eval(const T* x0c, T dtau, T* out, bool only_active) {
  if constexpr (IPW * 16 >= 128) {
    if (tid < 64)
      sweep_state<PERT, true, ALT_X02>(0, x0c, dtau, S.R, S.xT, only_active);
    else
      coeffs_chunked<PERT, MODE>(dtau, out, only_active);
    CGM_STAMP(*this, 4);
    __syncthreads();
  } else {
    sweep_state<PERT, false>(0, x0c, dtau, S.R, S.xT, only_active);
    __syncthreads();
    CGM_STAMP(*this, 4);
    sweep_coeffs<PERT, MODE>(dtau, S.R, out, only_active);
    __syncthreads();
  }
  CGM_STAMP(*this, 5);
  sweep_costate<MODE>(dtau, S.xT, out, only_active);
}

// cgmres.hpp:83-85 on the sweep lanes: x_dxh = x + h*f(x, U0)
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::make_xh() {
  if (!sweep_lane) return;
  constexpr int NX = M::NX;
  const int i = tid;
  T x[NX], u0[M::NU], f[NX], tr[M::NC > 0 ? M::NC : 1];
#pragma unroll
  for (int c = 0; c < NX; ++c) x[c] = S.xs[c * IPW + i];
#pragma unroll
  for (int j = 0; j < M::NU; ++j) u0[j] = ROW_NEWTON ? so_unow()[j * IPW + i] : (LEAN ? S.W : S.U)[i * P.Lp + j];  // (lean: call after publish_U)
  model_dxdt(f, x, u0, tr, i, 0);
#pragma unroll
  for (int c = 0; c < NX; ++c) S.xh[c * IPW + i] = f[c] * P.h + x[c];
}
// The three sweeps control() needs before the Arnoldi loop are independent of each other
//     #1 Fh  = F(U, x_dxh, t+h)              cgmres.hpp:88
//     #2 b   = (F(U, x, t)(1-zeta h) - Fh)/h   :91-96
//     #3 Ax0 = (F(U + h dUdt, x_dxh, t+h) - Fh)/h   :99 -> gmres.hpp:33 (only when WITH_AX0; W must hold dUdt)
// so their state sweeps — the long serial phase — run CONCURRENTLY on waves 0, 1, 2; #1 uses the LDS stage table,
// #2/#3 park theirs in this workgroup's HBM scratch (written once, read once by the parallel coefficient phase).
// Results: Fh in S.Fh; b and Ax0 delivered in registers (row layout) because both pass through S.W.
// COLLECTIVE; needs at least 3 waves (falls back to sequential sweeps otherwise).
CGM_WGCTX_T
template <bool WITH_AX0>
__device__ __forceinline__ void CGM_WGCTX::preamble(T* bb, T* ax0, const T* dir) {  // dir: registers of the W direction
  if constexpr (LEAN) {
    // Lean plan: W is the only row array.  #1 and #2 read the unperturbed U through it (state sweeps concurrently on
    // waves 0/1, then their coefficient/costate phases one after the other, U re-published in between because the
    // results pass through W), #3 follows as an ordinary pipelined sweep on W = U + h*dUdt: one serial sweep more
    // than the full plans, the price of fitting two workgroups on a CU.
    static_assert(IPW * 16 >= 128, "lean preamble: two sweep waves");
    T* tab0 = P.scr + size_t(blockIdx.x) * 2 * Lds::tab_count(P.dv);
    T* xT0 = S.xT, *xT1 = S.xT + M::NX * IPW;
    publish_U();
    __syncthreads();
    make_xh();
    __syncthreads();
    sweep_state<false, false>(0, S.xh, dtau_h, S.R, xT0, false);
    sweep_state<false, false>(64, S.xs, dtau_0, tab0, xT1, false);
    __threadfence_block();
    __syncthreads();  // drains vmcnt: the parked table is complete and visible to the other waves of this CU
    CGM_STAMP(*this, 4);
    sweep_coeffs<false, F_PLAIN>(dtau_h, S.R, S.W, false);  // in place: every entry of W is read (as u) before it is written
    __syncthreads();
    CGM_STAMP(*this, 5);
    sweep_costate<F_PLAIN>(dtau_h, xT0, S.W, false);
    __syncthreads();
    {
      T fh[MAXM];
      lds_to_reg(fh, S.W);
      reg_to_row(P.Fh, P.Lg, fh);
    }
    __threadfence_block();
    __syncthreads();  // F(U,x+hf,t+h) rows visible to the coefficient phases of this CU; W is free again
    publish_U();
    __syncthreads();
    sweep_coeffs<false, F_RHS>(dtau_0, tab0, S.W, false);
    __syncthreads();
    CGM_STAMP(*this, 5);
    sweep_costate<F_RHS>(dtau_0, xT1, S.W, false);
    __syncthreads();
    lds_to_reg(bb, S.W);
    __syncthreads();
    if (WITH_AX0) {
      publish_direction(dir);
      __syncthreads();
      f_eval<true, F_AX>(S.xh, dtau_h, S.W, false);
      __syncthreads();
      lds_to_reg(ax0, S.W);
      __syncthreads();
    }
    return;
  }
  make_xh();
  __syncthreads();
  if constexpr (IPW * 16 >= 192) {
    const size_t tab_n = Lds::tab_count(P.dv);
    T* tab0 = P.scr + size_t(blockIdx.x) * 2 * tab_n;
    T* tab1 = tab0 + tab_n;
    T* xT0 = S.xT, *xT1 = S.xT + M::NX * IPW, *xT2 = S.xT + 2 * M::NX * IPW;
    sweep_state<false, false>(0, S.xh, dtau_h, S.R, xT0, false);
    sweep_state<false, false>(64, S.xs, dtau_0, tab0, xT1, false);
    if (WITH_AX0) sweep_state<true, false>(128, S.xh, dtau_h, tab1, xT2, false);
    __threadfence_block();
    __syncthreads();  // drains vmcnt: the HBM tables are complete and visible to the other waves of this CU
    CGM_STAMP(*this, 4);
    sweep_coeffs<false, F_PLAIN>(dtau_h, S.R, S.Fh, false);  // (S.Fh is S.W itself when fh_hbm)
    __syncthreads();
    CGM_STAMP(*this, 5);
    sweep_costate<F_PLAIN>(dtau_h, xT0, S.Fh, false);
    __syncthreads();
    if (fh_hbm()) {
      // Fh went through W: move it to its HBM row and put the direction of A*x0 back (its first copy served the
      // concurrent state sweep #3; the coefficient phase of #3 reads it again)
      T fh[MAXM];
      lds_to_reg(fh, S.W);
      reg_to_row(P.Fh, P.Lg, fh);
      __threadfence_block();
      __syncthreads();  // drains vmcnt: the rows are visible to the other waves of this CU
      if (WITH_AX0) publish_direction(dir);
      __syncthreads();
    }
    if (WITH_AX0) {
      sweep_coeffs<true, F_AX>(dtau_h, tab1, S.W, false);
      __syncthreads();
      CGM_STAMP(*this, 5);
      sweep_costate<F_AX>(dtau_h, xT2, S.W, false);
      __syncthreads();
      lds_to_reg(ax0, S.W);
      __syncthreads();
    }
    sweep_coeffs<false, F_RHS>(dtau_0, tab0, S.W, false);
    __syncthreads();
    CGM_STAMP(*this, 5);
    sweep_costate<F_RHS>(dtau_0, xT1, S.W, false);
    __syncthreads();
    lds_to_reg(bb, S.W);
    __syncthreads();
  } else {
    f_eval<false, F_PLAIN>(S.xh, dtau_h, S.Fh, false);
    __syncthreads();
    if (WITH_AX0) {
      f_eval<true, F_AX>(S.xh, dtau_h, S.W, false);
      __syncthreads();
      lds_to_reg(ax0, S.W);
      __syncthreads();
    }
    f_eval<false, F_RHS>(S.xs, dtau_0, S.W, false);
    __syncthreads();
    lds_to_reg(bb, S.W);
    __syncthreads();
  }
}
// Ax_func in place on W (cgmres.hpp:164-175).  Collective; ends with W published.
CGM_WGCTX_T
template <class After, class Idle>
__device__ __forceinline__ void CGM_WGCTX::ax(bool only_active, After&& after_sweep, Idle&& idle_work) {
  CGM_STAMP(*this, 3);
  f_eval<true, F_AX>(S.xh, dtau_h, S.W, only_active, after_sweep, idle_work);
  __syncthreads();
  CGM_STAMP(*this, 6);
}
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::ax(bool only_active) {
  ax(only_active, [] {}, [] {});
}

}  // namespace cgm
