// cgmres_hip_horizon_device: the predicted horizon and the optimality error of every instance, on the stream.
//
// One evaluation of F_func(ret, U, x, t) (cgmres.hpp:113-162) with the handle's U, ptau and t that KEEPS what the tick
// kernels throw away: the state trajectory xtau (:132-140), the costate trajectory ltau (:145-153), F itself (:156-161)
// and ||F||.  It is a kernel of its own, outside the tick kernels: nothing a tick reads is written here.
//
// Mapping: one lane per instance, 64 instances per workgroup (one wavefront), the model called exactly as the lane
// mapping calls it (tick_lane.hip.h: f_eval_lane / state_eq), statement order of the reference: multiply by dtau, add.
// Both recurrences are serial in the stage, so what the kernel must not do is wait for memory between two stages:
//   * U and ptau come on chip in CHUNKS of stages.  The 64 lanes load a chunk together — along the rows where an
//     instance's row is contiguous (wg contexts), across the instances where the batch index is innermost (lane
//     context) — into registers while the previous chunk is consumed from LDS, and park them in LDS between two chunks
//     (element-major, pitch 65: the row-wise stores of the wg layout spread over the banks).  No global load sits between
//     two stages of a chunk.
//   * x and the trig values of a chunk stay in lane-private LDS columns; every stage also stores them to global memory
//     (the caller's xtau_dev or the context's scratch; plain stores, nothing waits for them).  The costate sweep walks
//     the chunks in reverse: the last chunk is still on chip, the earlier ones are fetched back one chunk ahead.
//     A horizon of at most one chunk never reads x or trig from global memory.
//   * ||F|| is accumulated e ascending, as the interface says, in a third pass over F (the caller's F_dev or scratch).
// horizon_plan() is the one place that decides the chunk length and the LDS carve-up.
#pragma once
#include <hip/hip_runtime.h>

#include "models.hip.h"
#include "tick_common.hip.h"

namespace cgm {

constexpr int kHorizonLanes = 64;         // instances per workgroup = lanes of its one wavefront
constexpr int kHorizonPitch = 65;         // LDS pitch of a chunk's U / ptau elements (scalars)
constexpr int kHorizonMaxChunk = 16;      // stages
constexpr int kHorizonRegBudget = 32;     // scalars a lane holds in flight of U + ptau, and of x + trig
constexpr int kHorizonLdsBytes = 64 * 1024;  // static LDS of a workgroup

// Chunk length and LDS carve-up (host and device; no kernel code).  A chunk is `ch` consecutive stages:
//   up: [ch*(nu+np)][kHorizonPitch]   U then ptau of the chunk, element-major, any lane reads any instance's column
//   xt: [ch*(nx+nc)][kHorizonLanes]   x then trig of the chunk, lane-private columns
// ch is the largest of 1..kHorizonMaxChunk that keeps a lane's in-flight copy of either block within the register budget
// and both blocks within the LDS; fits = false when even one stage does not (a model of several hundred dimensions).
struct HorizonPlan {
  int ch, n_u, n_p, n_x, n_t;      // per instance and chunk: scalars of U, ptau, x, trig
  int off_u, off_p, off_x, off_t;  // LDS offsets, scalars
  int lds_elems;
  bool fits;
};
constexpr HorizonPlan horizon_plan(int nx, int nu, int np, int nc, int elem_bytes) {
  const int up = nu + np, xt = nx + nc, big = up > xt ? up : xt;
  const int per_stage = (up * kHorizonPitch + xt * kHorizonLanes) * elem_bytes;
  int ch = kHorizonRegBudget / big;
  if (ch > kHorizonLdsBytes / per_stage) ch = kHorizonLdsBytes / per_stage;
  if (ch > kHorizonMaxChunk) ch = kHorizonMaxChunk;
  const bool fits = per_stage <= kHorizonLdsBytes;
  if (ch < 1) ch = 1;
  HorizonPlan p{};
  p.ch = ch, p.n_u = ch * nu, p.n_p = ch * np, p.n_x = ch * nx, p.n_t = ch * nc;
  p.off_u = 0, p.off_p = p.n_u * kHorizonPitch, p.off_x = (p.n_u + p.n_p) * kHorizonPitch;
  p.off_t = p.off_x + p.n_x * kHorizonLanes;
  p.lds_elems = fits ? p.off_t + p.n_t * kHorizonLanes : 1;
  p.fits = fits;
  return p;
}
template <class M, class T>
constexpr HorizonPlan horizon_plan_of() {
  return horizon_plan(M::NX, M::NU, M::NP, M::NC, int(sizeof(T)));
}

// Element e of instance b at p[b*sb + e*se]: instance-major rows (wg: sb = pitch, se = 1), element-major arrays (lane
// and the scratch: sb = 1, se = ldb), the caller's instance-major outputs (sb = row length, se = 1).
template <class T>
struct HorizonView {
  T* p;
  size_t sb, se;
  __host__ __device__ T* at(size_t b, size_t e) const { return p + b * sb + e * se; }
};

template <class T>
struct HorizonParams {
  int B, dv;
  T dtau;    // get_dtau(t), cgmres.hpp:32-34, computed on the host like every tick's
  const T* x;             // [B][NX]
  HorizonView<const T> U, ptau;
  HorizonView<T> xtau;    // [dv+1][NX] per instance: the caller's xtau_dev or scratch; never null
  HorizonView<T> trig;    // [dv][NC] per instance: scratch; null when no costate sweep runs
  HorizonView<T> F;       // [dv][NU] per instance: the caller's F_dev, scratch for fnorm alone, or null
  T* ltau;                // [B][dv+1][NX] or null
  T* fnorm;               // [B] or null
  int back;               // run the costate sweep (anything but xtau is wanted)
};

// A chunk's elements [e0, e0+ne) of the 64 instances from b0 (nb of them exist), NE per instance at most: global memory
// -> registers, by all lanes together.  ROWS: item i = k*64 + lane is element i % NE of instance i / NE, so that consecutive lanes
// read consecutive words of a row; otherwise lane = instance.  Every address is a wave-uniform 64-bit part plus a 32-bit
// lane part (at most 64 rows, or 64 words, from the uniform one): one address register per load, not two.
template <int NE, bool ROWS, class T>
__device__ __forceinline__ void horizon_fetch(T* r, const HorizonView<const T>& v, int b0, int nb, int e0, int ne, int lane) {
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int i = k * kHorizonLanes + lane;
    const int bl = ROWS ? i / NE : lane, el = ROWS ? i % NE : k;
    const bool ok = bl < nb && el < ne;
    // An absent item loads the chunk's first word instead, which exists, and keeps it: no branch around the load and no
    // select behind it, which would wait for the load where it is issued.  Nothing reads an absent element; the lanes
    // past the batch then compute on a real instance's finite values and store nothing.
    const int ke = k < ne ? k : 0;
    const T* base = ROWS ? v.p + (size_t(b0) * v.sb + size_t(e0)) : v.p + (size_t(b0) + size_t(e0 + ke) * v.se);
    const unsigned off = ROWS ? unsigned(bl) * unsigned(v.sb) + unsigned(el) : unsigned(lane);
    r[k] = base[ok ? off : 0u];
  }
}
// ... registers -> LDS [NE][kHorizonPitch]
template <int NE, bool ROWS, class T>
__device__ __forceinline__ void horizon_park(T* lds, const T* r, int lane) {
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const int i = k * kHorizonLanes + lane;
    const int bl = ROWS ? i / NE : lane, el = ROWS ? i % NE : k;
    lds[el * kHorizonPitch + bl] = r[k];
  }
}
// A lane's own NE values from e0 of a per-instance array (all NE exist): global memory -> registers -> its LDS column
template <int NE, class T>
__device__ __forceinline__ void horizon_fetch_own(T* r, const HorizonView<T>& v, bool act, int b0, int lane, int e0) {
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const T* base = v.p + (size_t(b0) * v.sb + size_t(e0 + k) * v.se);  // (wave-uniform; a lane past the batch reads b0's)
    r[k] = base[act ? unsigned(lane) * unsigned(v.sb) : 0u];
  }
}
template <int NE, class T>
__device__ __forceinline__ void horizon_park_own(T* lds, const T* r, int lane) {
#pragma unroll
  for (int k = 0; k < NE; ++k) lds[k * kHorizonLanes + lane] = r[k];
}

#ifdef CGM_HORIZON_DIRECT
// A/B builds only (tools/bench_horizon.py --direct-lib): the straightforward form of the same kernel, against which the
// staging is timed.  Every stage loads its U, ptau, x and trig values from global memory where it needs them: a
// dependent round trip to L2 or HBM per stage and sweep.  Same arithmetic, same outputs.
template <class M, class T, bool ROWS>
__global__ __launch_bounds__(kHorizonLanes) void horizon_kernel(HorizonParams<T> P) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NC = M::NC;
  const int b = blockIdx.x * kHorizonLanes + threadIdx.x, dv = P.dv;
  if (b >= P.B) return;
  const T dtau = P.dtau;
  typename M::Math mc;
  mc.init();
  T xs[NX], l[NX], p[NP > 0 ? NP : 1];
#pragma unroll
  for (int i = 0; i < NX; ++i) xs[i] = P.x[size_t(b) * NX + i];
  for (int s = 0; s < dv; ++s) {
    T u[NU], f[NX], tr[NC > 0 ? NC : 1];
#pragma unroll
    for (int q = 0; q < M::NU_DYN; ++q) u[q] = *P.U.at(b, s * NU + q);
#pragma unroll
    for (int i = 0; i < NX; ++i) *P.xtau.at(b, s * NX + i) = xs[i];
    if constexpr (DxdtUsesP<M, T>::value) {
#pragma unroll
      for (int q = 0; q < NP; ++q) p[q] = *P.ptau.at(b, s * NP + q);
      M::dxdt_p(f, xs, u, p);
    } else {
      M::dxdt(f, xs, u, tr, mc);
    }
#pragma unroll
    for (int q = 0; q < NC; ++q)
      if (P.trig.p) *P.trig.at(b, s * NC + q) = tr[q];
#pragma unroll
    for (int i = 0; i < NX; ++i) xs[i] = f[i] * dtau + xs[i];
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) *P.xtau.at(b, dv * NX + i) = xs[i];
  if (!P.back) return;
#pragma unroll
  for (int q = 0; q < NP; ++q) p[q] = *P.ptau.at(b, dv * NP + q);
  M::dPhidx(l, xs, p);
  if (P.ltau) {
#pragma unroll
    for (int i = 0; i < NX; ++i) P.ltau[(size_t(b) * (dv + 1) + dv) * NX + i] = l[i];
  }
  for (int s = dv - 1; s >= 0; --s) {
    T u[NU], tr[NC > 0 ? NC : 1], Fs[NU], gx[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xs[i] = *P.xtau.at(b, s * NX + i);
#pragma unroll
    for (int q = 0; q < NC; ++q) tr[q] = *P.trig.at(b, s * NC + q);
#pragma unroll
    for (int q = 0; q < NU; ++q) u[q] = *P.U.at(b, s * NU + q);
#pragma unroll
    for (int q = 0; q < NP; ++q) p[q] = *P.ptau.at(b, s * NP + q);
    M::dHdu(Fs, xs, u, p, l, tr);
    if (P.F.p) {
#pragma unroll
      for (int q = 0; q < NU; ++q) *P.F.at(b, s * NU + q) = Fs[q];
    }
    M::dHdx(gx, xs, u, p, l, tr);
#pragma unroll
    for (int i = 0; i < NX; ++i) l[i] = gx[i] * dtau + l[i];
    if (P.ltau) {
#pragma unroll
      for (int i = 0; i < NX; ++i) P.ltau[(size_t(b) * (dv + 1) + s) * NX + i] = l[i];
    }
  }
  if (P.fnorm) {
    T ss = T(0);
    for (int e = 0; e < dv * NU; ++e) {
      const T v = *P.F.at(b, e);
      ss += v * v;
    }
    P.fnorm[b] = sqrt_t<T>(ss);
  }
}
#else
template <class M, class T, bool ROWS>
__global__ __launch_bounds__(kHorizonLanes) void horizon_kernel(HorizonParams<T> P) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NC = M::NC;
  constexpr HorizonPlan pl = horizon_plan_of<M, T>();
  constexpr int CH = pl.ch;
  constexpr int RU = pl.n_u, RP = NP > 0 ? pl.n_p : 1, RX = pl.n_x, RT = NC > 0 ? pl.n_t : 1;
  __shared__ T lds[pl.lds_elems];
  T* const lu = lds + pl.off_u;
  T* const lp = lds + pl.off_p;
  T* const lx = lds + pl.off_x;
  T* const lt = lds + pl.off_t;

  const int lane = threadIdx.x, b0 = blockIdx.x * kHorizonLanes, b = b0 + lane;
  const int nb = P.B - b0 < kHorizonLanes ? P.B - b0 : kHorizonLanes;
  const bool act = lane < nb;
  const int dv = P.dv;
  const int nch = (dv + CH - 1) / CH;
  const T dtau = P.dtau;

  typename M::Math mc;
  mc.init();
  T xs[NX], pe[NP > 0 ? NP : 1];
#pragma unroll
  for (int i = 0; i < NX; ++i) xs[i] = act ? P.x[size_t(b) * NX + i] : T(0);
#pragma unroll
  for (int j = 0; j < NP; ++j) pe[j] = act ? *P.ptau.at(size_t(b), size_t(dv * NP + j)) : T(0);  // the terminal stage's p

  T ru[RU], rp[RP];  // the chunk in flight
  horizon_fetch<pl.n_u, ROWS>(ru, P.U, b0, nb, 0, (dv < CH ? dv : CH) * NU, lane);
  if constexpr (NP > 0) horizon_fetch<pl.n_p, ROWS>(rp, P.ptau, b0, nb, 0, (dv < CH ? dv : CH) * NP, lane);

  // ---- state sweep, cgmres.hpp:132-140 ----
  for (int c = 0; c < nch; ++c) {
    const int s0 = c * CH, n = dv - s0 < CH ? dv - s0 : CH;
    __syncthreads();  // the previous chunk has been read
    horizon_park<pl.n_u, ROWS>(lu, ru, lane);
    if constexpr (NP > 0) horizon_park<pl.n_p, ROWS>(lp, rp, lane);
    __syncthreads();
    if (c + 1 < nch) {  // the next chunk travels while this one is consumed
      const int s1 = s0 + CH, n1 = dv - s1 < CH ? dv - s1 : CH;
      horizon_fetch<pl.n_u, ROWS>(ru, P.U, b0, nb, s1 * NU, n1 * NU, lane);
      if constexpr (NP > 0) horizon_fetch<pl.n_p, ROWS>(rp, P.ptau, b0, nb, s1 * NP, n1 * NP, lane);
    }
    for (int j = 0; j < n; ++j) {
      const int s = s0 + j;
      T u[NU], f[NX], tr[NC > 0 ? NC : 1];
#pragma unroll
      for (int q = 0; q < M::NU_DYN; ++q) u[q] = lu[(j * NU + q) * kHorizonPitch + lane];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        lx[(j * NX + i) * kHorizonLanes + lane] = xs[i];
        if (act) *P.xtau.at(size_t(b), size_t(s * NX + i)) = xs[i];
      }
      if constexpr (DxdtUsesP<M, T>::value) {
        T p[NP > 0 ? NP : 1];
#pragma unroll
        for (int q = 0; q < NP; ++q) p[q] = lp[(j * NP + q) * kHorizonPitch + lane];
        M::dxdt_p(f, xs, u, p);
      } else {
        M::dxdt(f, xs, u, tr, mc);
      }
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        lt[(j * NC + q) * kHorizonLanes + lane] = tr[q];
        if (act && P.trig.p) *P.trig.at(size_t(b), size_t(s * NC + q)) = tr[q];
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) xs[i] = f[i] * dtau + xs[i];
    }
  }
  if (act) {
#pragma unroll
    for (int i = 0; i < NX; ++i) *P.xtau.at(size_t(b), size_t(dv * NX + i)) = xs[i];
  }
  if (!P.back) return;

  // ---- terminal costate, cgmres.hpp:145; costate sweep with dH/du, :146-161 ----
  T l[NX];
  M::dPhidx(l, xs, pe);
  if (act && P.ltau) {
#pragma unroll
    for (int i = 0; i < NX; ++i) P.ltau[(size_t(b) * (dv + 1) + dv) * NX + i] = l[i];
  }
  T rx[RX], rt[RT];
  for (int c = nch - 1; c >= 0; --c) {
    const int s0 = c * CH, n = dv - s0 < CH ? dv - s0 : CH;
    if (c != nch - 1) {  // (the last chunk of the state sweep is still on chip)
      __syncthreads();
      horizon_park<pl.n_u, ROWS>(lu, ru, lane);
      if constexpr (NP > 0) horizon_park<pl.n_p, ROWS>(lp, rp, lane);
      horizon_park_own<pl.n_x>(lx, rx, lane);
      if constexpr (NC > 0) horizon_park_own<pl.n_t>(lt, rt, lane);
      __syncthreads();
    }
    if (c > 0) {  // a full chunk
      const int s1 = s0 - CH;
      horizon_fetch<pl.n_u, ROWS>(ru, P.U, b0, nb, s1 * NU, CH * NU, lane);
      if constexpr (NP > 0) horizon_fetch<pl.n_p, ROWS>(rp, P.ptau, b0, nb, s1 * NP, CH * NP, lane);
      horizon_fetch_own<pl.n_x>(rx, P.xtau, act, b0, lane, s1 * NX);
      if constexpr (NC > 0) horizon_fetch_own<pl.n_t>(rt, P.trig, act, b0, lane, s1 * NC);
    }
    for (int j = n - 1; j >= 0; --j) {
      const int s = s0 + j;
      T u[NU], p[NP > 0 ? NP : 1], tr[NC > 0 ? NC : 1], Fs[NU], gx[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) xs[i] = lx[(j * NX + i) * kHorizonLanes + lane];
#pragma unroll
      for (int q = 0; q < NC; ++q) tr[q] = lt[(j * NC + q) * kHorizonLanes + lane];
#pragma unroll
      for (int q = 0; q < NU; ++q) u[q] = lu[(j * NU + q) * kHorizonPitch + lane];
#pragma unroll
      for (int q = 0; q < NP; ++q) p[q] = lp[(j * NP + q) * kHorizonPitch + lane];
      M::dHdu(Fs, xs, u, p, l, tr);
      if (act && P.F.p) {
#pragma unroll
        for (int q = 0; q < NU; ++q) *P.F.at(size_t(b), size_t(s * NU + q)) = Fs[q];
      }
      M::dHdx(gx, xs, u, p, l, tr);
#pragma unroll
      for (int i = 0; i < NX; ++i) l[i] = gx[i] * dtau + l[i];
      if (act && P.ltau) {
#pragma unroll
        for (int i = 0; i < NX; ++i) P.ltau[(size_t(b) * (dv + 1) + s) * NX + i] = l[i];
      }
    }
  }

  // ---- ||F||: sqrt(sum_e F[e]^2), e ascending ----
  if (act && P.fnorm) {
    const int L = dv * NU;
    T ss = T(0);
#pragma unroll 16
    for (int e = 0; e < L; ++e) {
      const T v = *P.F.at(size_t(b), size_t(e));
      ss += v * v;
    }
    P.fnorm[b] = sqrt_t<T>(ss);
  }
}
#endif  // CGM_HORIZON_DIRECT

}  // namespace cgm
