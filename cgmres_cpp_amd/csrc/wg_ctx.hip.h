// WgCtx: the per-thread view of one workgroup's job in the "wg" tick kernels (tick_wg.hip.h has the overview) — its
// state, the row I/O helpers, and the declarations of the three phases, which are defined in
//   wg_sweep_serial.hip.h   the horizon sweep of the serial-sweep kernel (full, fh_hbm and lean plans)
//   wg_sweep_rows.hip.h     the row-parallel sweeps: row-Newton (NWT = 1) and row-scan (NWT = 2)
//   wg_gmres.hip.h          the solver
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <type_traits>

#include "wave_scan.hip.h"
#include "stage_own.hip.h"
#include "dpp.hip.h"
#include "models.hip.h"
#include "newton_rot.hip.h"
#include "tick_common.hip.h"  // sqrt_t / FOut
#include "wg_layout.hip.h"
#include "wg_stamps.hip.h"

namespace cgm {

// Per-thread view of one workgroup's job.
// PAR: form of the costate sweep — 0 serial (one lane per instance walks all stages), 1 chunk-parallel with per-stage
// scratch in LDS (sweep_costate_par: full plans with short vectors), 2 chunk-parallel in two passes, boundary records only
// (sweep_costate_2pass: every plan).
// NWT = 1: the state sweeps of the Arnoldi loop run as Newton iterations on the whole trajectory, row-parallel on all
// four waves (row_newton_sweep) instead of the serial quad sweep on wave 0; the stage table then has NWT_TABX spare
// scalars per stage so that the 16 lanes of a row, which own four consecutive stages each, store into distinct banks.
template <class M, class T, int IPW, int MAXM, bool LEAN = false, int PAR = 0, int NWT = 0>
struct WgCtx {
  using Lds = WgLds<M, T, IPW, NWT ? NWT_TABX : 0>;
  static constexpr int NSTG = Lds::NSTG;
  // offset of (stage s, slot) in a stage table
  static __device__ __forceinline__ int tab_off(int s, int slot = 0) {
    if constexpr (NWT != 0) return s * TAB_STEP + slot * IPW;
    return (s * NSTG + slot) * IPW;
  }
  static constexpr int TAB_STEP = NSTG * IPW + (NWT ? NWT_TABX : 0);  // scalars from one stage to the next
  const WgParams<T>& P;
  Lds S;
  // lean plan: this row's U in the row layout for the whole launch — in registers, unless a row is 160 bytes per lane or
  // more (fp64 with MAXM = 20): those kernels are register-starved at 256 registers per wave and re-read their U row
  // from HBM/L2 where they need it (once per Arnoldi iteration, ~1/30 of the iteration's traffic)
  static constexpr bool U_IN_REGS = LEAN && sizeof(T) * MAXM < 160;
  static constexpr bool VK_IN_REGS = !LEAN || U_IN_REGS;  // v_k kept in registers between its creation and the next MGS
  T ureg[U_IN_REGS ? MAXM : 1];
  T* pTw;                   // lean plan: this workgroup's transposed parameter horizon [(stage*NP + j)*IPW + i]
  int tid, inst, r, b;  // b = global instance of this thread's row
  bool valid;           // row has a real instance
  bool sweep_lane;      // this thread runs the serial sweeps (for instance `tid`)
  T dtau_h, dtau_0;     // horizon steps of the current tick: F(., t+h) and F(., t)
  int bi;               // global instance of the sweep lane
  // S.flag of the instances this thread works on in the sweeps of the current Arnoldi iteration — instance tid mod IPW
  // (items of the coefficient and costate phases, the lane-per-instance state sweep) and instance (tid mod 64) / 4 (quad
  // state sweep) — read once per iteration with the loop-top flag reads (gmres()) instead of one LDS round trip at the
  // start of every phase; only meaningful where `only_active` is passed (the Arnoldi loop)
  int act_i = 1, act_q = 1;
  int rot_level = 0, rot_hold = 0;  // quad sweep: form of the trig update the sweeps of this wave currently take (sweep_state)
  typename M::template MathFor<LEAN> mc;  // per-thread math context (pinned sin/cos constants); A/B: keeping it live for the whole
                        // kernel is 13 us/tick FASTER than re-creating it inside every sweep
  __device__ __forceinline__ WgCtx(const WgParams<T>& P_, unsigned char* smem)
      : P(P_), S(smem, P_, LEAN ? PLAN_LEAN : (MAXM > 10 && P_.fh_hbm ? PLAN_FH_HBM : PLAN_FULL)), tid(threadIdx.x),
        inst(threadIdx.x >> 4), r(threadIdx.x & 15) {
    pTw = LEAN ? P.pT + size_t(blockIdx.x) * (P.dv + 1) * (M::NP > 0 ? M::NP : 1) * IPW : nullptr;
    const int q = blockIdx.x * IPW + inst, qs = blockIdx.x * IPW + tid;  // slots of this row / of the sweep lane
    valid = q < P.B;
    sweep_lane = tid < IPW && qs < P.B;
    b = (valid && P.perm) ? P.perm[q] : q;
    bi = (sweep_lane && P.perm) ? P.perm[qs] : qs;
    dtau_h = P.dtau_h, dtau_0 = P.dtau_0;
    mc.init();
    CGM_STAMP(*this, -1);
  }
  __device__ __forceinline__ int elem(int m) const { return r + 16 * m; }

  // rows: HBM [B][Lg] -> LDS row / registers
  __device__ __forceinline__ void load_row_to_lds(T* lds, const T* g) const {
    if (!valid) return;
    const T* src = g + size_t(b) * P.Lg;
    T* row = lds + inst * P.Lp;
    each_elem([&](int m, auto full) {
      if (decltype(full)::value || elem(m) < P.L) row[elem(m)] = src[elem(m)];
    });
  }
  __device__ __forceinline__ void load_row_to_reg(T* reg, const T* g, size_t pitch) const {
    const T* src = g + size_t(b) * pitch;
    each_elem([&](int m, auto full) {
      reg[m] = (valid && (decltype(full)::value || elem(m) < P.L)) ? src[elem(m)] : T(0);
    });
  }
  // (Elements r + 16 m with m < L / 16 exist in every lane.  A per-lane guard on every element is an exec-mask sequence
  // of ~8 instructions each — the masks live in spilled SGPRs — and lds_to_reg / publish_direction run in every Arnoldi
  // iteration on every wave.  When all but the last two elements are full — L > 16 (MAXM - 2): what a kernel of this
  // MAXM is normally chosen for — those are moved without a guard, in their own arm of a SCALAR branch (guards inside
  // one loop, `m < L / 16 || e < L`, the compiler folds back into ten per-lane masks).)
  static constexpr int MFAST = MAXM - 2;
  __device__ __forceinline__ bool mostly_full() const { return (P.L >> 4) >= MFAST; }
  template <class F>
  __device__ __forceinline__ void each_elem(F&& f) const {  // f(m, full): full = element m exists in every lane
    if (mostly_full()) {
#pragma unroll
      for (int m = 0; m < MFAST; ++m) f(m, std::true_type{});
#pragma unroll
      for (int m = MFAST; m < MAXM; ++m) f(m, std::false_type{});
    } else {
#pragma unroll
      for (int m = 0; m < MAXM; ++m) f(m, std::false_type{});
    }
  }
  __device__ __forceinline__ void lds_to_reg(T* reg, const T* lds) const {
    const T* row = lds + inst * P.Lp;
    each_elem([&](int m, auto full) { reg[m] = (decltype(full)::value || elem(m) < P.L) ? row[elem(m)] : T(0); });
  }
  __device__ __forceinline__ void reg_to_lds(T* lds, const T* reg) const {
    T* row = lds + inst * P.Lp;
    each_elem([&](int m, auto full) {
      if (decltype(full)::value || elem(m) < P.L) row[elem(m)] = reg[m];
    });
  }
  // The direction d of a matrix-vector product is published to the sweeps as the perturbed control U + h*d
  // (cgmres.hpp:166-168 forms it in every stage); the sweep phases then read one array instead of two.
  __device__ __forceinline__ void publish_direction(const T* reg) const {
    T uu[MAXM];  // all reads first (pad lanes read in-bounds words of the next row, never stored)
    if constexpr (LEAN) {
      get_urow(uu);
    } else {
#pragma unroll
      for (int m = 0; m < MAXM; ++m) uu[m] = S.U[inst * P.Lp + elem(m)];
    }
    T* row = S.W + inst * P.Lp;
    if constexpr (NWT != 0) {
      // also: did the direction change any control of this row?  One that the rounding of U + h*d absorbs completely
      // leaves F unchanged bit for bit in the serial sweeps — A*d = 0 exactly, the reference's breakdown case
      // (gmres.hpp:63-65) — while Newton's fixed point agrees with the serial trajectory up to rounding only: gmres()
      // answers that case from this flag.
      bool moved = false;
      each_elem([&](int m, auto full) {
        if (decltype(full)::value || elem(m) < P.L) {
          const T wv = reg[m] * P.h + uu[m];
          moved = moved || wv != uu[m];
          row[elem(m)] = wv;
        }
      });
      row_moved = ((__ballot(moved) >> (16 * ((tid >> 4) & 3))) & 0xffffull) != 0;
      return;
    }
    each_elem([&](int m, auto full) {  // (see lds_to_reg)
      if (decltype(full)::value || elem(m) < P.L) row[elem(m)] = reg[m] * P.h + uu[m];
    });
  }
  // lean plan: the unperturbed sweeps read U through W as well
  __device__ __forceinline__ void publish_U() const {
    if constexpr (LEAN) {
      T uu[MAXM];
      get_urow(uu);
      reg_to_lds(S.W, uu);
    }
  }
  // lean plan: this row's U (registers, or its HBM row — written by this same thread, so program order suffices)
  __device__ __forceinline__ void get_urow(T* dst) const {
    if constexpr (U_IN_REGS) {
#pragma unroll
      for (int m = 0; m < MAXM; ++m) dst[m] = ureg[m];
    } else {
      load_row_to_reg(dst, P.U, P.Lg);
    }
  }
  __device__ __forceinline__ void reg_to_row(T* g, size_t pitch, const T* reg) const {
    if (!valid) return;
    T* dst = g + size_t(b) * pitch;
    each_elem([&](int m, auto full) {
      if (decltype(full)::value || elem(m) < P.L) dst[elem(m)] = reg[m];
    });
  }
  __device__ __forceinline__ T* vrow(int j) const {  // Krylov vector j of this row's instance
    if constexpr (NWT != 0) {
      // From an opaque copy of the instance index at every use: the row addresses are invariant over the whole launch,
      // and hoisted to the kernel entry they are a dozen 64-bit values in scratch — each reload in the Gram-Schmidt rounds
      // sits behind s_waitcnt vmcnt(0), i.e. waits for every basis row in flight.
      int bo = b;
      asm volatile("" : "+v"(bo));
      return P.V + (size_t(bo) * (P.kmax + 1) + j) * P.Lv;
    }
    return P.V + (size_t(b) * (P.kmax + 1) + j) * P.Lv;
  }
  // Krylov rows have pitch 16*MAXM and zero pads (every vector written here has zero pads: lds_to_reg clears
  // them and all later operations are linear), so neither direction needs a guard.  That matters for more than the
  // compare: a guarded load is an exec-masked branch, and the compiler cannot count outstanding loads across
  // branches — every wait in the Gram-Schmidt rounds became vmcnt(0) and serialised the register ring.
  // In HBM a Krylov row is stored pair-interleaved — element (r + 16 m) at (m/2)*32 + 2r + (m&1) — so a lane moves
  // two of its elements per 16-byte access: half the vector-memory instructions (the CU's address unit takes ~16
  // cycles per 64-lane access and four waves issue their rows at once).  ctx_wg undoes the permutation on export.
  struct alignas(2 * sizeof(T)) Pair {
    T a, b;
  };
  // Row-parallel Newton kernel: a lane's NVEC = 12 elements are those of its own four stages (stage_own.hip.h) — the same
  // row format, slot pair i/2 of lane r at (i/2)*32 + 2r + (i&1) (StageOwn::hbm_pos), rows of 16*NVEC scalars.
  static constexpr int NVEC = NWT == 1 ? StageOwn::NV : MAXM;  // elements of a solver vector per lane
  static_assert(NVEC % 2 == 0, "pair-interleaved Krylov rows");
  __device__ __forceinline__ int vec_elem(int m) const { return NWT == 1 ? StageOwn::elem(r, m) : elem(m); }
  __device__ __forceinline__ void load_vec(T* reg, const T* row) const {
    const Pair* q = reinterpret_cast<const Pair*>(row) + r;
#pragma unroll
    for (int m = 0; m < NVEC; m += 2) {
      const Pair t = q[(m / 2) * 16];
      reg[m] = t.a, reg[m + 1] = t.b;
    }
  }
  __device__ __forceinline__ void store_vec(T* row, const T* reg) const {
    Pair* q = reinterpret_cast<Pair*>(row) + r;
#pragma unroll
    for (int m = 0; m < NVEC; m += 2) q[(m / 2) * 16] = Pair{reg[m], reg[m + 1]};
  }

  // element q of this row's parameter horizon: LDS row, or (lean) the workgroup's transposed copy in HBM/L2, which the
  // coefficient phase reads 16 instances at a time.  Readers are other waves of this workgroup = same CU, same L1:
  // visible after a barrier that drains vmcnt (__syncthreads), like the parked stage tables.
  __device__ __forceinline__ void put_p(int q, T v) const {
    if constexpr (LEAN)
      pTw[size_t(q) * IPW + inst] = v;
    else
      S.p[inst * P.Pp + q] = v;
  }
  __device__ __forceinline__ T get_p(int i, int q) const { return LEAN ? pTw[size_t(q) * IPW + i] : S.p[i * P.Pp + q]; }
  // the state equation at `stage` for instance i: the built-in models ignore p; a user model compiled through the
  // plugin path may read it (Model::dxdt(ret, x, u, p), <example>/model.hpp:36)
  __device__ __forceinline__ void model_dxdt(T* f, const T* x, const T* u, T* tr, int i, int stage) const {
    if constexpr (DxdtUsesP<M, T>::value) {
      T p[M::NP > 0 ? M::NP : 1];
#pragma unroll
      for (int j = 0; j < M::NP; ++j) p[j] = get_p(i, stage * M::NP + j);
      M::dxdt_p(f, x, u, p);
    } else {
      M::dxdt(f, x, u, tr, mc);
    }
  }
  // Common prologue: U, ptau -> LDS; x -> LDS (component-major); flags cleared.  All global loads of the row are
  // issued before the first LDS store so they overlap (one HBM/L2 round trip instead of one per element).
  __device__ __forceinline__ void load_common(const T* Ug) {
    constexpr int PMAX = 8;  // ptau entries per lane held in flight (covers dim_p*(dv+1) <= 128)
    const int np_all = M::NP * (P.dv + 1);
    T urow[NVEC], preg[PMAX], xreg = T(0);
    if constexpr (ROW_NEWTON)
      so_load_row(urow, Ug);
    else if constexpr (!LEAN || U_IN_REGS)
      load_row_to_reg(urow, Ug, P.Lg);
    if (valid) {
#pragma unroll
      for (int n = 0; n < PMAX; ++n) {
        const int q = r + 16 * n;
        preg[n] = q < np_all ? P.ptau[size_t(b) * np_all + q] : T(0);
      }
      if (r < M::NX && P.x_in) {
        xreg = P.x_in[size_t(b) * M::NX + r];
        if (__builtin_expect(P.pin != nullptr, 0) && P.pin->meas) xreg = xreg + P.pin->meas[size_t(b) * P.pin->meas_inst + r];  // y_0 = x_0 + v_0 of this launch
      }
    }
    if constexpr (U_IN_REGS) {
#pragma unroll
      for (int m = 0; m < MAXM; ++m) ureg[m] = urow[m];
    }
    if (valid) {
      if constexpr (ROW_NEWTON)
        so_put_U(urow);
      else if constexpr (!LEAN)
        reg_to_lds(S.U, urow);
#pragma unroll
      for (int n = 0; n < PMAX; ++n) {
        const int q = r + 16 * n;
        if (q < np_all) put_p(q, preg[n]);
      }
      for (int q = r + 16 * PMAX; q < np_all; q += 16) put_p(q, P.ptau[size_t(b) * np_all + q]);
      if (r < M::NX) S.xs[r * IPW + inst] = xreg;
    }
    if (r == 0) {
      S.flag[inst] = 0;
      S.reason[inst] = 0;
      S.nax[inst] = 0;
      S.ksolve[inst] = 0;
      S.binst[inst] = b;
    }
  }

  // set_ptau before a tick of the fused loop (cgmres.hpp:36-39): this row's parameter horizon -> LDS
  __device__ __forceinline__ void load_ptau_tick(const T* seq_tick) {
    if (!valid) return;
    const int np_all = M::NP * (P.dv + 1);
    const T* src = seq_tick + size_t(b) * P.pseq_inst;
    for (int q = r; q < np_all; q += 16) put_p(q, src[q]);
  }

  // ---- constants, nested types and state of the phases below (each explained where it is used)
  // stages of the last pipeline chunk under SPLIT_TAIL (chunk_len)
  static constexpr int SPLIT_N = 12;
  // what the coefficient phase is compiled with (wg_sweep_serial.hip.h)
  static constexpr bool HBM_OPERANDS = LEAN || MAXM > 10;  // kernels that carry the fh_hbm / lean code
  // the pipelined quad sweep stores x0 / x2 every other stage; the coefficient phase works on stage pairs
  static constexpr bool ALT_X02 = M::HAS_QUAD_SWEEP && IPW * 16 >= 128;
  static constexpr bool SPLIT_TAIL = ALT_X02 && !HBM_OPERANDS && IPW == 16;
  static_assert(!SPLIT_TAIL || IPW * 16 - 64 == 16 * 12, "SPLIT_N stages x 16 instances = the lanes of the three coefficient waves");
  static constexpr int COEFF_GROUP = sizeof(T) == 8 ? 2 : 3;
  struct CoeffPre {
    T p[M::NP > 0 ? M::NP : 1], fh[M::NU];
  };
  // chunk-parallel costate sweeps (sweep_costate_par, sweep_costate_2pass)
  static constexpr int HL = M::NX * IPW;  // homogeneous lanes per chunk
  // PAR is a KERNEL TEMPLATE parameter, not a run-time switch: with both forms of the sweep in one kernel (or one body
  // with run-time chunk parameters) the register allocation of the Arnoldi loop tips over — two more spills inside the
  // loop, each reload behind an s_waitcnt vmcnt(0), cost 5 % of the tick (measured).
  static constexpr bool PAR_OK = M::COSTATE_HOM && IPW == 16 && M::NX * IPW <= 64 && M::NX % 2 == 0;
  static constexpr bool PAR_COSTATE = PAR == 1 && PAR_OK && !LEAN;
  static constexpr bool PAR_2PASS = PAR == 2 && PAR_OK;
  // row-parallel kernels (wg_sweep_rows.hip.h)
  static constexpr bool ROW_NEWTON = NWT == 1;
  // its 16 lanes all store the words of the Hessenberg column that they all hold (mgs_round, gmres)
  static constexpr bool ROW_ALL_STORE = ROW_NEWTON;
  // (Newton on an explicit recurrence cannot fail to terminate: iteration n makes stage n exact — its predecessor is —
  // so dv iterations reproduce the serial sweep whatever the start; the bound below is never reached by the test on the
  // correction, it only has to be >= dv.  Two iterations is what the mat-vecs of a tick take.)
  static constexpr int SPL = 4, NEWTON_MAX = 64;
  struct RowBase {
    T x0[SPL], x1[SPL], x2[SPL], sd[SPL], cd[SPL], s1[SPL], c1[SPL];
  };
  static constexpr int NBASE = 7;  // arrays of RowBase
  static_assert(SPL == WG_ROW_SPL && NBASE == WG_ROW_NBASE, "wg_layout.hip.h: what the planner places");
  struct NoBase {};
  std::conditional_t<ROW_NEWTON, RowBase, NoBase> nb;
  mutable bool row_moved = true;  // the direction changed at least one control of this row (row_newton_sweep; NWT = 2: publish_direction)
  static constexpr size_t base_array_bytes() { return wg_base_array_bytes<T>(IPW); }  // one of the NBASE arrays
  // 1 / dtau_h of the tick whose base store_base() stored
  T inv_dtau_nb = T(0);
  // stage ownership (stage_own.hip.h; the so_* accessors)
  static constexpr int NV = StageOwn::NV;
  static_assert(!ROW_NEWTON || (SPL == StageOwn::SPL && M::NU == StageOwn::NU && IPW == 16), "stage_own.hip.h");
  // the small Krylov arrays of this row's instance in LDS
  struct Krylov {
    T* H;    // compact: column k has k+1 entries (rows 0..k) at offset hoff(k); h(k+1,k): S.hsub
    T* rho;  // the residual vector e, then y
    T* g;    // reflector k: words 3k .. 3k+2
  };
  static __device__ __forceinline__ int hoff(int k) { return (k * (k + 1)) >> 1; }

  // ---- wg_sweep_serial.hip.h: the serial-sweep kernel's horizon sweep
  // F(U,x+hf,t+h) lives in HBM only (compiled out of the short-vector full-plan kernels)
  __device__ __forceinline__ bool fh_hbm() const;
  // value of lane `src` of this wave, through the LDS crossbar
  static __device__ __forceinline__ double row_bcast(double v, int src);
  static __device__ __forceinline__ float row_bcast(float v, int src);
  // workgroup barrier that orders LDS only (HBM traffic stays in flight)
  __device__ __forceinline__ void lds_barrier() const;
  // stages per pipeline chunk of phases 1 / 2 (even)
  __device__ __forceinline__ int chunk_len() const;
  // phase 1 on the wave [lane0, lane0 + 64): x(s), trig(s) -> tab, x(dv) -> xT; PIPE: one lds_barrier() per chunk
  template <bool PERT, bool PIPE, bool ALT = false>
  __device__ __forceinline__ void sweep_state(int lane0, const T* x0c, T dtau, T* tab, T* xT, bool only_active);
  // the HBM/L2 operands of item (s, i) of phase 2
  template <int MODE>
  __device__ __forceinline__ void coeff_prefetch(CoeffPre& c, int s, int i) const;
  // phase 2 for stage s of instance i: tab -> coefficients in S.R, costate-free part of the result -> out
  template <bool PERT, int MODE>
  __device__ __forceinline__ void coeff_item(int s, int i, T dtau, const T* tab, T* out, const CoeffPre* pre = nullptr,
                                             const T* x02 = nullptr);
  // instance i of this workgroup exists (and, with only_active, is still iterating)
  __device__ __forceinline__ bool item_on(int i, bool only_active) const;
  // COEFF_GROUP items q0, q0 + stride, ... of [0, n_items): fetch, between(), compute
  template <bool PERT, int MODE, class Between>
  __device__ __forceinline__ void coeff_group(int q0, int stride, int n_items, int s0, T dtau, const T* tab, T* out,
                                              bool only_active, Between&& between);
  // the same for (stage pair, instance) items of the LDS table (ALT_X02)
  template <bool PERT, int MODE, class Between>
  __device__ __forceinline__ void coeff_group_pairs(int q0, int stride, int s0, int s_end, T dtau, T* out,
                                                    bool only_active, Between&& between);
  // phase 2 for all stages, all threads
  template <bool PERT, int MODE>
  __device__ __forceinline__ void sweep_coeffs(T dtau, const T* tab, T* out, bool only_active);
  // phase 2 on the waves other than wave 0, chunk by chunk behind sweep_state<PERT, true>
  template <bool PERT, int MODE>
  __device__ __forceinline__ void coeffs_chunked(T dtau, T* out, bool only_active);
  // phase 3 in the kernel's form (PAR); COLLECTIVE, the caller publishes `out`
  template <int MODE>
  __device__ __forceinline__ void sweep_costate(T dtau, const T* xT, T* out, bool only_active);
  // l = dPhi/dx at the terminal state of instance i
  __device__ __forceinline__ void costate_terminal(T* l, const T* xT, int i) const;
  // `count` (+ `extra` where `more`) stages hi, hi-1, ... of the costate recurrence on this lane
  template <int MODE, bool HOM, bool WRITE, class Init>
  __device__ __forceinline__ void costate_run(T* l, int i, int hi, int count, T dtau, const T* coef, T* orow, Init&& init,
                                              int extra = 0, bool more = false);
  // phase 3 chunk-parallel with per-stage scratch in LDS (PAR = 1)
  template <int MODE>
  __device__ __forceinline__ void sweep_costate_par(T dtau, const T* xT, T* out, bool only_active);
  // phase 3 chunk-parallel in two passes, boundary records only (PAR = 2)
  template <int MODE>
  __device__ __forceinline__ void sweep_costate_2pass(T dtau, const T* xT, T* out, bool only_active);
  // one complete sweep on the LDS table: out = F / RHS / A*W per MODE.  COLLECTIVE; the caller publishes `out`
  template <bool PERT, int MODE, class After, class Idle>
  __device__ __forceinline__ void f_eval(const T* x0c, T dtau, T* out, bool only_active, After&& after_sweep,
                                         Idle&& idle_work);
  template <bool PERT, int MODE>
  __device__ __forceinline__ void f_eval(const T* x0c, T dtau, T* out, bool only_active);
  // S.xh = x + h f(x, U0) on the sweep lanes
  __device__ __forceinline__ void make_xh();
  // the sweeps in front of the solve: Fh -> S.Fh / HBM, b -> bb, A*dUdt -> ax0 (WITH_AX0).  COLLECTIVE
  template <bool WITH_AX0>
  __device__ __forceinline__ void preamble(T* bb, T* ax0, const T* dir = nullptr);
  // W <- A W in place.  COLLECTIVE; ends with W published
  template <class After, class Idle>
  __device__ __forceinline__ void ax(bool only_active, After&& after_sweep, Idle&& idle_work);
  __device__ __forceinline__ void ax(bool only_active);

  // ---- wg_sweep_rows.hip.h: the row-parallel sweeps (NWT)
  // array k of the Newton base trajectory in LDS, as seen by `thread`
  __device__ __forceinline__ Pair* base_pairs(int k, int thread) const;
  // nb -> LDS; call after the preamble's last barrier
  __device__ __forceinline__ void store_base();
  // array k of the base trajectory -> dst[SPL]
  __device__ __forceinline__ void load_base(int k, T* dst, int thread) const;
  // lanes of a row that own a stage
  __device__ __forceinline__ int so_lanes() const;
  // lane-private array `which` (0: U, 1: F(U,x+hf,t+h)) of the owned stages, as seen by `thread`
  __device__ __forceinline__ Pair* so_pairs(int which, int thread) const;
  // lane-private array `which` -> dst[NV]
  __device__ __forceinline__ void so_load(int which, T* dst, int thread) const;
  // src[NV] -> lane-private array `which` (lanes without a stage store nothing)
  __device__ __forceinline__ void so_store(int which, const T* src, int thread) const;
  // first controls by stage, [instance][stage] — 0: of U, 1: of U + h dUdt, 2: so_unow()
  __device__ __forceinline__ T* so_stage(int which) const;
  // the controls of stage 0, [j*IPW + i]
  __device__ __forceinline__ T* so_unow() const;
  // the row's new U: private array + the controls of stage 0
  __device__ __forceinline__ void so_put_U(const T* u) const;
  // HBM row [B][Lg] of this instance -> reg[NV] in stage ownership
  __device__ __forceinline__ void so_load_row(T* reg, const T* g) const;
  // reg[NV] in stage ownership -> HBM row [B][Lg]
  __device__ __forceinline__ void so_store_row(T* g, const T* reg) const;
  // first controls of U and of U + h d by stage, for the preamble's serial sweeps
  __device__ __forceinline__ void so_publish_u0(const T* d) const;
  // sin dl and cos dl - 1 of a Newton increment (newton_rot.hip.h); (s, c) turned by the angle they belong to
  static __device__ __forceinline__ void newton_rot_step(T dl, T* sn_out, T* cm1_out);
  static __device__ __forceinline__ void turn(T* s, T* c, T sn, T cm1);
  // costate recurrence + dH/du of the row's instance from the owned stages' x and trig, in registers
  template <int MODE>
  __device__ __forceinline__ void row_costate(const T* x0f, const T* y1, const T* x2f, const T* y3, const T* sd, const T* cd,
                                              const T* c1, const T* u, T dtau, T* out, int tid_o);
  // NWT = 2: one evaluation of F as two scans over the row
  template <int MODE>
  __device__ __forceinline__ void row_affine_sweep(const T* x0c, T dtau, const T* urow, T* out, bool run);
  // NWT = 2: the three evaluations in front of the solve, every row for itself
  __device__ __forceinline__ void preamble_affine(T* bb, T* ax0);
  // NWT = 1: serial state sweeps on waves 0-2, everything behind them per row in registers.  COLLECTIVE
  __device__ __forceinline__ void preamble_rows(T* bb, T* ax0, const T* du);
  // NWT = 1: out = A v for the row's instance, registers to registers; sets row_moved.  COLLECTIVE over the wave
  template <int MODE>
  __device__ __forceinline__ void row_newton_sweep(T dtau, const T* v, T* out, bool run);

  // ---- wg_gmres.hip.h: the solver
  // Hessenberg column k of one instance (reflectors, residual rotation); returns rho_e[k+1]
  static __device__ __forceinline__ T hess_column(T* Hi, T* gi, T* rhoi, int k, T hn, bool writer);
  // one round of modified Gram-Schmidt: Hk[i] = <v_i, w>, w -= Hk[i] v_i
  template <bool PARKED = false>
  __device__ __forceinline__ void mgs_round(T* w, T* Hk, const T* vrow_i, int i) const;
  // one term of x += V y
  __device__ __forceinline__ void axpy(T* acc, const T* y, const T* vj, int j) const;
  // the clamped ring's first requests for rows [first, end): all DEPTH buffers or none
  template <int DEPTH>
  __device__ __forceinline__ void ring_request(T (&buf)[DEPTH][NVEC], int first, int end) const;
  // the clamped ring's rounds: pre(rows in flight), body(row, index), refill, post()
  template <bool SCHED, int DEPTH, class Body, class Pre, class Post>
  __device__ __forceinline__ void ring_walk(T (&buf)[DEPTH][NVEC], int first, int end, Body&& body, Pre&& pre, Post&& post) const;
  // the steps of gmres() that stand alone (the others are regions of its frame, see there)
  // lazy_qr: all Hessenberg columns behind the loop, one per lane of the row
  __device__ __forceinline__ void qr_columns(Krylov K) const;
  // y from the leading ks x ks block (gmres.hpp:100-107), in the form k_max selects; y -> K.rho
  __device__ __forceinline__ void back_substitute(Krylov K, int ks) const;
  // Gmres::gmres around ax(): xv updated in place from b (bb) and A*x0 (ax0).  COLLECTIVE
  __device__ __forceinline__ void gmres(T* xv, const T* bb, const T* ax0);
  // status + small Krylov arrays of this row's instance -> HBM
  __device__ __forceinline__ void store_status() const;
};

// the members above are defined outside the class, in the phase headers, as
//   CGM_WGCTX_T [template <...>] __device__ __forceinline__ ret CGM_WGCTX::name(...) { ... }
#define CGM_WGCTX_T template <class M, class T, int IPW, int MAXM, bool LEAN, int PAR, int NWT>
#define CGM_WGCTX WgCtx<M, T, IPW, MAXM, LEAN, PAR, NWT>

}  // namespace cgm
