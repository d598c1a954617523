// The solver of the "wg" kernels — Hessenberg columns, the Gram-Schmidt rounds and the walk of the Krylov basis rows,
// Gmres::gmres itself and the export of its status: members of WgCtx (wg_ctx.hip.h).  gmres() calls the sweeps of
// whichever kernel it is compiled into.
#pragma once
#include "wg_ctx.hip.h"

namespace cgm {

// hn = sqrt(ss) and 1 / hn of the new basis row's squared norm from ONE reciprocal square root (row-Newton kernel): the
// library's sqrt is 22 dependent instructions around v_rsq_f64 and the division behind it 14 more around v_rcp_f64,
// all on the one chain every lane of the row waits for.  Here: the hardware's estimate y (about 2^-26 relative), one
// coupled step on g = ss y -> sqrt and h = y / 2 -> 1 / (2 sqrt), two corrections of g from its own residual (the
// library's steps, without its rescaling of arguments outside 2^+-767: ss is a squared norm of O(1) quantities, and a
// value so small that the steps lose accuracy is far below the breakdown bound whatever they return), and one
// correction of 2 h from the residual 1 - g (2 h).  Both values are within an ulp or two of the rounded ones (on the
// bench: the same bits, profiles/r10_iter_diet_ab.json).  ss = 0 (the breakdown case: a direction the rounding of
// U + h d absorbs) gives 0, a NaN or infinite ss a NaN — non-finite either way, as with sqrt.
__device__ __forceinline__ void norm_and_inverse(double ss, double* hn, double* inv) {
  const double y = __builtin_amdgcn_rsq(ss);
  const double g0 = ss * y, h0 = 0.5 * y;
  const double r0 = __builtin_fma(-h0, g0, 0.5);
  const double g1 = __builtin_fma(g0, r0, g0), h1 = __builtin_fma(h0, r0, h0);
  const double g2 = __builtin_fma(__builtin_fma(-g1, g1, ss), h1, g1);
  const double g3 = __builtin_fma(__builtin_fma(-g2, g2, ss), h1, g2);
  const double i1 = h1 + h1;
  *inv = __builtin_fma(__builtin_fma(-g3, i1, 1.0), i1, i1);
  *hn = ss > 0.0 ? g3 : ss;
}

// Hessenberg column k of one instance: stored reflectors, new reflector, residual rotation (gmres.hpp:71-90) — scalar
// work on the instance's small Krylov arrays in LDS.  hn = h(k+1,k).  Returns rho_e[k+1]; `writer` lanes store.
CGM_WGCTX_T
__device__ __forceinline__ T CGM_WGCTX::hess_column(T* Hi, T* gi, T* rhoi, int k, T hn, bool writer) {
  T* Hk = Hi + ((k * (k + 1)) >> 1);  // compact: column k = rows 0..k (h(k+1,k) arrives as `hn` and becomes 0)
  // The running entry stays in a register (a) and only ORIGINAL column entries / reflector words are read
  // from LDS, one step ahead: no store-to-load round trip through LDS between consecutive reflectors.
  // (the look-ahead reads one or two words past the column: the next column / array, in bounds, never used)
  T a = Hk[0];
  T g0n = gi[0], g1n = gi[1], g2n = gi[2], cn = Hk[1];
  for (int i = 0; i < k; ++i) {
    const T g0 = g0n, g1 = g1n, g2 = g2n, c = cn;
    g0n = gi[3 * i + 3], g1n = gi[3 * i + 4], g2n = gi[3 * i + 5], cn = Hk[i + 2];
    const ReflectorApply<T> p(g0, g1, g2, a, c);
    if (writer) Hk[i] = p.first();
    a = p.second();
  }
  const Reflector<T> q = reflector_make(a, hn);
  const ResidualRotate<T> e(q.g0, q.g1, q.g2, rhoi[k]);
  const T en = e.second();
  if (writer) {
    gi[3 * k] = q.g0, gi[3 * k + 1] = q.g1, gi[3 * k + 2] = q.g2;
    Hk[k] = q.sigma;
    rhoi[k] = e.first();
    rhoi[k + 1] = en;
  }
  return en;
}

// ---- the older Krylov basis rows, HBM -> registers (gmres(): the Gram-Schmidt rounds and x += V y) -----------------
// Rows V[first .. end-1] pass through DEPTH register buffers (the array's extent) with STATIC indices — no rotation by
// register moves: 20 v_mov per round, and a move would wait for the newest request.  A row is requested DEPTH rounds
// ahead and its buffer refilled right after its round, so each load has DEPTH-1 rounds (~1000 cycles) to arrive.

// One round of modified Gram-Schmidt (gmres.hpp:52-58): h(i,k) = <v_i, w> into Hk[i], w -= h(i,k) v_i
// PARKED: the row lives in the accumulator file (the kept rows and the ring buffers of the row-Newton kernel).  It is
// brought into arithmetic registers ONCE, for the dot product and the update: left to itself the allocator
// re-materialises the copy for the update — 2 NVEC v_accvgpr_read per pass, twice per round, all of them issue slots
// of a wave that has its SIMD to itself.  An opaque copy cannot be re-materialised.
CGM_WGCTX_T
template <bool PARKED>
__device__ __forceinline__ void CGM_WGCTX::mgs_round(T* w, T* Hk, const T* vrow_i, int i) const {
  T row[NVEC];
  const T* vi = vrow_i;
  if constexpr (PARKED) {
#pragma unroll
    for (int m = 0; m < NVEC; ++m) {
      row[m] = vrow_i[m];
      asm volatile("" : "+v"(row[m]));
    }
    vi = row;
  }
  T pa = 0, pb = 0;  // two partial sums: the fp64 FMA chain is latency-bound (8 cycles/op dependent)
#pragma unroll
  for (int m = 0; m < NVEC; m += 2) {
    pa += vi[m] * w[m];
    if (m + 1 < NVEC) pb += vi[m + 1] * w[m + 1];
  }
  const T hik = row16_sum(pa + pb);
#pragma unroll
  for (int m = 0; m < NVEC; ++m) w[m] = w[m] - vi[m] * hik;
  // (row-Newton kernel: all 16 lanes hold the same bits and store the same word — one store instead of a compare, an
  // exec mask saved and restored around it, and the read of r back from the accumulator file)
  if (ROW_ALL_STORE || r == 0) Hk[i] = hik;
}
// One term of x += V y (gmres.hpp:110-111): acc += v_j y_j
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::axpy(T* acc, const T* y, const T* vj, int j) const {
  const T yj = y[j];
#pragma unroll
  for (int m = 0; m < NVEC; ++m) acc[m] += vj[m] * yj;
}

// The clamped ring's first requests: all DEPTH buffers or none — a buffer past the last needed row re-reads that row.
CGM_WGCTX_T
template <int DEPTH>
__device__ __forceinline__ void CGM_WGCTX::ring_request(T (&buf)[DEPTH][NVEC], int first, int end) const {
  if (end > first) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) load_vec(buf[d], vrow(first + d < end ? first + d : end - 1));
  }
}
// The clamped ring's rounds, after ring_request(buf, first, end): DEPTH rounds per trip, the remaining < DEPTH rounds
// in a peeled tail that finds its rows already requested.  A round is pre(rows requested after this one and still in
// flight), body(row, its index), the refill, post().
// The refill is UNCONDITIONAL, its row index clamped to the last needed row (the last trip re-reads it): a guard would
// be a branch between a load and its use, and the compiler then waits with vmcnt(0) — i.e. also for the row it has
// just requested, and nothing overlaps.  So the walk leaves up to DEPTH requests nobody consumes: see drain_stream.
// SCHED: a sched_barrier in front of every round keeps the requests TOGETHER and ahead of the arithmetic — under
// register pressure the scheduler otherwise sinks every load next to its use, one exposed round trip per element.
CGM_WGCTX_T
template <bool SCHED, int DEPTH, class Body, class Pre, class Post>
__device__ __forceinline__ void CGM_WGCTX::ring_walk(T (&buf)[DEPTH][NVEC], int first, int end, Body&& body, Pre&& pre, Post&& post) const {
  int i = first;
  for (; i + DEPTH <= end; i += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      if constexpr (SCHED) __builtin_amdgcn_sched_barrier(0);
      pre(DEPTH - 1);
      body(buf[d], i + d);
      const int nxt = i + d + DEPTH;
      load_vec(buf[d], vrow(nxt < end ? nxt : end - 1));
      post();
    }
  }
#pragma unroll
  for (int d = 0; d < DEPTH - 1; ++d)
    if (i + d < end) {
      pre(DEPTH - 1 - d);
      body(buf[d], i + d);
      post();
    }
}

// gmres.hpp:71-90 for all columns at once (lazy_qr): lane c of the row owns column c and carries its running entry `a`
// through the reflectors in order — step i: lane i turns (a, h(i+1,i)) into reflector i and leaves it in LDS, every
// lane reads it back (same wave: LDS operations complete in order), the lanes c > i apply it to their column, and all
// lanes advance the residual vector.  Per column the arithmetic and its order are those of hess_column; the serial
// chain is k_max steps instead of k_max^2 / 2.
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::qr_columns(Krylov K) const {
  const int kmax = P.kmax;
  const int rs = S.reason[inst], nx = S.nax[inst];
  const int n_col = !valid ? 0 : (rs == 0 ? nx : nx - 1);  // (a breakdown leaves its own column unrotated, :63-65)
  const int c = r < kmax ? r : 0;
  T* Hc = K.H + hoff(c);
  const bool mine = r < n_col;
  T a = mine ? Hc[0] : T(0);
  T ek = K.rho[0];
  for (int i = 0; i < kmax; ++i) {
    if (!__any(i < n_col)) break;
    const bool on = i < n_col;
    const T cN = K.g[3 * i + 1];
    const Reflector<T> q = reflector_make(a, cN);
    if (on && r == i) {
      K.g[3 * i] = q.g0, K.g[3 * i + 2] = q.g2;
      Hc[i] = q.sigma;
    }
    const T g0 = K.g[3 * i], g1 = cN, g2 = K.g[3 * i + 2];
    // (ResidualRotate and ReflectorApply of tick_common.hip.h, spelled out: through them the code of the two
    // row-parallel kernels changes — profiles/wg_solver_steps_identity.md)
    const T beta_r = g0 * ek * g2;
    if (on && r == 0) K.rho[i] = ek - beta_r * g0;
    ek = on ? -beta_r * g1 : ek;
    if (mine && r > i) {
      const T cn = Hc[i + 1];
      const T beta = (g0 * a + g1 * cn) * g2;
      Hc[i] = a - beta * g0;
      a = cn - beta * g1;
    }
  }
  if (r == 0 && n_col > 0) K.rho[n_col] = ek;
}

// Back substitution (gmres.hpp:100-107), column-oriented over the lanes of the row: lane j owns e_j; step i
// (descending) turns e_i into y_i = e_i / H_ii, broadcasts it inside the row (ds_bpermute) and every lane j < i
// subtracts H(j,i) y_i — for a fixed j the subtractions come in the reference's order (i = ks-1 ... j+1).
// One LDS read + one crossbar round trip per step instead of a dependent LDS chain of length ks-i on lane 0.
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::back_substitute(Krylov K, int ks) const {
  const int kmax = P.kmax;
  T* const Hi = K.H;
  T* const rhoi = K.rho;
  if (kmax <= 15) {
    T e = r < ks ? rhoi[r] : T(0);
    const int row_lane0 = (threadIdx.x & 63) & ~15;
    for (int i = ks - 1; i >= 0; --i) {
      // (r > i + 1 reads words of the following columns / arrays: in bounds, only used where r < i)
      const T hii = Hi[hoff(i) + i], hji = Hi[hoff(i) + r];
      const T y = e / hii;                                   // meaningful in lane i
      const T yi = row_bcast(y, row_lane0 + i);
      e = r < i ? e - hji * yi : (r == i ? y : e);
    }
    if (r < ks) rhoi[r] = e;
    if (r == 0) S.ksolve[inst] = ks;
  } else if (kmax <= 31) {
    // the same with TWO unknowns per lane (e_r and e_(r+16)): k_max = 20 of the long-horizon configuration — on lane 0
    // alone the 200 dependent LDS steps of this solve were 2.7 % of that tick
    T e0 = r < ks ? rhoi[r] : T(0), e1 = r + 16 < ks ? rhoi[r + 16] : T(0);
    const int row_lane0 = (threadIdx.x & 63) & ~15;
    for (int i = ks - 1; i >= 0; --i) {
      // (rows beyond i + 1 read words of the following columns / arrays: in bounds, only used where the row is < i)
      const T hii = Hi[hoff(i) + i], h0 = Hi[hoff(i) + r], h1 = Hi[hoff(i) + r + 16];
      const bool hi_half = i >= 16;                           // (uniform) which of the lane's two unknowns e_i is
      const T y = (hi_half ? e1 : e0) / hii;                  // meaningful in lane i & 15
      const T yi = row_bcast(y, row_lane0 + (i & 15));
      e0 = r < i ? e0 - h0 * yi : (r == i ? y : e0);
      e1 = r + 16 < i ? e1 - h1 * yi : (r + 16 == i ? y : e1);
    }
    if (r < ks) rhoi[r] = e0;
    if (r + 16 < ks) rhoi[r + 16] = e1;
    if (r == 0) S.ksolve[inst] = ks;
  } else if (r == 0) {
    for (int i = ks - 1; i >= 0; --i) {
      T ei = rhoi[i];
      for (int j = ks - 1; j > i; --j) ei -= Hi[hoff(j) + i] * rhoi[j];
      rhoi[i] = ei / Hi[hoff(i) + i];
    }
    S.ksolve[inst] = ks;
  }
}

// Gmres::gmres (gmres.hpp:28-112).  In: x (registers `xv`), b (`bb`) and A*x0 (`ax0`), all in the row layout.
// Out: xv updated.  All threads of the block must call this (it contains workgroup barriers).
// The QR of all columns behind the loop and the back substitution are members (above).  The start, the iteration
// gate, the mat-vec, the Gram-Schmidt rounds, the new basis row and the update of x are regions of this one frame, and
// NBUF .. PARK its locals: as members, or with the constants in the class, every kernel's register allocation changed
// (profiles/wg_solver_steps_identity.md has the trials), and the kernels are held to the code they had.
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::gmres(T* xv, const T* bb, const T* ax0) {
  const int kmax = P.kmax, k1 = kmax + 1;
  T* Hi = S.H + inst * P.Hp;  // compact: column k has k+1 entries (rows 0..k) at offset k(k+1)/2; h(k+1,k): S.hsub
  T* rhoi = S.rho + inst * k1;
  T* gi = S.g + inst * 3 * kmax;
  T vcur[NVEC], w[NVEC];
  // Ring of NBUF register buffers for the older basis vectors of the full-plan kernels, bases up to KRING rows: the
  // first NBUF rows are requested before the sweep starts.
  constexpr int NBUF = MAXM <= 10 ? 3 : 2, KRING = 12;
  // row buffers of the streaming loops (lean kernels, k_max > KRING).  Three buffers were measured as well: the 256-register
  // kernels then spill inside the Arnoldi loop (fp32 N = 100: 384 spilled VGPRs, cfg 5 526 -> 609 us/tick)
  constexpr int SDEPTH = 2;
  // The streaming loops end with a row request nobody consumes (their unconditional look-ahead).  In the kernels that
  // ALSO carry the register ring (not lean: k_max picks the form at run time) the compiler must assume those registers
  // are still being written wherever it reuses them on the ring path — it reuses them in the sweeps — and, the counter
  // being in order, it put s_waitcnt vmcnt(0) at the start of wave 0's state sweep (draining the store of the new
  // basis row) and at the start of its costate sweep (waiting for the ring rows requested just before, which are not
  // needed until the Gram-Schmidt rounds).  Draining the look-ahead where the streaming loop ends keeps the ring path
  // free of both: s_waitcnt vmcnt(0), other counters untouched.
  auto drain_stream = [] {
    if constexpr (!LEAN) __builtin_amdgcn_s_waitcnt(cgm_vmcnt_imm(0));
  };
  // The first NKEEP basis vectors never leave the row lanes' registers (the compiler parks them in the AGPR file): v_0
  // and v_1 are read again in every later iteration — 17 of the 55 Gram-Schmidt row reads of a k = 10 solve — and the
  // Gram-Schmidt rounds are bounded by the CU's 64 B/clk vector-memory path, not by issue.  The ring then serves the
  // rows from NKEEP on.  Pays for itself only where registers are left: the one-workgroup-per-CU kernels with short
  // vectors, with the solution vector parked in HBM for the duration of the loop like the long-vector kernels do.
  constexpr int NKEEP = (!LEAN && MAXM <= 10) ? 2 : 0;
  T vkeep[NKEEP > 0 ? NKEEP : 1][NVEC];
  // Row-Newton kernel: the ring rounds and the ring part of the x update are the clamped ring (ring_walk over the NBUF
  // buffers, rows NKEEP on) instead of twelve straight-line cases.  Of the look-ahead nobody consumes, the requests of
  // the rounds are drained by the s_waitcnt vmcnt(0) in front of the next iteration's requests (request_rows, at the
  // loop top in this form: no sweep inherits them; an explicit drain behind the rounds was measured, 86.6 vs 86.1 us
  // per tick), those of the x update where its walk ends.  A property of the kernel (template-selected).
  constexpr bool COMPACT = NWT == 1 && NKEEP > 0;
  // (lambdas here, not members like ring_walk: keep_rows and ring_cases capture vkeep, and cases_request stays next to
  // the walker whose rows it requests)
  auto keep_rows = [&](int n, auto&& body) {  // the rounds on the rows that stayed in registers
#pragma unroll
    for (int i = 0; i < NKEEP; ++i)
      if (i < n) body(vkeep[i], i);
  };
  // The other full-plan kernels walk rows 0 .. n-1 in one straight-line instance per n <= KRING: with no branch between
  // a load and its use the compiler counts the outstanding loads exactly (s_waitcnt vmcnt(2*MAXM) in the steady state
  // instead of vmcnt(0)), so the requests are exact as well — no clamping, a guarded refill, nothing left in flight.
  auto cases_request = [&](T (&buf)[NBUF][NVEC], int n) {
#pragma unroll
    for (int i = 0; i < NBUF; ++i)
      if (i + NKEEP < n) load_vec(buf[i], vrow(i + NKEEP));
  };
  auto ring_cases = [&](T (&buf)[NBUF][NVEC], int n, auto&& body, auto&& pre, auto&& post) {
    auto rounds = [&](auto kc) {
      constexpr int K = decltype(kc)::value;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        if constexpr (NKEEP > 0) {
          if (i < NKEEP) {
            body(vkeep[i < NKEEP ? i : 0], i);
            continue;
          }
        }
        pre(K - 1 - i < NBUF - 1 ? K - 1 - i : NBUF - 1);
        body(buf[(i - NKEEP) % NBUF], i);
        if (i + NBUF < K) load_vec(buf[(i - NKEEP) % NBUF], vrow(i + NBUF));
        post();
      }
    };
#define CGM_KCASE(n) \
case n:            \
  rounds(std::integral_constant<int, n>{}); \
  break;
    switch (n) {
      CGM_KCASE(1) CGM_KCASE(2) CGM_KCASE(3) CGM_KCASE(4) CGM_KCASE(5) CGM_KCASE(6)
      CGM_KCASE(7) CGM_KCASE(8) CGM_KCASE(9) CGM_KCASE(10) CGM_KCASE(11) CGM_KCASE(12)
      default: break;
    }
#undef CGM_KCASE
  };
  static_assert(KRING == 12, "ring_cases has one case per basis length");
  const Krylov K{Hi, rhoi, gi};  // for the steps that are members (qr_columns, back_substitute)
  auto no_stamp = [](auto...) {};
  // Diagnostic build: the Gram-Schmidt stamp split in three — 28 closes an explicit wait for the ring row a round is
  // about to use (the `younger` rows requested after it stay in flight, as in the product build), 29 the ring round
  // itself (arithmetic, instruction fetch, refill request), 7 keeps the register rounds and the norm.
  auto stamp_row_wait = [&](int younger) {
#ifdef CGM_STAMPS
    if constexpr (NWT == 1) {
      CGM_STAMP(*this, 7);
      constexpr int LPR = NVEC / 2;  // 16-byte loads per row and lane
      switch (younger) {
        case 0: __builtin_amdgcn_s_waitcnt(cgm_vmcnt_imm(0)); break;
        case 1: __builtin_amdgcn_s_waitcnt(cgm_vmcnt_imm(LPR)); break;
        default: __builtin_amdgcn_s_waitcnt(cgm_vmcnt_imm(2 * LPR)); break;
      }
      CGM_STAMP(*this, 28);
    }
#endif
  };
  auto stamp_ring_round = [&] {
#ifdef CGM_STAMPS
    if constexpr (NWT == 1) CGM_STAMP(*this, 29);
#endif
  };
  // workgroup-uniform; longer bases use the plain streaming loop.  So does the lean plan: with 256 registers per wave the
  // twelve straight-line copies of the rounds push everything that lives across them (U, the sweep constants) into
  // scratch — in every block of the kernel, executed or not.
  const bool preload = !LEAN && kmax <= KRING;
  bool active = valid;
  // Long vectors: x is not touched again before the final update (gmres.hpp:110-111), and 2*MAXM more live registers
  // push the Gram-Schmidt rounds into AGPR copies and scratch (profiles/r02_isa_summary.md).  Park it in HBM
  // (own row, same thread writes and reads it back: program order) and fetch it back behind the back substitution.
  T* const park_row = P.park + size_t(blockIdx.x * IPW + inst) * P.Lv;
  constexpr bool PARK = MAXM > 10 || (LEAN && sizeof(T) == 8) || NKEEP > 0 || NWT != 0;  // (lean fp64: 256 registers per wave)
  if constexpr (PARK) store_vec(park_row, xv);
  // r0 = b - A x0 ; rho = ||r0||      gmres.hpp:33-37
  {
    T ss = 0;
#pragma unroll
    for (int m = 0; m < NVEC; ++m) {
      vcur[m] = bb[m] - ax0[m];
      ss += vcur[m] * vcur[m];
    }
    const T rho0 = sqrt_t<T>(row16_sum(ss));
    if (r == 0) rhoi[0] = rho0;
    if (active && !finite_t(rho0)) {  // CGMRES_HIP_EXIT_NONFINITE (row-uniform; see poison_nonfinite in tick_lane.hip.h)
      active = false;
      if (r == 0) S.reason[inst] = 4;
    }
    if (active && rho0 < P.tol) {  // gmres.hpp:39-41
      active = false;
      if (r == 0) S.reason[inst] = 2;
    }
    if (active) {
      const T inv = T(1.0) / rho0;  // gmres.hpp:44
#pragma unroll
      for (int m = 0; m < NVEC; ++m) vcur[m] = vcur[m] * inv;
      store_vec(vrow(0), vcur);
      if constexpr (NKEEP > 0) {
#pragma unroll
        for (int m = 0; m < NVEC; ++m) vkeep[0][m] = vcur[m];
      }
      if constexpr (!ROW_NEWTON) publish_direction(vcur);  // (stage ownership: v_k is where the sweep needs it)
    }
    if (r == 0) S.flag[inst] = active ? 1 : 0;
  }
  // Fixed-k mode (tol = 0: no residual test can succeed, every running instance does all k_max iterations): the
  // Hessenberg column of iteration k is not needed before the final triangular solve, so it is taken off the critical
  // path — 16 lanes of wave 1 (one per instance) do column k-1 while wave 0 runs the first chunk of sweep k, where
  // the coefficient waves would otherwise wait; the last column is done in place.  With tol > 0 the column decides
  // whether the next mat-vec runs at all (gmres.hpp:93-95) and stays where the reference has it.
  // (NWT: the rows of a workgroup do not meet inside the loop at all — every row does its own column in place)
  const bool defer_hess = NWT == 0 && IPW * 16 >= 128 && P.tol == T(0);  // workgroup-uniform
  // NWT in fixed-k mode: no column is needed before the triangular solve either, and no wave has idle time to hide one
  // in — the loop only records h(k+1,k) (in the slot of the reflector's second word, which is what it becomes) and
  // the QR factorisation of the whole Hessenberg matrix follows the loop, the columns spread over the lanes of the row.
  const bool lazy_qr = NWT != 0 && P.tol == T(0);
  int k = 0;
  for (; k < kmax; ++k) {  // gmres.hpp:46
    CGM_STAMP(*this, 14);
    if constexpr (LEAN || NWT != 0 || MAXM > 10) {
      // Whatever derives from the thread index alone is invariant over the whole launch, gets hoisted to the kernel
      // entry and — there being no room in these kernels — spilled; its reloads inside the iteration sit behind
      // s_waitcnt vmcnt(0), i.e. wait for the basis rows in flight.  Opaque copies once per iteration: the few integer
      // operations are redone instead.  (Spilled VGPRs: lean pendulum fp64 91 -> 2, lean two-mass system 81 -> 0,
      // lean pendulum fp32 k = 20 86 -> 0, the row-parallel kernel 108 -> 0 and 103.6 -> 99.8 us per tick; the
      // short-vector serial-sweep kernels have next to none to lose and are 1 % slower with it: left alone.)
      asm volatile("" : "+v"(tid), "+v"(inst), "+v"(r), "+v"(b));
    }
    if constexpr (NWT != 0) {
      // Row-parallel sweeps: everything an iteration touches in LDS — the row of W, the row's small Krylov arrays —
      // is written and read by the 16 lanes of ONE row, i.e. inside one wave, whose LDS operations complete in
      // order: no workgroup barrier in the loop, and every wave leaves it when ITS four rows are done.
      if (!__any(active)) break;
    } else {
    // Workgroup barrier that orders LDS only (W and the flags are what the sweep lanes need).  __syncthreads()
    // would also drain this wave's HBM store of the new basis row (s_waitcnt vmcnt(0)) — nobody else reads it.
    lds_barrier();
    {
      // (16-byte reads, all requested before the first is used: left as IPW scalar reads the compiler issued them as
      // eight ds_read2_b32 into ONE register pair, each behind s_waitcnt lgkmcnt(0) — eight LDS round trips in a row on
      // every wave, at the top of every iteration.  The int arrays start on a 16-byte boundary: every array in front of
      // them is a multiple of IPW scalars.)
      static_assert(IPW % 4 == 0, "flags are read four at a time");
      const int4* f4 = reinterpret_cast<const int4*>(__builtin_assume_aligned(S.flag, 16));
      int4 fl[IPW / 4];
#pragma unroll
      for (int j = 0; j < IPW / 4; ++j) fl[j] = f4[j];
      act_i = S.flag[tid & (IPW - 1)], act_q = S.flag[(tid & 63) >> 2];  // (IPW = 8: lanes 32.. read `reason` words, unused)
      int any = 0;
#pragma unroll
      for (int j = 0; j < IPW / 4; ++j) any |= (fl[j].x | fl[j].y) | (fl[j].z | fl[j].w);
      if (!any) break;
    }
    }
    CGM_STAMP(*this, 15);
    // The first basis vectors this iteration needs are requested from HBM/L2 early.  Waves 1-3 do it NOW (the rows
    // arrive while wave 0 sweeps); wave 0 — four waves' row requests take the CU's address unit ~800 cycles, which
    // would delay the sweep — does it after its state sweep, where it otherwise waits for the coefficient tail.
    T vbuf[NBUF][NVEC];
    // (vmcnt(0) first: the two call sites below write the same registers, so without it the compiler must assume the
    // other site's requests are still in flight — with an in-order counter and conditional requests that leaves it
    // only s_waitcnt vmcnt(0) in front of EVERY row: each request waited for the previous row to arrive, on wave 0
    // right after its state sweep.  What is really outstanding here is this thread's store of the newest basis row,
    // at most.  Together with drain_stream: state phase -0.8 k cycles per sweep, headline 134.2 -> 133.1 us/tick.)
    auto request_rows = [&]() {
      if (preload && active) {
        __builtin_amdgcn_s_waitcnt(cgm_vmcnt_imm(0));
        if constexpr (COMPACT) ring_request(vbuf, NKEEP, k);
        else cases_request(vbuf, k);
      }
    };
    if (NWT == 0 && tid >= 64) request_rows();
    auto deferred_column = [&]() {  // column k-1 of instance j = tid-64, if iteration k-1 produced one for it
      const int j = tid - 64;
      if (defer_hess && k > 0 && j >= 0 && j < IPW && S.reason[j] == 0 && S.nax[j] == k) {
        T* Hj = S.H + j * P.Hp;
        hess_column(Hj, S.g + j * 3 * kmax, S.rho + j * k1, k - 1, S.hsub[j], true);
      }
    };
    if constexpr (NWT != 0) {
      CGM_STAMP(*this, 3);
      request_rows();
      if constexpr (NWT == 2) {
        // (a light sweep: the rows may be in flight across it)
        row_affine_sweep<F_AX>(S.xh, dtau_h, S.W + inst * P.Lp, S.W, active);
      } else {
        static_assert(COMPACT, "the row-Newton sweep goes with the clamped ring");
        // (the ring sits in AGPRs whichever way — requested here, a whole sweep ahead, the first NBUF rows have arrived
        // when their rounds come: 86.5 vs 87.6 us per tick against a request between the Newton iterations and the
        // costate scans, profiles/r07_gs_ab.json)
        row_newton_sweep<F_AX>(dtau_h, vcur, w, active);  // :48  w <- A v_k, registers to registers
      }
      CGM_STAMP(*this, 6);
    } else {
      ax(true, request_rows, deferred_column);  // :48  W <- A v_k, in place
    }
    if (active) {
      if constexpr (!ROW_NEWTON) {
        lds_to_reg(w, S.W);
        if constexpr (NWT != 0) CGM_STAMP_LDS(*this, 2);
      }
      if constexpr (NWT != 0) {
        if (!row_moved) {  // (see publish_direction)
#pragma unroll
          for (int m = 0; m < NVEC; ++m) w[m] = T(0);
        }
      }
      T* Hk = Hi + hoff(k);
      // modified Gram-Schmidt, gmres.hpp:52-58, in order; v_k itself is still in registers
      auto round = [&](const T* vi, int i) { mgs_round(w, Hk, vi, i); };
      if (preload) {
        if constexpr (COMPACT) {
          auto round_parked = [&](const T* vi, int i) { mgs_round<true>(w, Hk, vi, i); };
          keep_rows(k, round_parked);
          if (k > NKEEP) ring_walk<false>(vbuf, NKEEP, k, round_parked, stamp_row_wait, stamp_ring_round);
        } else {
          ring_cases(vbuf, k, round, stamp_row_wait, stamp_ring_round);
        }
      } else {
        // (register-starved lean kernels: v_k is streamed back from its row like the older ones instead of being
        // held in registers through the whole sweep; the row was written by this same thread)
        T vq[SDEPTH][NVEC];
        const int kk = VK_IN_REGS ? k : k + 1;
        ring_request(vq, 0, kk);
        ring_walk<true>(vq, 0, kk, round, no_stamp, no_stamp);
        drain_stream();
      }
      if constexpr (VK_IN_REGS) round(vcur, k);
      T na = 0, nb = 0;
#pragma unroll
      for (int m = 0; m < NVEC; m += 2) {
        na += w[m] * w[m];
        if (m + 1 < NVEC) nb += w[m + 1] * w[m + 1];
      }
      CGM_STAMP(*this, 7);
      constexpr bool RSQ_NORM = ROW_NEWTON && std::is_same<T, double>::value;
      T hn, inv_hn = T(0);  // :60, and :67 with it in the row-Newton kernel
      if constexpr (RSQ_NORM) norm_and_inverse(row16_sum(na + nb), &hn, &inv_hn);
      else hn = sqrt_t<T>(row16_sum(na + nb));
      if (ROW_ALL_STORE || r == 0) {
        S.hsub[inst] = hn;
        S.nax[inst] = k + 1;
      }
      if (abs_t(hn) < T(DBL_EPSILON) || !finite_t(hn)) {  // :63-65 breakdown: x untouched; non-finite: x <- NaN below
        active = false;
        if (r == 0) {
          S.reason[inst] = finite_t(hn) ? 3 : 4;
          S.flag[inst] = 0;
        }
      } else {
        const T inv = RSQ_NORM ? inv_hn : T(1.0) / hn;  // :67
#pragma unroll
        for (int m = 0; m < NVEC; ++m) vcur[m] = w[m] * inv;
        store_vec(vrow(k + 1), vcur);
        if constexpr (NKEEP > 1) {
#pragma unroll
          for (int q = 1; q < NKEEP; ++q)
            if (k + 1 == q) {
#pragma unroll
              for (int m = 0; m < NVEC; ++m) vkeep[q][m] = vcur[m];
            }
        }
        if constexpr (!ROW_NEWTON) {
          if constexpr (NWT != 0) CGM_STAMP(*this, 8);
          publish_direction(vcur);
          if constexpr (NWT != 0) CGM_STAMP_LDS(*this, 25);
        }
        // Hessenberg column k: stored reflectors, new reflector, residual rotation (:71-90) — scalar work.
        // Every lane of the row computes it from the same LDS words (broadcast reads; a row never straddles
        // a wave, and LDS operations of one wave complete in order), lane 0 writes back: the convergence
        // decision is therefore row-uniform.
        CGM_STAMP(*this, 8);
        // (deferred in fixed-k mode, except for the last column: no sweep follows it)
        const bool column_now = !lazy_qr && (!defer_hess || k + 1 == kmax);
        if (lazy_qr && r == 0) gi[3 * k + 1] = hn;
        const T en = column_now ? hess_column(Hi, gi, rhoi, k, hn, r == 0) : T(1);
        CGM_STAMP(*this, 9);
        if (column_now && abs_t(en) < P.tol) {  // :93-95 — converged: column k is NOT used by the solve
          active = false;
          if (r == 0) {
            S.reason[inst] = 1;
            S.ksolve[inst] = k;
            S.flag[inst] = 0;
          }
        }
      }
    }
  }
  if constexpr (NWT == 0) __syncthreads();  // (NWT: the status words of a row are its own wave's)
  if constexpr (NWT != 0) {
    if (lazy_qr) qr_columns(K);  // :71-90
  }
  CGM_STAMP(*this, 10);
  // natural exit: every column is used
  const int reason = S.reason[inst];
  const int ks = reason == 0 ? (valid ? kmax : 0) : (reason == 1 ? S.ksolve[inst] : 0);
  // the first basis rows of the x update are requested before the (serial) back substitution
  T vbx[NBUF][NVEC];
  if (preload && valid && reason <= 1) {
    if constexpr (COMPACT) ring_request(vbx, NKEEP, ks);
    else cases_request(vbx, ks);
  }
  if (valid && reason <= 1) back_substitute(K, ks);  // :100-107
  if constexpr (PARK) load_vec(xv, park_row);
  if constexpr (NWT == 0) __syncthreads();  // (NWT: y is written and read by the lanes of one row, i.e. one wave)
  CGM_STAMP(*this, 11);
  if (valid && reason <= 1) {
    // x += V[:,0:ks] y  (gmres.hpp:110-111), accumulated j-ascending from 0 like matrix.hpp:82-91
    T acc[NVEC];
#pragma unroll
    for (int m = 0; m < NVEC; ++m) acc[m] = T(0.0);
    auto term = [&](const T* vj, int j) { axpy(acc, rhoi, vj, j); };
    if (preload) {  // the Gram-Schmidt rounds' walk, on the rows requested before the back substitution
      if constexpr (COMPACT) {
        keep_rows(ks, term);
        if (ks > NKEEP) {
          ring_walk<false>(vbx, NKEEP, ks, term, no_stamp, no_stamp);
          drain_stream();
        }
      } else {
        ring_cases(vbx, ks, term, no_stamp, no_stamp);
      }
    } else {
      T vq[SDEPTH][NVEC];
      ring_request(vq, 0, ks);
      ring_walk<true>(vq, 0, ks, term, no_stamp, no_stamp);
      drain_stream();
    }
#pragma unroll
    for (int m = 0; m < NVEC; ++m) xv[m] = xv[m] + acc[m];
  }
  if (valid && reason == 4) {  // CGMRES_HIP_EXIT_NONFINITE: what the reference's fall-through ends with
#pragma unroll
    for (int m = 0; m < NVEC; ++m) xv[m] = vec_elem(m) < P.L ? quiet_nan<T>() : T(0);
  }
}

// status + small Krylov arrays of this row's instance -> HBM
CGM_WGCTX_T
__device__ __forceinline__ void CGM_WGCTX::store_status() const {
  if (!valid) return;
  const int kmax = P.kmax, k1 = kmax + 1, ks_all = k1 * k1 + k1 + 3 * kmax;
  T* dst = P.kry + size_t(b) * ks_all;
  const T* Hi = S.H + inst * P.Hp;  // compact columns -> the reference's (k_max+1) x (k_max+1) column-major array
  for (int q = r; q < k1 * k1; q += 16) {
    const int col = q / k1, row = q - col * k1;
    // rows 0..col from the compact columns; the subdiagonal entry is 0 once the column has been rotated (gmres.hpp:85) —
    // a breakdown leaves at column nax-1 BEFORE its rotation (gmres.hpp:63-65): there it still holds h(k+1,k)
    T v = (col < kmax && row <= col) ? Hi[((col * (col + 1)) >> 1) + row] : T(0);
    if (row == col + 1 && col + 1 == S.nax[inst] && S.reason[inst] == 3) v = S.hsub[inst];
    dst[q] = v;
  }
  for (int q = r; q < k1; q += 16) dst[k1 * k1 + q] = S.rho[inst * k1 + q];
  for (int q = r; q < 3 * kmax; q += 16) dst[k1 * k1 + k1 + q] = S.g[inst * 3 * kmax + q];
  if (r == 0) {
    P.n_ax[b] = S.nax[inst];
    P.reason[b] = S.reason[inst];
  }
}

}  // namespace cgm
