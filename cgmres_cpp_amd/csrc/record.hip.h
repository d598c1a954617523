// The record of a closed loop (cgmres_hip_closed_loop_device_rec) and the ensemble of a batch
// (cgmres_hip_ensemble_device): the log rows of one recorded tick and the statistics over its `batch` instances.
//
// Kernels of their own, launched BETWEEN the tick launches on the handle's stream: no tick kernel, parameter struct or
// kernel argument knows about them.  They read what every mapping keeps in caller order and instance-major — the caller's
// x [B][nx] and u [B][nu], the status arrays n_ax [B] and reason [B] — so they are independent of model and mapping;
// nx, nu and k_max are run-time arguments, and a user model gets them from the library, not from its plugin.
//
// record_kernel, kRecordBlock lanes per workgroup, one pass over the row of a record:
//   * the log rows that are wanted: flat, coalesced copies of [B][nx], [B][nu], [B], [B];
//   * the ensemble: a lane walks the instances b = wg*kRecordBlock + lane, strided by the grid.  Finiteness of the WHOLE
//     row (nx + nu values) is decided first; an instance counts when all are finite.  Per component c (x, then u) the
//     lane keeps {s1, s2, min, max} of z = double(value) - centre[c] (min / max of the value itself) in registers, for
//     kRecordGroup components at a time (a model with more is walked in groups: nothing spills).  A lane past the batch
//     loads the row of the batch's last instance and contributes the identity; no branch goes around a load.
//     Wave: DPP steps inside the rows of 16, the four rows in lane order.  Workgroup: the waves through LDS, in wave
//     order.  One partial per workgroup goes to the context's scratch with plain vector stores.
//   * the counts: integer LDS atomics into [k_max + 7] bins, one integer partial per workgroup.
// record_combine_kernel, one workgroup: adds the partials IN WORKGROUP ORDER.  No floating-point atomic anywhere, every
// tree is fixed by (B, nx, nu): two runs from the same state give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dpp.hip.h"

namespace cgm {

constexpr int kRecordBlock = 256;    // lanes of a workgroup = instances it covers per grid step (exported: W of the tests)
constexpr int kRecordGroup = 8;      // components whose {s1, s2, min, max} a lane holds at a time
constexpr int kRecordMaxGrid = 64;   // workgroups at most: the partials one combine workgroup adds
constexpr int kRecordMaxBins = 8192; // k_max + 7 at most: the LDS histogram

template <class T>
struct RecordArgs {
  int B, nx, nu, kmax;
  const T *x, *u;                  // [B][nx], [B][nu]
  const int32_t *n_ax, *reason;    // [B]
  T *x_log, *u_log;                // this record's rows, or null
  int32_t *n_ax_log, *reason_log;  // or null
  const double* centre;            // [nx+nu] or null = zeros
  double* part_m;                  // [grid][nx+nu][4] workgroup partials; null: no moments wanted
  int32_t* part_c;                 // [grid][kmax+7]; null: no counts wanted
};

struct RecSum {
  __device__ static double op(double a, double b) { return a + b; }
};
struct RecMin {
  __device__ static double op(double a, double b) { return b < a ? b : a; }
};
struct RecMax {
  __device__ static double op(double a, double b) { return b > a ? b : a; }
};
// All 64 lanes of a wave -> lane 0 (every lane of row 0, in fact): DPP inside the rows of 16, then rows 0..3 in order.
template <class Op>
__device__ __forceinline__ double record_wave_reduce(double v) {
  v = Op::op(v, dpp_move<DPP_QUAD_SWAP1>(v));
  v = Op::op(v, dpp_move<DPP_QUAD_SWAP2>(v));
  v = Op::op(v, dpp_move<DPP_ROW_HALF_MIRROR>(v));
  v = Op::op(v, dpp_move<DPP_ROW_MIRROR>(v));
  double r = __shfl(v, 0);
  r = Op::op(r, __shfl(v, 16));
  r = Op::op(r, __shfl(v, 32));
  r = Op::op(r, __shfl(v, 48));
  return r;
}

template <class T>
__device__ __forceinline__ bool record_finite(T v) {
  return fabs(double(v)) <= 1.7976931348623157e308;  // false for NaN and +-Inf
}

template <class T>
__global__ __launch_bounds__(kRecordBlock) void record_kernel(RecordArgs<T> A) {
  extern __shared__ int32_t rec_bins[];                       // [kmax+7] when counts are wanted
  __shared__ double rec_w[kRecordBlock / 64][kRecordGroup][4];  // the waves' partials of one component group
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = A.B, nx = A.nx, nu = A.nu, nc = nx + nu, nbins = A.kmax + 7;
  const size_t gsz = size_t(gridDim.x) * kRecordBlock, g0 = size_t(blockIdx.x) * kRecordBlock + tid;

  // ---- the log rows: flat copies ----
  if (A.x_log)
    for (size_t q = g0; q < size_t(B) * nx; q += gsz) A.x_log[q] = A.x[q];
  if (A.u_log)
    for (size_t q = g0; q < size_t(B) * nu; q += gsz) A.u_log[q] = A.u[q];
  if (A.n_ax_log)
    for (size_t q = g0; q < size_t(B); q += gsz) A.n_ax_log[q] = A.n_ax[q];
  if (A.reason_log)
    for (size_t q = g0; q < size_t(B); q += gsz) A.reason_log[q] = A.reason[q];
  if (!A.part_m && !A.part_c) return;

  if (A.part_c) {
    for (int q = tid; q < nbins; q += kRecordBlock) rec_bins[q] = 0;
    __syncthreads();
  }
  // every lane of the workgroup makes the same number of steps (no barrier sits inside the loop, but no lane idles either)
  const int steps = int((size_t(B) + gsz - 1) / gsz);
  const int ngroups = A.part_m ? (nc + kRecordGroup - 1) / kRecordGroup : 1;
  for (int grp = 0; grp < ngroups; ++grp) {
    const int c0 = grp * kRecordGroup;
    double s1[kRecordGroup], s2[kRecordGroup], mn[kRecordGroup], mx[kRecordGroup], ctr[kRecordGroup];
#pragma unroll
    for (int k = 0; k < kRecordGroup; ++k) {
      s1[k] = 0.0, s2[k] = 0.0, mn[k] = __builtin_inf(), mx[k] = -__builtin_inf();
      const int c = c0 + k < nc ? c0 + k : nc - 1;
      ctr[k] = A.centre ? A.centre[c] : 0.0;
    }
    for (int s = 0; s < steps; ++s) {
      const size_t bq = g0 + size_t(s) * gsz;
      const bool in = bq < size_t(B);
      const size_t b = in ? bq : size_t(B) - 1;  // a lane past the batch loads the last instance's row and masks it
      const T* xr = A.x + b * nx;
      const T* ur = A.u + b * nu;
      bool fin = true;  // of the whole row, before anything is added
      for (int i = 0; i < nx; ++i) fin = fin && record_finite(xr[i]);
      for (int i = 0; i < nu; ++i) fin = fin && record_finite(ur[i]);
      const bool cnt = in && fin;
#pragma unroll
      for (int k = 0; k < kRecordGroup; ++k) {
        const int c = c0 + k < nc ? c0 + k : nc - 1;  // (a component past the row repeats the last one; never stored)
        const double v = c < nx ? double(xr[c]) : double(ur[c - nx]);
        const double z = v - ctr[k];
        s1[k] += cnt ? z : 0.0;
        s2[k] += cnt ? z * z : 0.0;
        mn[k] = cnt && v < mn[k] ? v : mn[k];
        mx[k] = cnt && v > mx[k] ? v : mx[k];
      }
      if (grp == 0 && A.part_c && in) {
        const int na = A.n_ax[b], why = A.reason[b];
        if (na >= 0 && na <= A.kmax) atomicAdd(&rec_bins[na], 1);
        if (why >= 0 && why <= 4) atomicAdd(&rec_bins[A.kmax + 1 + why], 1);
        if (fin) atomicAdd(&rec_bins[A.kmax + 6], 1);
      }
    }
    if (A.part_m) {
#pragma unroll
      for (int k = 0; k < kRecordGroup; ++k) {
        const double r1 = record_wave_reduce<RecSum>(s1[k]), r2 = record_wave_reduce<RecSum>(s2[k]);
        const double rn = record_wave_reduce<RecMin>(mn[k]), rx = record_wave_reduce<RecMax>(mx[k]);
        if (lane == 0) rec_w[wave][k][0] = r1, rec_w[wave][k][1] = r2, rec_w[wave][k][2] = rn, rec_w[wave][k][3] = rx;
      }
      __syncthreads();
      if (tid < kRecordGroup * 4 && c0 + tid / 4 < nc) {  // the waves in wave order
        const int k = tid / 4, f = tid & 3;
        double r = rec_w[0][k][f];
        for (int w = 1; w < kRecordBlock / 64; ++w) {
          const double o = rec_w[w][k][f];
          r = f < 2 ? r + o : f == 2 ? RecMin::op(r, o) : RecMax::op(r, o);
        }
        A.part_m[(size_t(blockIdx.x) * nc + c0 + k) * 4 + f] = r;
      }
      __syncthreads();  // rec_w is written again by the next group
    }
  }
  if (A.part_c) {
    __syncthreads();
    for (int q = tid; q < nbins; q += kRecordBlock) A.part_c[size_t(blockIdx.x) * nbins + q] = rec_bins[q];
  }
}

// The partials of `grid` workgroups, in workgroup order -> moments [nc][4] and counts [nbins] (either may be null).
__global__ __launch_bounds__(kRecordBlock) void record_combine_kernel(const double* part_m, const int32_t* part_c, int grid, int nc,
                                                                      int nbins, double* moments, int32_t* counts) {
  const int tid = threadIdx.x;
  if (moments)
    for (int q = tid; q < nc * 4; q += kRecordBlock) {
      const int f = q & 3;
      double r = part_m[q];
      for (int w = 1; w < grid; ++w) {
        const double o = part_m[size_t(w) * nc * 4 + q];
        r = f < 2 ? r + o : f == 2 ? RecMin::op(r, o) : RecMax::op(r, o);
      }
      moments[q] = r;
    }
  if (counts)
    for (int q = tid; q < nbins; q += kRecordBlock) {
      int32_t r = 0;
      for (int w = 0; w < grid; ++w) r += part_c[size_t(w) * nbins + q];
      counts[q] = r;
    }
}

}  // namespace cgm
