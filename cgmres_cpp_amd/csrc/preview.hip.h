// The preview of a sampled reference signal (cgmres_hip_closed_loop_device_preview, cgmres_hip_preview_device): forms the
// parameter horizon of every tick of a launch on the device,
//     ptau_k = [ p(t_k), p(t_k + dtau_k), ..., p(t_k + dv * dtau_k) ]          (cgmres.hpp:37, dtau_k = get_dtau(t_k), :32-34)
// from a signal sampled on a uniform grid, sig [batch or 1][n_samples][dim_p] in the handle's dtype, sample j at time
// t0 + j * ts.  For tick k, stage i and component c, in DOUBLE for fp32 handles too (an fp32 t / ts near 1e4 has no
// fraction bits left):
//     tau = double(t_k) + i * double(dtau_k)
//     s   = clamp((tau - t0) / ts, 0, n_samples - 1)
//     hold:    j = min(floor(s), n_samples - 1);           p = sig[j][c]
//     linear:  j = min(floor(s), max(n_samples - 2, 0));   w = s - j;   p = sig[j][c] + w * (sig[j+1][c] - sig[j][c])
//                                                          (n_samples == 1: p = sig[0][c])
//     row[k][b][i * dim_p + c] = T(p)
// Before t0 the first sample holds, past the end the last.  (t_k, dtau_k) are the handle's own values in T, computed on
// the host by the statements that advance its clock (ctx_common.hip.h: dtau_of) and passed as kernel arguments like
// WgParams::dtau_tab.
//
// A kernel of its own, launched in FRONT of the tick launch on the handle's stream like the record and plant kernels
// behind it: no tick kernel, parameter struct or kernel argument knows about it; the tick kernels reload ptau from
// WgParams::ptau_seq at the top of every tick and are pointed at the rows written here.  Independent of the model, so it
// lives in the library (inst_preview.hip) and a plugin holds none of it.
//
// A plain streaming kernel without atomics or LDS: blockIdx.y is the tick, the lanes of blockIdx.x run along the
// (stage, component) elements of an instance and on into the next instance, so a wavefront writes 64 consecutive
// elements of the tick's [batch][(dv+1) * dim_p] row and reads the few neighbouring samples its stages fall on together
// (one stage moves dtau / ts samples: the loads of a wavefront share cache lines).  A lane past the row returns before its
// first load.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/cgmres_hip.h"

namespace cgm {

constexpr int kPreviewBlock = 256;

template <class T>
struct PreviewArgs {
  unsigned row_elems;  // batch * (dv+1) * dim_p: the elements of one tick's row
  int W, np;           // (dv+1) * dim_p, dim_p
  int n_samples, linear;
  size_t sig_inst;  // n_samples * dim_p per instance, 0 for one broadcast signal
  double t0, ts;
  const T* sig;
  T* rows;                                    // [n][batch][W]
  T tab[2 * CGMRES_HIP_TICKS_PER_LAUNCH];     // (t_k, dtau_k) of tick k = blockIdx.y
};

template <class T>
__global__ __launch_bounds__(kPreviewBlock) void preview_kernel(PreviewArgs<T> A) {
  const unsigned q = blockIdx.x * unsigned(kPreviewBlock) + threadIdx.x;  // b * W + i * np + c
  if (q >= A.row_elems) return;
  const unsigned k = blockIdx.y;
  const unsigned b = q / unsigned(A.W), e = q - b * unsigned(A.W);
  const unsigned i = e / unsigned(A.np), c = e - i * unsigned(A.np);
  const double tau = double(A.tab[2 * k]) + double(i) * double(A.tab[2 * k + 1]);
  const double last = double(A.n_samples - 1);
  const double s = fmin(fmax((tau - A.t0) / A.ts, 0.0), last);
  const T* sg = A.sig + size_t(b) * A.sig_inst + c;
  double p;
  if (A.linear && A.n_samples > 1) {
    const double jf = fmin(floor(s), last - 1.0);
    const size_t j = size_t(jf);
    const double lo = double(sg[j * A.np]), hi = double(sg[(j + 1) * A.np]);
    p = lo + (s - jf) * (hi - lo);
  } else {
    p = double(sg[size_t(floor(s)) * A.np]);  // (s <= n_samples - 1: the clamp is the min of the hold rule)
  }
  A.rows[size_t(k) * A.row_elems + q] = T(p);
}

}  // namespace cgm
