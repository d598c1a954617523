// Which form of a caller's operator the stand-alone Gmres runs and on which mapping (user_operator.hip.h):
// gmres_plan() decides it from (len, k_max, form) alone.  Pure arithmetic, __host__ __device__, no HIP call:
// gmres_op_solve launches by it, cgmres_hip_operator_plan reports it (without a GPU), so there is one decision.
#pragma once
#include <cstddef>

namespace cgm {

constexpr size_t kGmresWaveLdsLimit = 150 * 1024;

// LDS of one system on the one-wave-per-system solver (gmres_wave_kernel), in doubles:
//   vin [len]  operand row of the warm-start product     vout [len]  result row of a SERIAL operator (no such row
//   V [k_max + 1][len]  Krylov basis                                  in the row form: the product stays in registers)
//   compact Hessenberg, residual vector, reflectors
struct GmresWaveLds {
  static __host__ __device__ int pitch_H(int kmax) { return ((kmax * (kmax + 1)) / 2 + 2) & ~1; }
  static __host__ __device__ int op_rows(bool row_form) { return row_form ? 1 : 2; }  // vin (+ vout)
  static __host__ __device__ size_t count(int L, int kmax, bool row_form = false) {
    return size_t(kmax + 1 + op_rows(row_form)) * L + pitch_H(kmax) + (kmax + 2) + 3 * kmax + 2;
  }
};

struct GmresPlan {
  int form;     // 0: serial Op::Ax, 1: Op::Ax_row
  int mapping;  // 0: one lane per system (gmres_op_kernel), 1: one wavefront per system (gmres_wave_kernel)
  size_t lds_bytes;  // dynamic LDS of the wave kernel (also when it is not taken)
};

inline __host__ __device__ GmresPlan gmres_plan(int L, int kmax, bool row_form) {
  const size_t lds = GmresWaveLds::count(L, kmax, row_form) * sizeof(double);
  return {row_form ? 1 : 0, lds <= kGmresWaveLdsLimit ? 1 : 0, lds};
}

// the sizes a solve accepts at all: the reference indexes v_mat with 16 bits (gmres.hpp:29, matrix.hpp:10)
inline __host__ __device__ bool gmres_sizes_ok(int L, int kmax) { return L >= 1 && kmax >= 1 && long(L) * (long(kmax) + 1) < 65536; }

}  // namespace cgm
