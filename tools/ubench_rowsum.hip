// Micro-benchmark and check (dev tool): the 16-lane row sum of a double on gfx950, as four DPP steps (row16_sum of
// cgmres_cpp_amd/csrc/dpp.hip.h) and as two v_mfma_f64_4x4x4 (row16_sum_mfma below: a CANDIDATE, not in the library).
// What it found (profiles/r09_iter_chain_ab.json): the four blocks of v_mfma_f64_4x4x4 are not the four DPP rows.  Lane
// i + 4 b + 16 k holds A[i][k] of block b (B[k][j]: lane j + 4 b + 16 k) and lane j + 4 b + 16 i receives D[i][j] — the
// sum over k runs ACROSS the four 16-lane rows of the wave, never inside one, whichever operand carries the value.  No
// form of the instruction is a row sum, so the correctness half fails and the library keeps the DPP form.
//   1. layout: the lanes whose value reaches each lane of the first product, and which combination of operand roles
//      (the value as A or as B, in either product) gives the row sum
//   2. correctness of row16_sum_mfma on random, signed, denormal, +-Inf and NaN inputs (exit status 1 on a mismatch):
//      the 16 lanes of a row hold identical bits, the value is within 16 eps sum|p| of the sequential sum, a NaN or
//      Inf makes every lane of ITS row non-finite and leaves the other rows alone
//   3. timing: a dependent chain of 256 row sums (each sum, scaled by 1/16, is the next input) on one wave, in cycles
//      per link, five repetitions; the scaling alone is measured as well and is part of both figures
//   hipcc --offload-arch=gfx950 -O3 -o _diag/ubench_rowsum tools/ubench_rowsum.hip && ./_diag/ubench_rowsum
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../cgmres_cpp_amd/csrc/dpp.hip.h"

#define CHECK(x)                                                              \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      printf("%s: %s\n", #x, hipGetErrorString(e_));                          \
      return 2;                                                               \
    }                                                                         \
  } while (0)

// The candidate: with B = 1 the first product sums groups of four lanes, the second product those sums.
__device__ __forceinline__ double row16_sum_mfma(double x) {
  const double one = 1.0;
  const double t = __builtin_amdgcn_mfma_f64_4x4x4f64(x, one, 0.0, 0, 0, 0);
  return __builtin_amdgcn_mfma_f64_4x4x4f64(t, one, 0.0, 0, 0, 0);
}

// FORM 0: DPP; 1: the candidate; 2..5: the four assignments of operand roles (layout probe)
template <int FORM>
__device__ __forceinline__ double rowsum(double x) {
  const double one = 1.0;
  if constexpr (FORM == 0) return cgm::row16_sum(x);
  if constexpr (FORM == 1) return row16_sum_mfma(x);
  if constexpr (FORM == 2) return __builtin_amdgcn_mfma_f64_4x4x4f64(__builtin_amdgcn_mfma_f64_4x4x4f64(x, one, 0.0, 0, 0, 0), one, 0.0, 0, 0, 0);
  if constexpr (FORM == 3) return __builtin_amdgcn_mfma_f64_4x4x4f64(one, __builtin_amdgcn_mfma_f64_4x4x4f64(x, one, 0.0, 0, 0, 0), 0.0, 0, 0, 0);
  if constexpr (FORM == 4) return __builtin_amdgcn_mfma_f64_4x4x4f64(__builtin_amdgcn_mfma_f64_4x4x4f64(one, x, 0.0, 0, 0, 0), one, 0.0, 0, 0, 0);
  if constexpr (FORM == 5) return __builtin_amdgcn_mfma_f64_4x4x4f64(one, __builtin_amdgcn_mfma_f64_4x4x4f64(one, x, 0.0, 0, 0, 0), 0.0, 0, 0, 0);
  return x;
}

// out[t * 64 + lane] = row sum of in[t * 64 + ...]; one wave, n sets
template <int FORM>
__global__ void apply(const double* in, double* out, int n) {
  for (int t = 0; t < n; ++t) out[t * 64 + threadIdx.x] = rowsum<FORM>(in[t * 64 + threadIdx.x]);
}
// first product alone with lane s = 1 and every other lane 0, for s = 0..63: out[(form * 64 + s) * 64 + lane]
__global__ void first_product(double* out) {
  for (int s = 0; s < 64; ++s) {
    const double x = int(threadIdx.x) == s ? 1.0 : 0.0;
    out[s * 64 + threadIdx.x] = __builtin_amdgcn_mfma_f64_4x4x4f64(x, 1.0, 0.0, 0, 0, 0);
    out[(64 + s) * 64 + threadIdx.x] = __builtin_amdgcn_mfma_f64_4x4x4f64(1.0, x, 0.0, 0, 0, 0);
  }
}

constexpr int LINKS = 256;
// FORM -1: the scaling alone
template <int FORM>
__global__ void chain(double* out, long long* cyc, double x0, double scale) {
  double x = x0 + threadIdx.x * 1e-3;
  const long long t0 = __builtin_readcyclecounter();
#pragma unroll
  for (int i = 0; i < LINKS; ++i) {
    if constexpr (FORM >= 0) x = rowsum<FORM>(x);
    x *= scale;
    asm volatile("" : "+v"(x));
  }
  const long long t1 = __builtin_readcyclecounter();
  out[threadIdx.x] = x;
  if (threadIdx.x == 0) *cyc = t1 - t0;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

template <int FORM>
static int time_chain(const char* name, double* d_out, long long* d_cyc, double* per_link) {
  double v[5];
  for (int rep = -1; rep < 5; ++rep) {  // (one launch to warm the instruction cache)
    long long h;
    chain<FORM><<<1, 64>>>(d_out, d_cyc, 1.0, 1.0 / 16);
    CHECK(hipMemcpy(&h, d_cyc, 8, hipMemcpyDeviceToHost));
    if (rep >= 0) v[rep] = double(h) / LINKS;
  }
  double lo = v[0], hi = v[0];
  for (double q : v) lo = q < lo ? q : lo, hi = q > hi ? q : hi;
  printf("%-44s cycles per link: %.2f %.2f %.2f %.2f %.2f   min %.2f  spread %.2f\n", name, v[0], v[1], v[2], v[3], v[4], lo, hi - lo);
  *per_link = lo;
  per_link[1] = hi - lo;
  return 0;
}

template <int FORM>
static int probe(const char* name, const double* d_in, double* d_out, const std::vector<double>& in, const std::vector<int>& special, int n) {
  std::vector<double> out(size_t(n) * 64);
  apply<FORM><<<1, 64>>>(d_in, d_out, n);
  CHECK(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
  int good = 0, all = 0;
  for (int t = 0; t < n; ++t)
    for (int row = 0; row < 4; ++row) {
      if (special[t * 4 + row]) continue;
      ++all;
      double s = 0, sa = 0;
      for (int l = 0; l < 16; ++l) s += in[t * 64 + row * 16 + l], sa += std::fabs(in[t * 64 + row * 16 + l]);
      bool ok = true;
      for (int l = 0; l < 16; ++l) ok = ok && std::fabs(out[t * 64 + row * 16 + l] - s) <= 16 * 2.220446049250313e-16 * sa;
      good += ok;
    }
  printf("layout probe: %-44s %d of %d rows are the row sum\n", name, good, all);
  return 0;
}

int main() {
  constexpr int N = 4096;  // sets of 64 lanes
  std::vector<double> in(size_t(N) * 64), out(size_t(N) * 64);
  std::vector<int> special(size_t(N) * 4, 0);  // rows with an Inf or NaN among the inputs
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::uniform_int_distribution<int> ex(-300, 300), lane(0, 15), kind(0, 9);
  const double denorm = 4.9406564584124654e-324;
  for (int t = 0; t < N; ++t)
    for (int row = 0; row < 4; ++row) {
      const int k = kind(rng);  // 0-3: same scale, 4-5: wide exponents, 6: denormals, 7: denormals + normals, 8: Inf, 9: NaN
      const double sc = std::ldexp(1.0, ex(rng));
      for (int l = 0; l < 16; ++l) {
        double v = u(rng);
        if (k <= 3) v *= sc;
        else if (k <= 5) v = std::ldexp(v, ex(rng));
        else if (k == 6) v = denorm * double(int(v * 1000));
        else if (k == 7) v = (l & 1) ? denorm * double(int(v * 1000)) : v * 1e-300;
        in[t * 64 + row * 16 + l] = v;
      }
      if (k == 8) {
        in[t * 64 + row * 16 + lane(rng)] = (t & 1) ? INFINITY : -INFINITY;
        if (t & 2) in[t * 64 + row * 16 + lane(rng)] = -INFINITY;  // (possibly Inf - Inf)
        special[t * 4 + row] = 1;
      }
      if (k == 9) in[t * 64 + row * 16 + lane(rng)] = NAN, special[t * 4 + row] = 1;
    }
  double *d_in, *d_out;
  long long* d_cyc;
  CHECK(hipMalloc(&d_in, in.size() * 8));
  CHECK(hipMalloc(&d_out, out.size() * 8));
  CHECK(hipMalloc(&d_cyc, 8));
  CHECK(hipMemcpy(d_in, in.data(), in.size() * 8, hipMemcpyHostToDevice));

  // ---- 1. layout
  {
    std::vector<double> lo(2 * 64 * 64);
    first_product<<<1, 64>>>(d_out);
    CHECK(hipMemcpy(lo.data(), d_out, lo.size() * 8, hipMemcpyDeviceToHost));
    for (int form = 0; form < 2; ++form) {
      printf("first product, value as %s, the other operand 1: lanes of the wave summed into lane l\n", form ? "B" : "A");
      for (int l = 0; l < 64; ++l) {
        printf("  lane %2d <-", l);
        for (int src = 0; src < 64; ++src)
          if (lo[size_t(form * 64 + src) * 64 + l] != 0.0) printf(" %d", src);
        printf("\n");
      }
    }
    if (probe<2>("value as A, then A", d_in, d_out, in, special, 64)) return 2;
    if (probe<3>("value as A, then B", d_in, d_out, in, special, 64)) return 2;
    if (probe<4>("value as B, then A", d_in, d_out, in, special, 64)) return 2;
    if (probe<5>("value as B, then B", d_in, d_out, in, special, 64)) return 2;
  }

  // ---- 2. correctness of the candidate
  int bad_bits = 0, bad_value = 0, bad_special = 0, rows = 0, rows_special = 0;
  double worst = 0;
  apply<1><<<1, 64>>>(d_in, d_out, N);
  CHECK(hipMemcpy(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost));
  for (int t = 0; t < N; ++t)
    for (int row = 0; row < 4; ++row) {
      const double* p = &in[t * 64 + row * 16];
      const double* o = &out[t * 64 + row * 16];
      if (special[t * 4 + row]) {
        ++rows_special;
        for (int l = 0; l < 16; ++l) bad_special += std::isfinite(o[l]) ? 1 : 0;
        continue;
      }
      ++rows;
      double s = 0, sa = 0;
      for (int l = 0; l < 16; ++l) s += p[l], sa += std::fabs(p[l]);
      bool same = true, close = true, finite = true;
      for (int l = 0; l < 16; ++l) {
        same = same && same_bits(o[l], o[0]);
        finite = finite && std::isfinite(o[l]);
        const double err = std::fabs(o[l] - s), bound = 16 * 2.220446049250313e-16 * sa;
        close = close && err <= bound;
        if (bound > 0 && err / bound > worst) worst = err / bound;
      }
      bad_bits += !same, bad_value += !close, bad_special += !finite;
    }
  printf("row16_sum_mfma: %d finite rows, %d rows with Inf/NaN; lanes not bit-identical in %d rows, outside 16 eps sum|p| in %d rows "
         "(worst error / bound %.3f), wrong finiteness in %d lanes/rows\n", rows, rows_special, bad_bits, bad_value, worst, bad_special);
  const bool ok = bad_bits == 0 && bad_value == 0 && bad_special == 0;
  printf("correctness: %s\n", ok ? "PASS" : "FAIL");

  // ---- 3. timing
  double base[2], dpp[2], mfma[2];
  if (time_chain<-1>("scaling alone (v_mul_f64)", d_out, d_cyc, base)) return 2;
  if (time_chain<0>("row16_sum (DPP) + scaling", d_out, d_cyc, dpp)) return 2;
  if (time_chain<1>("row16_sum_mfma + scaling", d_out, d_cyc, mfma)) return 2;
  printf("{\"links\": %d, \"scaling_alone\": %.2f, \"row16_sum\": %.2f, \"row16_sum_spread\": %.2f, \"row16_sum_mfma\": %.2f, "
         "\"row16_sum_mfma_spread\": %.2f, \"correct\": %s}\n", LINKS, base[0], dpp[0], dpp[1], mfma[0], mfma[1], ok ? "true" : "false");
  CHECK(hipFree(d_in));
  CHECK(hipFree(d_out));
  CHECK(hipFree(d_cyc));
  return ok ? 0 : 1;
}
