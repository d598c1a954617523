// Diagnostic builds of the wg and wave tick kernels: the -DCGM_DEBUG_LDS flag word and the -DCGM_STAMPS phase clocks
// (tools/phase_stamps.py).  Both compile to nothing in the product build; cgm_vmcnt_imm serves both builds.
#pragma once
#include <hip/hip_runtime.h>

namespace cgm {

// s_waitcnt that leaves the `vm` youngest vector-memory operations in flight (gfx9 encoding: vmcnt in bits 3:0 and 15:14,
// the other counters untouched)
constexpr int cgm_vmcnt_imm(int vm) { return 0x0F70 | (vm & 15) | ((vm >> 4) << 14); }

#ifdef CGM_DEBUG_LDS
// Diagnostic build only: set by the costate sweep when one of its LDS addresses falls outside the workgroup's allocation
// (0x10000 | what << 12 | thread); read back through cgmres_hip_plugin_debug_lds_oob (user_model.hip.h)
__device__ int g_cgm_lds_oob;
#endif
// Diagnostic build only: accumulate shader-clock deltas per phase (thread 0 of block 0).  Compiles to nothing
// in the product build.
#ifdef CGM_STAMPS
// Diagnostic build only (tools/phase_stamps.py): per-phase shader-clock totals of block 0 in a device-global buffer
// (kept out of WgParams on purpose: any use of the kernel-argument struct through a pointer made hipcc spill the whole
// struct to scratch and distorted the very thing being measured).
__device__ long long g_cgm_stamps[64];
// The per-phase totals are accumulated in LDS (static, outside the dynamic carve-up) and added to the global buffer
// once at the end of the kernel: a global atomic per stamp queues behind the basis-row loads in flight and made the
// stamps after them look ~1.5 k cycles long.
__device__ __forceinline__ long long* cgm_stamp_lds() {
  __shared__ long long acc[66];  // [0..31] cycles, [32..63] visits, [64] last stamp (ids 28, 29: see cgm_stamp_flush)
  return acc;
}
__device__ __forceinline__ void cgm_stamp(int id) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    long long* acc = cgm_stamp_lds();
    const long long now = (long long)__builtin_amdgcn_s_memtime();
    if (id >= 0) {
      acc[id] += now - acc[64];
      acc[32 + id] += 1;
    } else {
      for (int i = 0; i < 64; ++i) acc[i] = 0;
      g_cgm_stamps[30] = (long long)__builtin_amdgcn_s_memrealtime();
      g_cgm_stamps[31] = now;
    }
    acc[64] = now;
  }
}
__device__ __forceinline__ void cgm_stamp_flush() {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    long long* acc = cgm_stamp_lds();
    for (int i = 0; i < 28; ++i) g_cgm_stamps[i] += acc[i], g_cgm_stamps[32 + i] += acc[32 + i];
    g_cgm_stamps[28] += (long long)__builtin_amdgcn_s_memrealtime() - g_cgm_stamps[30];
    g_cgm_stamps[29] += (long long)__builtin_amdgcn_s_memtime() - g_cgm_stamps[31];
    // ids 28 and 29 (the split of the Gram-Schmidt rounds): the buffer keeps its 64 words, their cycles go to the unused
    // words 60, 61 and their visits to 62, 63
    for (int i = 0; i < 2; ++i) g_cgm_stamps[60 + i] += acc[28 + i], g_cgm_stamps[62 + i] += acc[60 + i];
  }
}
#define CGM_STAMP(ctx, id) cgm_stamp(id)
// the same behind the LDS operations in flight: what the stamp closes is a fetch, whose cost is the round trip and not the issue
#define CGM_STAMP_LDS(ctx, id) (__extension__({ asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); cgm_stamp(id); }))
#else
#define CGM_STAMP(ctx, id) ((void)0)
#define CGM_STAMP_LDS(ctx, id) ((void)0)
#endif

#ifdef CGM_AMAX
// Diagnostic build only (tools/rot_increments.py): the angle increments the row-Newton sweep hands to its rotation, per
// wave and Newton iteration — words 0-7 for iteration 0 (the change of x0 under U + h v), 8-15 for the later ones (the
// Newton correction): [0] the largest increment (bits of a non-negative double order as integers), [1] wave visits,
// [2..6] visits with an increment above 2^-18, 2^-14, 2^-10, 2^-8, 2^-6.
__device__ unsigned long long g_cgm_amax[16];
__device__ __forceinline__ void cgm_amax_record(bool run, double amax, int it) {
  unsigned long long* w = g_cgm_amax + (it == 0 ? 0 : 8);
  const bool on = run && amax == amax;
  const unsigned long long bits = (unsigned long long)__double_as_longlong(amax);
  if (on && bits > w[0]) atomicMax(w, bits);
  const bool a18 = __any(on && amax > 0x1p-18), a14 = __any(on && amax > 0x1p-14), a10 = __any(on && amax > 0x1p-10),
             a8 = __any(on && amax > 0x1p-8), a6 = __any(on && amax > 0x1p-6), any = __any(on);
  if ((threadIdx.x & 63) == 0 && any) {
    atomicAdd(w + 1, 1ull);
    if (a18) atomicAdd(w + 2, 1ull);
    if (a14) atomicAdd(w + 3, 1ull);
    if (a10) atomicAdd(w + 4, 1ull);
    if (a8) atomicAdd(w + 5, 1ull);
    if (a6) atomicAdd(w + 6, 1ull);
  }
}
#endif

}  // namespace cgm
