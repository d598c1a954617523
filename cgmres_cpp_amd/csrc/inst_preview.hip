// The preview kernel (preview.hip.h) for both scalar types and the one host function that launches it.  A translation
// unit of its own, like inst_record.hip: the code objects of the tick kernels (the other inst_*.hip) hold nothing of it.
#include "preview.hip.h"

#include "ctx_common.hip.h"
#include "factory.hip.h"

namespace cgm {

template <class T>
static int preview_fill_t(cgmres_hip_ctx* c, const PreviewCall& call) {
  const PreviewSig& s = *call.s;
  const size_t W = size_t(c->np) * (c->cfg.dv + 1), row = size_t(c->cfg.batch) * W;
  if (call.n <= 0 || row == 0) return 0;
  if (call.n > CGMRES_HIP_TICKS_PER_LAUNCH)
    return fail(CGMRES_HIP_EINVAL, "preview: %d ticks in one launch, the kernel's table holds %d", call.n, CGMRES_HIP_TICKS_PER_LAUNCH);
  if (row > 0xffffff00u)  // (the kernel indexes a tick's row with 32 bits)
    return fail(CGMRES_HIP_EINVAL, "preview: batch * dim_p * (dv+1) = %zu exceeds the kernel's 32-bit row index", row);
  PreviewArgs<T> A{};
  A.row_elems = unsigned(row), A.W = int(W), A.np = c->np;
  A.n_samples = s.n_samples, A.linear = s.interp == CGMRES_HIP_PREVIEW_LINEAR;
  A.sig_inst = s.per_instance ? size_t(s.n_samples) * c->np : 0;
  A.t0 = s.t0, A.ts = s.ts;
  A.sig = static_cast<const T*>(s.sig), A.rows = static_cast<T*>(call.rows);
  const T* tab = static_cast<const T*>(call.tab);
  for (int k = 0; k < 2 * call.n; ++k) A.tab[k] = tab[k];
  const dim3 grid(unsigned((row + kPreviewBlock - 1) / kPreviewBlock), unsigned(call.n));
  preview_kernel<T><<<grid, kPreviewBlock, 0, c->stream>>>(A);
  HIP_TRY(hipGetLastError());
  return 0;
}

int preview_fill(cgmres_hip_ctx* c, const PreviewCall& call) {
  return c->cfg.dtype == CGMRES_HIP_F32 ? preview_fill_t<float>(c, call) : preview_fill_t<double>(c, call);
}

// cgmres_hip_preview_device: the rows of the n_ticks ticks from the handle's time on, launch-sized pieces of the clock
template <class T>
static int preview_export_t(cgmres_hip_ctx* c, const PreviewSig& s, int n_ticks, void* rows) {
  const size_t row = size_t(c->cfg.batch) * c->np * (c->cfg.dv + 1);
  T t = T(c->time());  // (time() widens the handle's T: exact both ways)
  for (int i = 0; i < n_ticks; i += CGMRES_HIP_TICKS_PER_LAUNCH) {
    const int n = n_ticks - i < CGMRES_HIP_TICKS_PER_LAUNCH ? n_ticks - i : CGMRES_HIP_TICKS_PER_LAUNCH;
    T tab[2 * CGMRES_HIP_TICKS_PER_LAUNCH];
    tick_clock<T>(c->cfg, t, n, tab);
    t = tab[2 * (n - 1)] + T(c->cfg.dt);
    PreviewCall call;
    call.s = &s, call.rows = static_cast<T*>(rows) + size_t(i) * row, call.n = n, call.tab = tab;
    if (int rc = preview_fill_t<T>(c, call)) return rc;
  }
  return 0;
}

int preview_export(cgmres_hip_ctx* c, const PreviewSig& s, int n_ticks, void* rows) {
  return c->cfg.dtype == CGMRES_HIP_F32 ? preview_export_t<float>(c, s, n_ticks, rows) : preview_export_t<double>(c, s, n_ticks, rows);
}

}  // namespace cgm
