// The record kernels (record.hip.h) for both scalar types and the one host function that launches them.  A translation
// unit of its own, like inst_horizon.hip: the code objects of the tick kernels (the other inst_*.hip) hold nothing of it.
#include "record.hip.h"

#include "ctx_common.hip.h"
#include "factory.hip.h"

namespace cgm {

static_assert(kRecordBlock == CGMRES_HIP_RECORD_BLOCK, "include/cgmres_hip.h states the record kernel's workgroup");

template <class T>
static int record_take_t(cgmres_hip_ctx* c, const void* x, const void* u, const int32_t* n_ax, const int32_t* reason,
                         const RecordOut& o) {
  const int B = c->cfg.batch, nc = c->nx + c->nu, nbins = c->cfg.k_max + 7;
  const bool want_m = o.moments != nullptr, want_c = o.counts != nullptr;
  if (!want_m && !want_c && !o.x_log && !o.u_log && !o.n_ax_log && !o.reason_log) return 0;  // (t_host alone: host work)
  if (want_c && nbins > kRecordMaxBins)
    return fail(CGMRES_HIP_EINVAL, "record: counts of k_max = %d need %d bins, the kernel's LDS histogram holds %d", c->cfg.k_max,
                nbins, kRecordMaxBins);
  int grid = (B + kRecordBlock - 1) / kRecordBlock;
  if (grid > kRecordMaxGrid) grid = kRecordMaxGrid;
  RecordArgs<T> A{};
  A.B = B, A.nx = c->nx, A.nu = c->nu, A.kmax = c->cfg.k_max;
  A.x = static_cast<const T*>(x), A.u = static_cast<const T*>(u), A.n_ax = n_ax, A.reason = reason;
  A.x_log = static_cast<T*>(o.x_log), A.u_log = static_cast<T*>(o.u_log), A.n_ax_log = o.n_ax_log, A.reason_log = o.reason_log;
  A.centre = o.centre;
  if (want_m || want_c) {  // one scratch serves every record of the handle: they follow each other on the stream
    const size_t n_m = size_t(grid) * nc * 4, n_c = (size_t(grid) * nbins + 1) / 2;  // (the integers behind the doubles)
    if (int rc = c->grow(&c->rec_scratch, &c->rec_scratch_n, n_m + n_c)) return rc;
    A.part_m = want_m ? c->rec_scratch : nullptr;
    A.part_c = want_c ? reinterpret_cast<int32_t*>(c->rec_scratch + n_m) : nullptr;
  }
  record_kernel<T><<<dim3(grid), kRecordBlock, want_c ? size_t(nbins) * sizeof(int32_t) : 0, c->stream>>>(A);
  HIP_TRY(hipGetLastError());
  if (want_m || want_c) {
    record_combine_kernel<<<1, kRecordBlock, 0, c->stream>>>(A.part_m, A.part_c, grid, nc, nbins, o.moments, o.counts);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int record_take(cgmres_hip_ctx* c, const void* x, const void* u, const int32_t* n_ax, const int32_t* reason, const RecordOut& o) {
  return c->cfg.dtype == CGMRES_HIP_F32 ? record_take_t<float>(c, x, u, n_ax, reason, o)
                                         : record_take_t<double>(c, x, u, n_ax, reason, o);
}

}  // namespace cgm
