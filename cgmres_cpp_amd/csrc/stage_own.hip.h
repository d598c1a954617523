// Stage ownership of the solver vectors in the row-parallel Newton kernel (tick_wg.hip.h, WgCtx::NWT = 1).
//
// The sweeps of that kernel give lane r of an instance's 16-lane row the stages 4r .. 4r+3.  In the reference's stage-major
// vector (dim_u = 3 controls per stage) these are the 12 contiguous elements 12r .. 12r+11, and the kernel's vector
// algebra holds every solver vector in the same ownership:
//     (lane r, slot i)  <->  element e = 12 r + i,   i = 3 q + j  for control j of the lane's stage q.
// One description for the kernel, the Krylov rows in HBM and the host's export.
#pragma once

namespace cgm {

struct StageOwn {
  static constexpr int SPL = 4;        // stages per lane
  static constexpr int NU = 3;         // controls per stage
  static constexpr int NV = SPL * NU;  // vector elements per lane
  static constexpr int LANES = 16;
  static constexpr int LV = LANES * NV;  // pitch of a Krylov row in HBM (pads kept zero)
  static constexpr int DV_MIN = 33, DV_MAX = 53;  // horizons the kernel is chosen for (wg_plan.hip.h: 3 dv <= 160)
  static constexpr int elem(int r, int i) { return NV * r + i; }
  static constexpr int lane_of(int e) { return e / NV; }
  static constexpr int slot_of(int e) { return e % NV; }
  // lanes that own at least one stage / at least one of the dv + 1 parameter stages
  static constexpr int lanes(int dv) { return (dv + SPL - 1) / SPL; }
  // Krylov rows are stored pair-interleaved and lane-contiguous: slot pair i/2 of all 16 lanes in one 256-byte line, a
  // lane moving two of its slots per 16-byte access
  static constexpr int hbm_pos(int r, int i) { return (i / 2) * 2 * LANES + 2 * r + (i & 1); }
  static constexpr int hbm_pos_of_elem(int e) { return hbm_pos(lane_of(e), slot_of(e)); }

  // LDS scalars per instance of the kernel's private arrays — U and F(U,x+hf,t+h) of the owned stages, the first controls
  // of U and U + h dUdt staged for the preamble's serial sweeps (pitch: stage dv is the sweeps' look-ahead word), the
  // controls of stage 0 for the plant step — which live in the storage of the three row arrays they replace
  static constexpr int stage_pitch(int dv) { return (dv + 1) | 1; }
  static constexpr int lds_scalars(int dv) { return 2 * NV * lanes(dv) + 2 * stage_pitch(dv) + NU; }
  static constexpr int lds_row_arrays(int dv) { return 3 * ((NU * dv) | 1); }

  // for every dv of the range: the slots cover [0, 3 dv) exactly once, every other slot is a pad, the HBM positions are a
  // permutation of the row, and the private arrays fit
  static constexpr bool covers(int dv) {
    const int L = NU * dv;
    int next = 0;
    for (int r = 0; r < LANES; ++r)
      for (int i = 0; i < NV; ++i) {
        const int e = elem(r, i);
        if (e != next++) return false;                                     // every element once, in order
        if (lane_of(e) != r || slot_of(e) != i) return false;              // the two directions agree
        if ((e < L) != (SPL * r + i / NU < dv)) return false;              // pads are exactly the stages beyond the horizon
        if ((e < L) && r >= lanes(dv)) return false;                       // real elements sit in the owning lanes only
      }
    return next >= L && lanes(dv) <= LANES;
  }
  static constexpr bool hbm_is_permutation() {
    bool seen[LV] = {};
    for (int e = 0; e < LV; ++e) {
      const int p = hbm_pos_of_elem(e);
      if (p < 0 || p >= LV || seen[p]) return false;
      seen[p] = true;
    }
    return true;
  }
  static constexpr bool all_dv_ok() {
    for (int dv = DV_MIN; dv <= DV_MAX; ++dv)
      if (!covers(dv) || lds_scalars(dv) > lds_row_arrays(dv)) return false;
    return true;
  }
};
static_assert(StageOwn::all_dv_ok(), "stage ownership: coverage / pads / LDS fit for dv = 33 .. 53");
static_assert(StageOwn::hbm_is_permutation(), "stage ownership: HBM row format");
static_assert(StageOwn::lds_scalars(33) == 289 && StageOwn::lds_row_arrays(33) == 297, "tightest horizon");

}  // namespace cgm
