// The rotation of the row-Newton sweep's trig pairs (wg_sweep_rows.hip.h: newton_rot_step), sized for the increments
// the sweep really hands it (profiles/r09_iter_chain_ab.json has their distribution):
//   sin d = d + d^3 (S[0] + z (S[1] + ...)),    cos d - 1 = z (C[0] + z (C[1] + ...)),    z = d^2,    |d| <= 2^LOG2_R,
// Taylor coefficients, as few as keep the truncation of either below 2e-17 on that range; a larger increment takes the
// fresh sin / cos pair.  The quad sweep and the wave mapping keep MathCtx::rot_sin / rot_cos and rot_zmax.
// tests/test_rotation_range.py reads the three lines below and checks that bound in exact rational arithmetic: keep
// them in this form (an integer; a brace list of quotients of integers).
#pragma once

#define CGM_NEWTON_ROT_LOG2_R (-13)
#define CGM_NEWTON_ROT_SIN {-1.0 / 6.0}
#define CGM_NEWTON_ROT_COS {-1.0 / 2.0}
