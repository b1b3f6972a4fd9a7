/* fsim_clearance.h -- what-if clearance queries of libfsim.so, computed on the device (a C-ABI of its own beside fsim.h and fsim_pairs.h,
 * whose pair sensors it evaluates).
 *
 * fsim_pair_distance (fsim_pairs.h) answers for the state an env is in.  fsim_clearance answers the same question for states the robot
 * might move to: for every env, K candidate configurations of a list of hinge / slide joints -- an arm's seven joints, a whole tree, both
 * arms of a Baxter -- and per candidate the distance, geoms, witness points and normal of every pair sensor of the clearance set.  One call
 * for all envs and candidates; the env records are read and never written.
 *
 * Contract per (env e, candidate k): the outputs are what fsim_pair_distance would give for env e with the clearance set's sensors if the
 * record's qpos at the listed dofs held candidate k.  Nothing else of the record enters differently: the other joints, every part and the
 * Cursor words are the record's.  Joint ranges are NOT applied: a candidate beyond a limit is evaluated where it says.  The per-pair and
 * per-sensor contract (cores, radii, portal depth, A-major order, strict <, dmax) is that of fsim_pairs.h.
 *
 * valid.  A candidate with a value that is not finite gets valid = 0, and its row is evaluated with the env's own value in place of each
 * such value (the other columns keep the candidate's).  Otherwise valid = 1.
 *
 * Carry.  A rule names a furniture part (a model body that moves by a free joint) and a carrier body (any model body, a gripper as a
 * rule).  Where bit r of the env's mask byte is set, the part of rule r keeps its present pose relative to the carrier:
 *     X_part' = X_carrier(candidate) o X_carrier(record)^-1 o X_part(record),
 * composed in fp32 on the device, and every colliding geom folded into the part's reduced body moves with it.  Parts connected to it by
 * welds are bodies of their own and need rules of their own.  X_carrier(candidate) is the carrier's pose by the candidate's kinematics: a
 * carrier that is itself a carried part is taken where the record has it (rules do not chain).  With the bit clear the part stays where
 * the record has it, and the row is bit for bit what it is without the rule.
 *
 * Outputs, per env, candidate and sensor (S sensors), laid out as fsim_pair_distance's with the candidate dimension behind the env's:
 *   dist    float32 [n_envs][K][S]       geoms  int32 [n_envs][K][S][2]
 *   fromto  float32 [n_envs][K][S][6]    normal float32 [n_envs][K][S][3]
 *   valid   uint8   [n_envs][K]
 *
 * No side effects: fsim_clearance writes no state, RNG draw, look-ahead shadow or counter -- nothing but its outputs and a pose scratch the
 * clearance set owns.  An output row depends only on its env's record, its own candidate, its env's mask byte and the set: not on K, on
 * the other candidates, on the other envs or on how the rows were split over launches.  A clearance set and a pair set (fsim_set_pairs)
 * coexist and know nothing of each other.  Without a clearance set, nothing is allocated or launched.
 *
 * Launches.  The scratch holds scratch_rows pose rows.  A call is split over envs into chunks of floor(scratch_rows / K) envs; each chunk
 * is two launches on the handle's stream, in stream order: k_clr_pose (one wave per row: kinematics at the candidate, carried parts, geom
 * poses) and k_pair_dist (the distance kernel of fsim_pair_distance, a row standing for an env).
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_CLEARANCE_H
#define FSIM_CLEARANCE_H
#include "fsim_pairs.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FSIM_CLR_MAX_DOFS 32
#define FSIM_CLR_MAX_CANDIDATES 1024 /* per env and call */
#define FSIM_CLR_MAX_CARRY 8

typedef struct fsim_clr_carry {
  int32_t part_body, carrier_body; /* model body ids */
} fsim_clr_carry_t;

/* Replace the handle's clearance set.  dofs: n_dofs = 1 .. FSIM_CLR_MAX_DOFS distinct dof indices of hinge or slide joints, in the order
 * of a candidate's columns.  sensors: n_sensors pair sensors exactly as fsim_set_pairs takes them (the same validation, caps and pair
 * order).  carry: n_carry = 0 .. FSIM_CLR_MAX_CARRY rules (NULL when 0), each a distinct furniture part and a carrier body outside it.
 * max_candidates = 1 .. FSIM_CLR_MAX_CANDIDATES: the largest K of a call.  scratch_rows: pose rows of the scratch, at least
 * max_candidates, at most n_envs * max_candidates (more is cut to that); 0 = min(n_envs * max_candidates, 32768).  n_sensors == 0 clears
 * the set and frees its tables (the other arguments are ignored).  Host pointers, copied before return; the call waits for the handle's
 * stream before it replaces the tables.  FSIM_EINVAL, each with a message: what fsim_set_pairs refuses; an empty dof list (a model
 * without hinge or slide joints -- the Cursor agent -- has nothing to list); more than 32 dofs, a dof out of range, listed twice or of a
 * free joint; a carry rule whose part is not a furniture part, is named by two rules, whose carrier is unknown or belongs to the part;
 * max_candidates or scratch_rows out of range.  A refused call leaves the previous set in place. */
int fsim_set_clearance(fsim_t *, int n_dofs, const int32_t *dofs, int n_sensors, const fsim_pair_sensor_t *sensors, int n_carry,
                       const fsim_clr_carry_t *carry, int max_candidates, int scratch_rows);

/* The clearance of every candidate of every env.  cand_dev float32 [n_envs][K][n_dofs]; carry_mask_dev uint8 [n_envs], bit r = rule r
 * (NULL: nothing is carried; bits at or beyond the number of rules are ignored); the outputs as above (any may be NULL, but not all four
 * of dist, geoms, fromto and normal).  Works in the state fsim_sync leaves, settled exactly as fsim_pair_distance settles it; then the
 * launches are enqueued on the handle's stream and the call returns without waiting for them.  FSIM_EINVAL: null handle, no clearance
 * set, K < 1, K > max_candidates, cand_dev NULL, the four pair outputs all NULL. */
int fsim_clearance(fsim_t *, int K, const float *cand_dev, const uint8_t *carry_mask_dev, float *dist_dev, int32_t *geoms_dev,
                   float *fromto_dev, float *normal_dev, uint8_t *valid_dev);

#ifdef __cplusplus
}
#endif
#endif
