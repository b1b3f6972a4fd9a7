/* fsim_contacts.h -- contact-force and touch sensors of libfsim.so, computed on the device (a C-ABI of its own beside fsim.h,
 * fsim_camera.h, fsim_points.h, fsim_voxels.h, fsim_normals.h, fsim_flow.h, fsim_rays.h, fsim_probes.h, fsim_pairs.h, fsim_frames.h and
 * fsim_dynamics.h).
 *
 * MuJoCo's sim.forward() followed by reading the contact forces (mj_contactForce, the touch sensor), for every env: how hard the
 * gripper presses on a part, how hard a leg sits in its hole.  The quantities are a pure function of the env record, evaluated at the
 * record's state: qpos, qvel, ctrl, qfrc_applied, xfrc_applied, the weld state and the collision masks go in -- the pass of
 * fsim_physics_forward (collision, constraint assembly, the Newton solve), on a copy of the record that is never stored back.  The
 * Newton problem is strictly convex, so the forces do not depend on the record's qacc_warmstart beyond the solver tolerance
 * (fsim_config_t::solver_tolerance / solver_iterations); they are the forces the NEXT step's first substep would start from, not an
 * average over the step's substeps.
 *
 * Sensors.  A set holds 1 .. FSIM_CON_MAX_SENSORS sensors.  A sensor is two sets of colliding geoms, A and B, given as model geom ids
 * (the numbering of fsim_state_ptrs_t::contact_geoms and of camera_segmentation); nb == 0 means "every colliding geom that is not in
 * A".  A contact belongs to the sensor when one of its geoms is in A and the other in B.
 *
 * Outputs, per env and sensor (S sensors):
 *   force   float32 [n_envs][S][3]  the net world-frame force that B exerts on A, newtons: the sum over the sensor's contacts, in the
 *                                   order of the contact list.
 *   touch   float32 [n_envs][S]     the sum of the normal force magnitudes of the sensor's contacts (MuJoCo's touch), never negative.
 *   count   int32   [n_envs][S]     the listed contacts of the sensor.  Listed means within the pair's margin, whether or not the force
 *                                   is nonzero: MuJoCo's ncon.
 * per env:
 *   status  int32   [n_envs]        bit 0: the pass dropped contacts because there were more than the handle's contact slots
 *                                   (fsim_max_contacts), so the forces are those of the truncated problem; bit 1: the instability guard
 *                                   fired or a Newton step could not be factored (the forces are not to be trusted).
 * and, when asked for, the contact list itself, C = fsim_max_contacts() rows per env in the order of fsim_physics_forward's
 * contact_geoms:
 *   con_geoms   int32   [n_envs][C][2]  model geom ids (geom 1, geom 2); -1 in the rows behind the list.
 *   con_pos     float32 [n_envs][C][3]  contact point, world frame.
 *   con_normal  float32 [n_envs][C][3]  unit normal, pointing from geom 1 to geom 2.
 *   con_dist    float32 [n_envs][C]     signed distance, negative = penetration.  For a contact that is an active constraint the
 *                                       value is recovered from the constraint's reference acceleration (the solver's record no
 *                                       longer holds it): it agrees with the collision pass's to about 1e-8 m.
 *   con_force   float32 [n_envs][C][3]  world-frame force on geom 2's body; geom 1's body takes the opposite.
 *   con_fn      float32 [n_envs][C]     its normal component, never negative.
 * Rows behind the list are exact zeros.  force of a sensor is the sum, in list order and in float32, of +con_force over its contacts
 * whose geom 2 is in A and -con_force over those whose geom 1 is in A; touch is the sum of con_fn in the same order.  Swapping A and B
 * negates force and leaves touch and count.
 *
 * Out of scope: the forces of welds (connected parts hold each other through a weld, not through contacts) and of joint limits are
 * part of the same solve but are not reported.  The mixed batch, the VecEnv wrapper and the multi-GPU gather do not carry these outputs.
 *
 * No side effects: fsim_contact_forces writes no state, warm start, RNG draw, look-ahead shadow or counter.  An env's output depends
 * only on its own record and the set, never on the batch around it; a sensor's bits do not depend on the other sensors of the set; an
 * output's bits do not depend on which other outputs are asked for.  Without a set, nothing is allocated or launched.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_CONTACTS_H
#define FSIM_CONTACTS_H
#include "fsim.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FSIM_CON_MAX_SENSORS 64
#define FSIM_CON_MAX_SLOTS 64 /* contact slots of the handle (fsim_max_contacts) the pass serves */

typedef struct fsim_contact_sensor_t {
  const int32_t *a; /* [na] model geom ids of side A, each a colliding geom, distinct */
  const int32_t *b; /* [nb] model geom ids of side B; nb == 0 (b ignored): every colliding geom not in A */
  int32_t na, nb;
} fsim_contact_sensor_t;

/* Replace the handle's sensor set: n_sensors = 1 .. FSIM_CON_MAX_SENSORS.  n_sensors == 0 clears the set and frees its table (the other
 * argument is ignored).  Host pointers, copied before return; the call settles the handle and waits for its stream before it replaces the
 * table.  FSIM_EINVAL, each with a message: a null handle or null table, too many sensors, a handle with more than FSIM_CON_MAX_SLOTS
 * contact slots, a geom id out of range, a geom that does not collide, a geom listed twice on a side, an empty A, A and B overlapping.
 * A refused call leaves the previous set in place. */
int fsim_set_contacts(fsim_t *, int n_sensors, const fsim_contact_sensor_t *sensors);

typedef struct fsim_contact_out_t { /* device pointers; any may be NULL, not all; what is not asked for is not computed */
  float *force;      /* [n_envs][S][3] */
  float *touch;      /* [n_envs][S] */
  int32_t *count;    /* [n_envs][S] */
  int32_t *status;   /* [n_envs] */
  int32_t *con_geoms; /* [n_envs][C][2] */
  float *con_pos;    /* [n_envs][C][3] */
  float *con_normal; /* [n_envs][C][3] */
  float *con_dist;   /* [n_envs][C] */
  float *con_force;  /* [n_envs][C][3] */
  float *con_fn;     /* [n_envs][C] */
} fsim_contact_out_t;

/* The contact forces of every env.  Works in the state fsim_sync leaves, settled exactly as fsim_physics_forward settles it (a step in
 * flight is waited for and the overflow re-step ladder runs first); then one launch is enqueued on the handle's stream and the call
 * returns without waiting for it.  Reads the env records and writes nothing but the outputs.  FSIM_EINVAL: null handle or argument, no
 * set, every pointer NULL. */
int fsim_contact_forces(fsim_t *, const fsim_contact_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
