/* fsim_momentum.h -- centre-of-mass, momentum and energy sensors of libfsim.so, computed on the device (a C-ABI of its own beside
 * fsim.h, fsim_camera.h, fsim_points.h, fsim_voxels.h, fsim_normals.h, fsim_flow.h, fsim_rays.h, fsim_probes.h, fsim_pairs.h,
 * fsim_frames.h, fsim_dynamics.h, fsim_contacts.h and fsim_wrench.h).
 *
 * MuJoCo's subtreecom, subtreelinvel, subtreeangmom, mj_jacSubtreeCom and data.energy (mj_energyPos / mj_energyVel) for every env, of
 * sets of bodies rather than of subtrees alone: where the centre of mass of the held leg, of the arm with its load or of the
 * half-assembled table is, how fast it moves, the angular momentum of those bodies, and the energy of the env.  Connected furniture
 * parts are joined by weld constraints, not by the tree, so "the table so far" is a list of parts.  The quantities are a pure function of
 * qpos and qvel of the env record, evaluated at the record's state.
 *
 * Sensors.  A set holds 1 .. FSIM_MOM_MAX_SENSORS sensors.  A sensor is a set of model bodies, given as model body ids, each optionally
 * with its kinematic subtree (the body and every model body below it).  A listed body is resolved to its body of the compiled model: a
 * body without a joint of its own (the hand behind Sawyer's last link) has been folded into its moving ancestor when the model was
 * compiled, and stands for that compiled body with everything folded into it.  A body fixed in the world is refused.  A body listed
 * twice, or covered twice through a subtree, counts once.
 *
 * Outputs, per env and sensor (S sensors):
 *   com     float32 [n_envs][S][3]      the centre of mass of the set, world frame, metres.
 *   linvel  float32 [n_envs][S][3]      the velocity of that centre of mass (subtreelinvel); the set's linear momentum is this times the
 *                                       set's mass, a constant of the model that the caller sums from its own tables.
 *   angmom  float32 [n_envs][S][3]      the angular momentum of the set about its own centre of mass, world frame (subtreeangmom):
 *                                       sum_b R I_b R^T w_b + m_b (x_b - c) x (v_b - v_c).
 *   jac     float32 [n_envs][S][3][nv]  mj_jacSubtreeCom of the set: linvel = jac qvel; an exact zero in the column of every dof that
 *                                       moves none of the set's bodies.
 * per env:
 *   energy  float32 [n_envs][2]         the potential energy -sum_b m_b g . x_b, then the kinetic energy 1/2 qvel^T M qvel with the
 *                                       armature in it (data.energy).  The models have no joint springs, so gravity is the whole
 *                                       potential.  The sum runs over the bodies of the compiled model that move: bodies fixed in the
 *                                       world add a constant to MuJoCo's potential that this output leaves out.
 * The sums run in a fixed order and in float32: over a set's bodies in ascending compiled-body order, positions relative to the inertial
 * origin of the set's lowest-numbered body (a part 8 m from the origin keeps the precision of a part at the origin); angmom from
 * (x_b - c) and (v_b - v_c), never as a difference of two moments about the origin; a body's own I_b w_b in the body frame, then turned.
 *
 * Out of scope: the composite inertia tensor of a set; per-sensor energies; models with more than 32 bodies after folding (one body per
 * lane, sets as 32-bit masks: the limit of fsim_frames.h, fsim_dynamics.h and fsim_wrench.h; every furniture shipped fits) or more
 * than 128 dofs (FSIM_DYN_MAX_NV of fsim_dynamics.h).  The mixed batch, the VecEnv wrapper and the multi-GPU gather do not carry these
 * outputs.
 *
 * No side effects: fsim_momenta writes no state, warm start, RNG draw, look-ahead shadow or counter.  An env's output depends only on
 * its own record and the set, never on the batch around it; a sensor's bits do not depend on the other sensors of the set; an output's
 * bits do not depend on which other outputs are asked for; every output word is written exactly once, zeros explicitly.  Without a set,
 * nothing is allocated or launched.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_MOMENTUM_H
#define FSIM_MOMENTUM_H
#include "fsim.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FSIM_MOM_MAX_SENSORS 64

/* Replace the handle's sensor set: n_sensors = 1 .. FSIM_MOM_MAX_SENSORS.  Sensor i lists bodies[adr[i]] .. bodies[adr[i + 1] - 1]
 * (adr[0] == 0, adr non-decreasing, at least one body per sensor); subtree[k] != 0 adds the kinematic subtree of bodies[k].
 * n_sensors == 0 clears the set and frees its table (the other arguments are ignored).  Host pointers, copied before return; the call
 * settles the handle and waits for its stream before it replaces the table.  FSIM_EINVAL, each with a message: a null handle or null
 * table, too many sensors, a model with more than 32 bodies after folding or more than 128 dofs, a bad adr table, a body id out of
 * range, a body that does not move, a set whose resolved bodies have zero total mass.  A refused call leaves the previous set in place. */
int fsim_set_momenta(fsim_t *, int n_sensors, const int32_t *adr /* [n_sensors + 1] */, const int32_t *bodies /* model body ids */,
                     const int32_t *subtree /* per listed body, 0 / 1 */);

typedef struct fsim_momentum_out_t { /* device pointers; any may be NULL, not all; what is not asked for is not stored */
  float *com;    /* [n_envs][S][3] */
  float *linvel; /* [n_envs][S][3] */
  float *angmom; /* [n_envs][S][3] */
  float *jac;    /* [n_envs][S][3][nv] */
  float *energy; /* [n_envs][2] */
} fsim_momentum_out_t;

/* The momenta of every env.  Works in the state fsim_sync leaves, settled exactly as fsim_dynamics settles it; then one launch is
 * enqueued on the handle's stream and the call returns without waiting for it.  Reads qpos and qvel of the env records and writes
 * nothing but the outputs.  FSIM_EINVAL: null handle or argument, no set, every pointer NULL. */
int fsim_momenta(fsim_t *, const fsim_momentum_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
