/* fsim_wrench.h -- force-torque, accelerometer and joint-load sensors of libfsim.so, computed on the device (a C-ABI of its own beside
 * fsim.h, fsim_camera.h, fsim_points.h, fsim_voxels.h, fsim_normals.h, fsim_flow.h, fsim_rays.h, fsim_probes.h, fsim_pairs.h,
 * fsim_frames.h, fsim_dynamics.h and fsim_contacts.h).
 *
 * MuJoCo's sim.forward() followed by mj_rnePostConstraint (cacc, cfrc_ext, cfrc_int) with the force, torque and accelerometer sensors on
 * top, plus data.qacc and data.qfrc_constraint, for every env: the wrench an arm feels through its wrist -- contacts plus the held
 * part's weight and inertia plus the weld of a connected part --, the accelerations, and how hard welds and joint limits hold.  The
 * quantities are a pure function of the env record, evaluated at the record's state after the same forward pass as fsim_contact_forces
 * (collision, constraint assembly, the Newton solve, on a copy of the record that is never stored back).  The Newton problem is strictly
 * convex, so they depend on the record's qacc_warmstart only within the solver tolerance.
 *
 * Sensors.  A set holds 1 .. FSIM_WRENCH_MAX_SENSORS sensors.  A sensor is a frame: a model body id with an offset pose (pos, quat wxyz)
 * in that body's frame, resolved exactly as fsim_frames.h resolves a frame (a site is its body plus the site's pose).  The body must be a
 * body of the compiled model that moves.  A body without a joint of its own (the hand behind Sawyer's last link) has been folded into its
 * moving ancestor when the model was compiled: the cut is then at that ancestor's joint.  A frame fixed in the world is refused.
 *
 * Outputs, per env and sensor (S sensors):
 *   force    float32 [n_envs][S][3]  the force that the parent side exerts on the sensor body's subtree through the body's joint, in the
 *                                    sensor frame, newtons.
 *   torque   float32 [n_envs][S][3]  the same wrench's torque about the sensor origin, in the sensor frame.
 *   accel    float32 [n_envs][S][3]  the proper acceleration of the material point at the sensor origin, in the sensor frame: with p the
 *                                    origin, d2p/dt2 - g, so a sensor at rest reads +9.81 along world z (MuJoCo's accelerometer).
 *   angacc   float32 [n_envs][S][3]  the angular acceleration of the body, in the sensor frame.
 *   external float32 [n_envs][S][6]  cfrc_ext: the net force, then the torque about the sensor origin, both in the WORLD frame, exerted on
 *                                    the sensor's body alone by the listed contacts, the active welds and xfrc_applied.
 * force and torque are the sum over the subtree's bodies of I a + v x* I v - f_ext with gravity inside a (cfrc_int of
 * mj_rnePostConstraint): actuator, passive, applied and joint-limit forces on that joint are part of what is measured, along the joint
 * axis.  "Subtree" means the bodies below the cut, "body alone" the compiled body with every body folded into it.  Through a free joint
 * nothing but qfrc_passive + qfrc_applied of its six dofs passes, and the library reads force and torque of such a body off those
 * (the subtree sum is the same quantity with the solve's rounding of qacc in it): exact zeros for a part at qvel = 0 with no applied
 * joint force; its external carries the content.
 * per env:
 *   qacc            float32 [n_envs][nv]  the accelerations of the forward pass.
 *   qfrc_constraint float32 [n_envs][nv]  the generalised force of contacts, welds and joint limits: M qacc - qfrc_smooth.
 *   status          int32   [n_envs]      bits 0 and 1 exactly as fsim_contact_out_t::status.
 * The sums run in a fixed order and in float32: external over the contact list in list order (+ the force on geom 2's body, - on geom
 * 1's), then the welds in model order, then xfrc_applied; force and torque over the subtree's bodies in ascending body order.
 *
 * Out of scope: a cut at a folded (jointless) body; the -DFSIM_MFMA_HESSIAN build; handles with more than FSIM_WRENCH_MAX_SLOTS contact
 * slots; models with more than 32 bodies after folding (one body per lane, subtrees as 32-bit masks: the limit of fsim_frames.h and
 * fsim_dynamics.h; every furniture shipped fits); gyro and velocimeter (fsim_frame_state's vel gives those).  The mixed batch, the VecEnv wrapper and the multi-GPU gather do not
 * carry these outputs.
 *
 * No side effects: fsim_wrenches writes no state, warm start, RNG draw, look-ahead shadow or counter.  An env's output depends only on
 * its own record and the set, never on the batch around it; a sensor's bits do not depend on the other sensors of the set; an output's
 * bits do not depend on which other outputs are asked for; every output word is written exactly once, zeros explicitly.  Without a set,
 * nothing is allocated or launched.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_WRENCH_H
#define FSIM_WRENCH_H
#include "fsim.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FSIM_WRENCH_MAX_SENSORS 64
#define FSIM_WRENCH_MAX_SLOTS 64 /* contact slots of the handle (fsim_max_contacts) the pass serves */

typedef struct fsim_wrench_sensor_t {
  int32_t body;  /* model body id; it (or the body it is folded into) must move */
  float pos[3];  /* the sensor origin in the body's frame */
  float quat[4]; /* the sensor orientation in the body's frame, wxyz, normalised by the library */
} fsim_wrench_sensor_t;

/* Replace the handle's sensor set: n_sensors = 1 .. FSIM_WRENCH_MAX_SENSORS.  n_sensors == 0 clears the set and frees its table (the
 * other argument is ignored).  Host pointer, copied before return; the call settles the handle and waits for its stream before it
 * replaces the table.  FSIM_EINVAL, each with a message: a null handle or null table, too many sensors, a handle with more than
 * FSIM_WRENCH_MAX_SLOTS contact slots, a model with more than 32 bodies after folding, a body id out of range, a body that does not move, a pose that is not finite, a zero quaternion.
 * A refused call leaves the previous set in place. */
int fsim_set_wrenches(fsim_t *, int n_sensors, const fsim_wrench_sensor_t *sensors);

typedef struct fsim_wrench_out_t { /* device pointers; any may be NULL, not all; what is not asked for is not stored */
  float *force;           /* [n_envs][S][3] */
  float *torque;          /* [n_envs][S][3] */
  float *accel;           /* [n_envs][S][3] */
  float *angacc;          /* [n_envs][S][3] */
  float *external;        /* [n_envs][S][6] */
  float *qacc;            /* [n_envs][nv] */
  float *qfrc_constraint; /* [n_envs][nv] */
  int32_t *status;        /* [n_envs] */
} fsim_wrench_out_t;

/* The wrenches of every env.  Works in the state fsim_sync leaves, settled exactly as fsim_contact_forces settles it; then one launch is
 * enqueued on the handle's stream and the call returns without waiting for it.  Reads the env records and writes nothing but the outputs.
 * FSIM_EINVAL: null handle or argument, no set, every pointer NULL, the -DFSIM_MFMA_HESSIAN build. */
int fsim_wrenches(fsim_t *, const fsim_wrench_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
