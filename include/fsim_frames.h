/* fsim_frames.h -- body and site frame sensors of libfsim.so with their Jacobians, computed on the device (a C-ABI of its own beside fsim.h,
 * fsim_camera.h, fsim_points.h, fsim_voxels.h, fsim_normals.h, fsim_flow.h, fsim_rays.h, fsim_probes.h and fsim_pairs.h).
 *
 * A frame sensor reports a frame F, optionally relative to a reference frame G: MuJoCo's framepos / framequat / framelinvel / frameangvel
 * sensors with their reftype / refid reference frame, and mj_jacBody / mj_jacSite -- the pose of a leg's connector site in the frame of
 * the table top's connector site and its rate, the grip site's Jacobian for an operational-space controller.  The sensors read the env
 * record; they need no cameras, rays, probes or pairs and disturb none of them.
 *
 * Frame.  A frame is (body, pos, quat): body is a model body id before reduction, -1 means the world; pos and quat are an offset in that
 * body's frame, quaternion wxyz, normalised by the library in double.  A site is its body plus site_pos / site_quat composed with the offset
 * by the caller.  The library folds the body into its reduced body with body_relpos / body_relquat in double at set time, as
 * fsim_set_cameras does for mounts.
 *
 * Contract.  Quantities per env: (p, R, q) is the world pose of F; (v, w) is the world-frame linear velocity of the material point at p
 * and the angular velocity of F's body.  The same quantities with index g describe G.  A world reference has p_g = 0, R_g = I,
 * v_g = w_g = 0.  r = p - p_g.
 *   pos      = R_g^T r.
 *   quat     = qnormalized(conj(q_g) (x) q), wxyz, not sign-canonicalised.
 *   vel[0:3] = R_g^T (v - v_g - w_g x r).  This is the exact time derivative of pos.
 *   vel[3:6] = R_g^T (w - w_g).  It satisfies d quat / dt = 1/2 (0, vel[3:6]) (x) quat.
 *   jac      is [6][nv], linear rows first, such that vel = jac @ qvel in real arithmetic.  With jp, jr the world Jacobians of the point
 *            and of the rotation:
 *              linear rows  = R_g^T (jp - jp_g + [r]x jr_g)
 *              angular rows = R_g^T (jr - jr_g)
 * Body twists follow fsim_flow.h's rule exactly: a hinge turns about its anchor, a slide moves along its axis, a free joint has
 * v(x_b) = qvel[0:3] and its angular qvel[3:6] in the body's own frame; reduced body 0 has twist 0.
 * The Jacobian column of dof d is that dof's unit twist about the world origin, taken at p:
 *   hinge (anchor x a, a); slide (a, 0); free translation (e_i, 0); free rotation (x_b x R_b e_i, R_b e_i).
 * The column is zero unless the dof's reduced body is an ancestor-or-self of the frame's.  (The device evaluates vel and jac from the
 * DIFFERENCE of the two bodies' twists about the world origin, taken at p -- the same quantity in real arithmetic, and exactly zero for
 * a dof that moves F and G alike.)
 * A frame on a Cursor body follows the env's cursor position exactly as a camera on a cursor body does.  It has no velocity and no
 * Jacobian columns, because the offset is a teleport.
 *
 * Outputs, per env and sensor (S sensors, nv dofs):
 *   pos   float32 [n_envs][S][3]       metres, in G's frame.
 *   quat  float32 [n_envs][S][4]       wxyz, F's orientation in G's frame.
 *   vel   float32 [n_envs][S][6]       linear (m/s), then angular (rad/s), in G's frame.
 *   jac   float32 [n_envs][S][6][nv]   linear rows, then angular rows.
 *
 * No side effects: fsim_frame_state writes no state, RNG draw, look-ahead shadow or counter.  An env's output depends only on its own
 * record and the frame set, never on the batch around it; a sensor's output does not depend on the other sensors of the set.  Without a
 * frame set, nothing is allocated or launched.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_FRAMES_H
#define FSIM_FRAMES_H
#include "fsim.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FSIM_FRAME_MAX_SENSORS 64
#define FSIM_FRAME_MAX_NV 128 /* dofs of the model */

typedef struct fsim_frame {
  int32_t body; /* model body id, -1 = the world */
  float pos[3], quat[4]; /* offset in the body's frame, wxyz */
} fsim_frame_t;

typedef struct fsim_frame_sensor {
  fsim_frame_t frame, ref; /* ref.body == -1 with identity offset: the world */
} fsim_frame_sensor_t;

/* Replace the handle's frame set: n_sensors = 1 .. FSIM_FRAME_MAX_SENSORS sensors.  n_sensors == 0 clears the set and frees its tables (the
 * other argument is ignored).  Host pointer, copied before return; the call waits for the handle's stream before it replaces the tables.
 * FSIM_EINVAL, each with a message: a null handle or null argument, more than 64 sensors, a body unknown to the model, a non-finite pose
 * or a zero quaternion, a model with more than 32 reduced bodies, nv above 128.  A refused set leaves the previous set in place. */
int fsim_set_frames(fsim_t *, int n_sensors, const fsim_frame_sensor_t *sensors);

/* The state of every sensor of every env: pos_dev float32 [n_envs][S][3], quat_dev float32 [n_envs][S][4], vel_dev float32 [n_envs][S][6],
 * jac_dev float32 [n_envs][S][6][nv] (any may be NULL, not all; what is not asked for is not computed).  Works in the state fsim_sync leaves,
 * settled exactly as fsim_pair_distance settles it (a step in flight is waited for and the overflow re-step ladder runs first); then one
 * launch is enqueued on the handle's stream and the call returns without waiting for it.  Reads the env records and writes nothing but the
 * outputs.  FSIM_EINVAL: null handle, no frame set, all four pointers NULL. */
int fsim_frame_state(fsim_t *, float *pos_dev, float *quat_dev, float *vel_dev, float *jac_dev);

#ifdef __cplusplus
}
#endif
#endif
