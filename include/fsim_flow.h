/* fsim_flow.h -- optical-flow and surface-velocity images of libfsim.so, computed on the device from the cameras of fsim_camera.h (a
 * C-ABI of its own beside fsim.h, fsim_camera.h, fsim_points.h, fsim_voxels.h and fsim_normals.h).
 *
 * The ray pass of fsim_render hits analytic surfaces of rigid geoms, so the motion of a pixel is a closed form of its hit point, of the
 * twist of the body it lies on and of the twist of the camera's body: no frame differencing, nothing wrong at a silhouette.
 *
 * Notation for one pixel (i, j) = (column, row) of a camera: (p_c, R_c) the camera pose (R_c: camera -> world) the pose launch of this
 * very call wrote, s its slope tan(fovy / 2) / (height / 2), cx = (i + 0.5 - width / 2) s, cy = (height / 2 - (j + 0.5)) s, d its depth
 * and g its segmentation.
 *
 * Surface point.  q = the pixel's world point, bit-identical to the dense map's point of fsim_render_points for that pixel (the same
 * device function computes both).
 *
 * Twists.  A body's twist comes from qpos and qvel of the env record: the state fsim_sync leaves, qvel belonging to that qpos.  With
 * (x_b, R_b) the world pose of a reduced body, each joint contributes
 *   hinge  w = (R_b axis) qvel  about the anchor x_b + R_b jpos
 *   slide  v = (R_b axis) qvel  (R_b: the body's world rotation, which a slide joint does not turn)
 *   free   v(x_b) = qvel[0:3],  w = R_b qvel[3:6]  (the angular velocity of a free joint is held in the body's own frame)
 * and the twists sum up the reduced tree.  Reduced body 0 (the world) has twist exactly 0.  The Cursor agent's cursor offset is a teleport
 * between steps and contributes no velocity.
 *
 * velocity (camera_velocity): u = v_g + w_g x (q - pos_g), with (v_g, w_g) the world twist of the body of geom g taken at that geom's
 *   origin pos_g of the pose launch.  m/s, world frame; it does not depend on the camera's motion.
 *
 * flow (camera_flow): the camera-frame rate of the material point is X' = R_c^T (u - v_c - w_c x (q - p_c)), with (v_c, w_c) the twist
 *   of the camera's body taken at p_c (zero for a world camera).  With d' = -X'_z:
 *     flow[0] = (X'_x - cx d') / (d s)     columns per second, positive to the right
 *     flow[1] = -(X'_y - cy d') / (d s)    rows per second, positive downward
 *     flow[2] = d'                         m/s
 *   d >= znear > 0, so nothing divides by zero.
 *
 * seg == -1 gives (0, 0, 0) in both outputs.  All rates are per second of simulated time.
 *
 * No side effects: fsim_render_flow writes no state, RNG draw, look-ahead shadow or counter.  An env's output depends only on its own
 * record and the camera set, never on the batch around it.  There are no settings, so there is no fsim_set_* call.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_FLOW_H
#define FSIM_FLOW_H
#include "fsim_camera.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Renders the cameras once and derives the flow and / or velocity image, in one call, for one state: the state fsim_sync leaves,
 * settled exactly as fsim_render settles it (fsim_render's two launches, then the twist launch and the flow pass; the call returns
 * without waiting for them).  depth_dev / seg_dev: the camera images, as fsim_render writes them (either may be NULL: the handle's
 * scratch is used).  flow_dev and velocity_dev: float32 [n_envs][n_cam][height][width][3] each (either may be NULL).  The twist scratch
 * and a small id table are allocated by the first call and freed by fsim_destroy (and by fsim_set_cameras, which changes their size).
 * FSIM_EINVAL: null handle, no cameras set, both outputs NULL. */
int fsim_render_flow(fsim_t *, float *depth_dev, int32_t *seg_dev, float *flow_dev, float *velocity_dev);

#ifdef __cplusplus
}
#endif
#endif
