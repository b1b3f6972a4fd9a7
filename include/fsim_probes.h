/* fsim_probes.h -- signed-distance proximity probes of libfsim.so, computed on the device (a C-ABI of its own beside fsim.h,
 * fsim_camera.h, fsim_points.h, fsim_voxels.h, fsim_normals.h, fsim_flow.h and fsim_rays.h).
 *
 * A probe sensor is a frame fixed in the world or mounted on a model body, with a set of probe POINTS given in that frame, a largest
 * distance dmax in metres and a set of colliding geoms it does not see (the body it is mounted on, as a rule).  Per point it answers the
 * clearance query a ray cannot: how far the point is from the nearest surface in ANY direction, which surface that is, and which way to
 * move to get away from it -- MuJoCo's mj_geomDistance / distance sensors, a planner's signed-distance query, the local SDF volume around
 * a gripper.  Inside a solid the distance is negative: the penetration depth.  The probes see exactly the collision geometry the cameras
 * of fsim_camera.h and the rays of fsim_rays.h see; they need neither and disturb neither.
 *
 * Probe.  A probe is at the world point p = o + R_s * pt: o, R_s the sensor frame's world pose of this very call (the pose launch of
 * fsim_camera.h with the sensors' own mount table; the Cursor agent's cursor offset is added for a sensor on a cursor body, exactly as
 * for a camera or a ray sensor), pt its point of the table.
 *
 * Distance, per colliding geom that is not excluded, with q = R_geom^T (p - c_geom) the probe in the geom frame:
 *   plane     d = q.z; gradient +z.
 *   sphere    (radius r) d = |q| - r; gradient q / |q|.
 *   capsule   (radius r, half-length h) v = q - (0, 0, clamp(q.z, -h, h)); d = |v| - r; gradient v / |v|.
 *   cylinder  (r, h) dr = hypot(q.x, q.y) - r, dz = |q.z| - h.  Outside (dr > 0 or dz > 0): d = hypot(max(dr, 0), max(dz, 0)), gradient
 *             (max(dr, 0) * radial + max(dz, 0) * sign(q.z) z) / d, radial = (q.x, q.y, 0) / hypot(q.x, q.y).  Inside (both <= 0):
 *             d = max(dr, dz); gradient radial when dr >= dz (the side wins a tie), else sign(q.z) z.
 *   box       (half sizes s) a = |q| - s per axis.  Outside (some a_k > 0): d = |max(a, 0)|, gradient sign(q) * max(a, 0) / d.  Inside
 *             (all a_k <= 0): d = max_k a_k, gradient sign(q_k) e_k of the maximum; the smallest axis wins a tie.
 *   hull      (face planes n_i . x <= c_i, the planes fsim_set_probes is given) the PLANE BOUND d = max_i (n_i . q - c_i), gradient n of
 *             the maximising plane; the smallest plane index wins a tie.  This is exact inside the hull and wherever the nearest feature
 *             is a face.  It is a lower bound near edges and vertices outside.  (Only the three mesh furniture have hulls.)
 * sign(x) is -1 for x < 0 and +1 otherwise.  The ties are settled the way the normal of fsim_normals.h settles them.  Degenerate points:
 * where the vector to normalise is shorter than 1e-12 (a sphere's centre, a capsule's axis between its end points, a cylinder's axis for
 * the radial direction) the unit vector is the geom's local +x.
 * The gradient goes to the world frame with R_geom.  Over geoms the smallest signed distance wins; a strict < in colliding-geom order
 * settles ties.  The winner is accepted when its distance is <= dmax; otherwise dist = dmax, geom = -1, grad = (0, 0, 0) (MuJoCo's
 * distmax convention).  Where the result is exact, the nearest surface point is p - dist * grad.
 *
 * Outputs, per env and probe (probes in the order of the point table):
 *   dist   the signed distance in metres, negative inside a solid; dmax when nothing is within dmax.
 *   geom   the MODEL geom id of the nearest surface, in the numbering of the segmentation image of fsim_camera.h and of the geom output
 *          of fsim_rays.h; -1 when nothing is within dmax.
 *   grad   the world-frame unit gradient of the distance at p (it points away from the surface, inside and outside).
 *
 * No side effects: fsim_probe_distance writes no state, RNG draw, look-ahead shadow or counter.  An env's output depends only on its own
 * record and the probe set, never on the batch around it.  Without probes set, nothing is allocated or launched.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_PROBES_H
#define FSIM_PROBES_H
#include "fsim.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FSIM_PROBE_MAX_SENSORS 16
#define FSIM_PROBE_MAX_PROBES 4096 /* per env, over all sensors */

typedef struct fsim_probe_sensor {
  int32_t body;                  /* model body the sensor is mounted on (before reduction), -1: the world */
  float pos[3], quat[4];         /* sensor frame in that body's frame, quaternion wxyz (normalised by the library) */
  float dmax;                    /* metres: 0 < dmax < inf */
  int32_t first_probe, n_probes; /* its slice of the point table; slices are contiguous, in sensor order, and cover it */
  uint32_t exclude[3];           /* bit k: colliding geom k (the order of the model's cg_orig table) is invisible to this sensor */
} fsim_probe_sensor_t;

/* Replace the handle's probe set: n_sensors = 1 .. FSIM_PROBE_MAX_SENSORS sensors over n_probes = 1 .. FSIM_PROBE_MAX_PROBES points
 * (pts[n_probes][3], sensor frame, metres).  n_sensors == 0 clears the probe set and frees its tables (the other arguments are ignored).
 * hull_planes / hull_adr / hull_num: the face planes of the convex-hull colliders, exactly as fsim_set_cameras takes them (may be NULL
 * when the model has no mesh collider); the probe set keeps its own copy.  Host pointers, copied before return; the call waits for the
 * handle's stream before it replaces the tables.  FSIM_EINVAL, each with a message: more than 16 sensors, no or more than 4096 probes, a
 * sensor without a probe, slices that are not contiguous or do not cover the table, a body unknown to the model, a pose that is not
 * finite, a dmax that is not 0 < dmax < inf, an exclude bit at or beyond the number of colliding geoms, a non-finite point, more than 96
 * colliding geoms or 1024 hull planes (the caps of fsim_camera.h), a mesh collider without planes.
 * A refused call leaves the previous set in place. */
int fsim_set_probes(fsim_t *, int n_sensors, const fsim_probe_sensor_t *sensors, int n_probes, const float *pts, int n_planes,
                    const float *hull_planes, const int32_t *hull_adr, const int32_t *hull_num);

/* The signed distance of every probe of every env: dist_dev float32 [n_envs][n_probes], geom_dev int32 [n_envs][n_probes], grad_dev
 * float32 [n_envs][n_probes][3] (any may be NULL, not all).  Works in the state fsim_sync leaves, settled exactly as fsim_cast_rays
 * settles it (a step in flight is waited for and the overflow re-step ladder runs first); then two launches are enqueued on the handle's
 * stream (poses, distances) and the call returns without waiting for them.  Reads the env records and writes nothing but the outputs
 * and a pose scratch the probe set owns.  FSIM_EINVAL: null handle, no probes set, all three pointers NULL. */
int fsim_probe_distance(fsim_t *, float *dist_dev, int32_t *geom_dev, float *grad_dev);

#ifdef __cplusplus
}
#endif
#endif
