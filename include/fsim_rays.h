/* fsim_rays.h -- ray-cast range sensors and lidar of libfsim.so, computed on the device (a C-ABI of its own beside fsim.h,
 * fsim_camera.h, fsim_points.h, fsim_voxels.h, fsim_normals.h and fsim_flow.h).
 *
 * A ray sensor is a frame fixed in the world or mounted on a model body, with a set of ray directions given in that frame, a range
 * [tmin, tmax] in metres along the ray and a set of colliding geoms it does not see (the body it is mounted on, as a rule).  It answers
 * the distance-along-a-ray query MuJoCo users know as the rangefinder sensor or mj_ray: a proximity sensor between the fingers, a few
 * whiskers on the wrist, a 360 degree lidar on the table.  The sensors see exactly the collision geometry the cameras of fsim_camera.h
 * see; they need no camera and do not disturb one.
 *
 * Rays.  The library normalises each direction in double; a zero or non-finite direction is FSIM_EINVAL.  A ray is o + t d in world
 * metres: o the sensor origin, d the rotated unit direction, both from the sensor frame's world pose of this very call (the pose launch
 * of fsim_camera.h with the sensors' own mount table; the Cursor agent's cursor offset is added for a sensor on a cursor body, exactly as
 * for a camera).
 *
 * Hit.  As in fsim_camera.h with t in place of depth: per colliding geom that is not excluded, take the interval [t0, t1] of the ray
 * inside the solid (planes are infinite and their only surface point is the crossing, t0 = t1); t = t0 >= tmin ? t0 : t1; the hit is
 * accepted when tmin <= t <= tmax.  Over geoms the smallest t wins; a strict < in colliding-geom order settles ties.
 *
 * Outputs, per env and ray (rays in the order of the direction table):
 *   dist    t, or -1 when nothing is hit (MuJoCo's rangefinder convention).  The hit point in the sensor frame is dist * dir.
 *   geom    the MODEL geom id of the surface, in the numbering of the segmentation image of fsim_camera.h; a miss gives -1.
 *   normal  the world-frame outward unit normal of that geom at the hit point, with the definition of fsim_normals.h: R_geom * the
 *           geom's local outward normal, not flipped towards the sensor; a miss gives (0, 0, 0).
 *
 * No side effects: fsim_cast_rays writes no state, RNG draw, look-ahead shadow or counter.  An env's output depends only on its own
 * record and the ray set, never on the batch around it.  Without rays set, nothing is allocated or launched.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_RAYS_H
#define FSIM_RAYS_H
#include "fsim.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FSIM_RAY_MAX_SENSORS 16
#define FSIM_RAY_MAX_RAYS 4096 /* per env, over all sensors */

typedef struct fsim_ray_sensor {
  int32_t body;              /* model body the sensor is mounted on (before reduction), -1: the world */
  float pos[3], quat[4];     /* sensor frame in that body's frame, quaternion wxyz (normalised by the library) */
  float tmin, tmax;          /* metres along the ray: 0 <= tmin < tmax, tmax finite */
  int32_t first_ray, n_rays; /* its slice of the direction table; slices are contiguous, in sensor order, and cover it */
  uint32_t exclude[3];       /* bit k: colliding geom k (the order of the model's cg_orig table) is invisible to this sensor */
} fsim_ray_sensor_t;

/* Replace the handle's ray set: n_sensors = 1 .. FSIM_RAY_MAX_SENSORS sensors over n_rays = 1 .. FSIM_RAY_MAX_RAYS directions
 * (dirs[n_rays][3], sensor frame, any nonzero length).  n_sensors == 0 clears the ray set and frees its tables (the other arguments are
 * ignored).  hull_planes / hull_adr / hull_num: the face planes of the convex-hull colliders, exactly as fsim_set_cameras takes them
 * (may be NULL when the model has no mesh collider); the ray set keeps its own copy.  Host pointers, copied before return; the call
 * waits for the handle's stream before it replaces the tables.  FSIM_EINVAL, each with a message: more than 16 sensors, no or more than
 * 4096 rays, a sensor without a ray, slices that are not contiguous or do not cover the table, a body unknown to the model, a pose that is
 * not finite, a range that is not 0 <= tmin < tmax < inf, an exclude bit at or beyond the number of colliding geoms, a zero or
 * non-finite direction, more than 96 colliding geoms or 1024 hull planes (the caps of fsim_camera.h), a mesh collider without planes.
 * A refused call leaves the previous set in place. */
int fsim_set_rays(fsim_t *, int n_sensors, const fsim_ray_sensor_t *sensors, int n_rays, const float *dirs, int n_planes,
                  const float *hull_planes, const int32_t *hull_adr, const int32_t *hull_num);

/* Cast every ray of every env: dist_dev float32 [n_envs][n_rays], geom_dev int32 [n_envs][n_rays], normal_dev float32
 * [n_envs][n_rays][3] (any may be NULL, not all).  Casts in the state fsim_sync leaves, settled exactly as fsim_render settles it (a step
 * in flight is waited for and the overflow re-step ladder runs first); then two launches are enqueued on the handle's stream (poses,
 * rays) and the call returns without waiting for them.  Reads the env records and writes nothing but the outputs and a pose scratch the
 * ray set owns.  FSIM_EINVAL: null handle, no rays set, all three pointers NULL. */
int fsim_cast_rays(fsim_t *, float *dist_dev, int32_t *geom_dev, float *normal_dev);

#ifdef __cplusplus
}
#endif
#endif
