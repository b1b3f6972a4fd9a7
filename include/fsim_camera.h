/* fsim_camera.h -- batched depth / segmentation cameras of libfsim.so (a C-ABI of its own beside fsim.h).
 *
 * The cameras see exactly the collision geometry the solver uses: planes (infinite, as they collide), spheres, capsules,
 * cylinders, boxes and the convex hulls of the mesh colliders.  The textured visual meshes of the reference are not part of
 * the compiled model, so there is no RGB image; this is the project's own observation, not a copy of the reference's renders.
 *
 * Camera model (MuJoCo's convention): a pinhole camera that looks along its own -z with +y up; fovy is the vertical field of
 * view in degrees; pixel (i, j) -- column i, row j, row 0 the top of the image -- is sampled through its centre (i + 0.5, j + 0.5).
 * Depth is the distance along the optical axis in metres (MuJoCo's linearised depth), of the nearest surface point the pixel's
 * ray meets with znear <= depth <= zfar; a pixel with none gets zfar and segmentation -1.  Segmentation is the MODEL geom id of
 * that surface (the numbering of the contact_geoms field of fsim_get_state).  An env's images depend on that env's state and the
 * camera set alone, never on the batch around it.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP
 * addresses; work is enqueued on the handle's stream.
 */
#ifndef FSIM_CAMERA_H
#define FSIM_CAMERA_H
#include "fsim.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FSIM_CAM_MAX = 8,          /* cameras per handle */
  FSIM_CAM_MAX_SIZE = 512,   /* width and height, each */
  FSIM_CAM_MAX_GEOMS = 96,   /* colliding geoms of the model (the catalogue's largest: 83, Baxter + toy_table) */
  FSIM_CAM_MAX_PLANES = 1024 /* face planes of all convex-hull colliders of the model together (coplanar facets merged; chair_agne_0010: 459) */
};

typedef struct fsim_camera {
  int32_t body;          /* -1: fixed in the world; else a model body id (before reduction): the camera moves with that body */
  float pos[3], quat[4]; /* pose in the body (or world) frame, quaternion wxyz (normalised by the library) */
  float fovy_deg;        /* vertical field of view, in (0, 180) */
  float znear, zfar;     /* 0 < znear < zfar, metres along the optical axis */
  int32_t width, height; /* pixels, 1 .. FSIM_CAM_MAX_SIZE; equal for all cameras of a handle */
} fsim_camera_t;

/* Replace the handle's camera set (n_cam = 1 .. FSIM_CAM_MAX) and upload what the kernels need: the camera poses and the face planes
 * of the convex-hull colliders (hull_planes[n_planes][4] = n.x n.y n.z d in the geom frame, |n| = 1, inside where n . x <= d; the
 * planes of colliding geom k -- rows of the model's colliding-geom table -- are rows hull_adr[k] .. hull_adr[k] + hull_num[k] - 1;
 * furniture_amd/camera.py computes them with scipy's ConvexHull).  The three tables may be NULL when the model has no mesh collider.
 * Host pointers, copied before return.  FSIM_EINVAL: an unknown body, fovy outside (0, 180), znear <= 0 or zfar <= znear, a size that is
 * zero, above the cap or different between cameras, more cameras / planes than the caps, a mesh collider without planes, a model with
 * more than FSIM_CAM_MAX_GEOMS colliding geoms. */
int fsim_set_cameras(fsim_t *, int n_cam, const fsim_camera_t *cams, int n_planes, const float *hull_planes, const int32_t *hull_adr,
                     const int32_t *hull_num);

/* Render every env from every camera: depth_dev float32 and seg_dev int32, each [n_envs][n_cam][height][width] (either may be NULL).
 * Renders the state fsim_sync leaves: a step still in flight is first waited for and its envs that overflowed the contact slots are
 * re-stepped (the overflow re-step ladder), exactly as fsim_sync does; then two launches are enqueued on the handle's stream (poses,
 * rays) and the call returns without waiting for them.  Reads the env records and writes nothing but the two images and a scratch
 * buffer of the handle: no state, RNG draw, look-ahead shadow or counter changes.  FSIM_EINVAL: no cameras set, both pointers NULL. */
int fsim_render(fsim_t *, float *depth_dev, int32_t *seg_dev);

#ifdef __cplusplus
}
#endif
#endif
