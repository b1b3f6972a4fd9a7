/* fsim_normals.h -- surface-normal and shaded images of libfsim.so, computed on the device from the cameras of fsim_camera.h (a C-ABI
 * of its own beside fsim.h, fsim_camera.h, fsim_points.h and fsim_voxels.h).
 *
 * The ray pass of fsim_render hits analytic surfaces, so the normal of a pixel is a closed form of its hit point: no finite differences
 * of the depth image, nothing wrong at a silhouette.  The shaded image is a Lambert-shaded, colour-by-geom picture of the collision
 * geometry -- a picture a person can look at, not the reference's RGB render (the compiled models hold no visual meshes).
 *
 * Surface point.  For a pixel with seg >= 0: q = the pixel's world point, bit-identical to the dense map's point of fsim_render_points
 * for that pixel (the same device function computes both), taken into the frame of the geom seg names: p = Rg^T (q - pos_g), with the
 * pose (pos_g, Rg: local -> world) the pose launch of this very call wrote for that geom.
 *
 * Local outward normal n, by geom type (r, h: radius and half-length; s: the box's half-sizes; (n_k, d_k): the hull's face planes of
 * fsim_set_cameras, in their order):
 *   plane     (0, 0, 1)
 *   sphere    p / |p|
 *   capsule   (p - c) / |p - c|,  c = (0, 0, clamp(p.z, -h, h))
 *   cylinder  (p.x, p.y, 0) / hypot(p.x, p.y)  when  hypot(p.x, p.y) - r >= |p.z| - h  (the side wins a tie),  else (0, 0, sign(p.z))
 *   box       sign(p_a) e_a  for the axis a with the largest |p_a| - s_a  (the smallest axis wins a tie)
 *   hull      n_k  of the face plane k with the largest n_k . p - d_k  (the smallest k wins a tie)
 *   sign(0) = +1.  A degenerate length (|.| < 1e-20) gives (0, 0, 0).
 * normal: Rg n -- world frame, unit length.  A surface seen from inside (the exit point of the camera contract: the camera centre is
 *   within the solid) keeps its OUTWARD normal, which then points away from the camera.  seg == -1 gives (0, 0, 0).
 *
 * shaded: RGBA8.  A pixel with seg == -1 gets background.  Otherwise lam = |normal . v|, v = the unit vector from q to the camera
 *   centre ((0, 0, 0) when its length is below 1e-20); I = ambient + (1 - ambient) * lam; each of R, G, B is
 *   (uint8) floorf(palette[seg][c] * I + 0.5f) (at most 255); A = palette[seg][3].  Each pixel is one 4-byte store.
 *
 * No side effects: fsim_render_normals writes no state, RNG draw, look-ahead shadow or counter.  An env's output depends only on its
 * own record, the camera set and the settings, never on the batch around it.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_NORMALS_H
#define FSIM_NORMALS_H
#include "fsim_camera.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Set the normals settings.  palette[ngeom][4]: RGBA by MODEL geom id (the numbering of the segmentation image), NULL = no palette
 * (normals only); background[4]: RGBA of a pixel that sees nothing, NULL = {0, 0, 0, 0}; ambient: 0 .. 1.  Host pointers, copied before
 * return (into small device tables of the handle; the image scratch is allocated by the first fsim_render_normals that needs it, and
 * freed by fsim_destroy).  FSIM_EINVAL: ambient outside [0, 1] or not finite, a model with more than FSIM_CAM_MAX_GEOMS colliding
 * geoms. */
int fsim_set_normals(fsim_t *, const uint8_t *palette, const uint8_t background[4], float ambient);

/* Renders the cameras once and derives the normal and / or shaded image, in one call, for one state: the state fsim_sync leaves,
 * settled exactly as fsim_render settles it (fsim_render's two launches, then one launch of the normal pass; the call returns without
 * waiting for them).  depth_dev / seg_dev: the camera images, as fsim_render writes them (either may be NULL: the handle's scratch is
 * used).  normal_dev float32 [n_envs][n_cam][height][width][3] (may be NULL), shaded_dev uint8 [n_envs][n_cam][height][width][4]
 * (may be NULL; 4-byte aligned; needs a palette).  FSIM_EINVAL: no cameras set, no normals settings (fsim_set_normals), both outputs
 * NULL, shaded_dev given without a palette or not 4-byte aligned. */
int fsim_render_normals(fsim_t *, float *depth_dev, int32_t *seg_dev, float *normal_dev, uint8_t *shaded_dev);

#ifdef __cplusplus
}
#endif
#endif
