/* fsim_points.h -- point-cloud observations of libfsim.so, built on the device from the cameras of fsim_camera.h (a C-ABI of its own
 * beside fsim.h and fsim_camera.h).
 *
 * Per env: the world points of the camera pixels that see a kept geom, fused over all cameras, cropped to a box, and either every
 * pixel's point (dense mode) or a fixed number of them chosen by farthest-point sampling (sampled mode).
 *
 * Kept pixel: a pixel is kept when all of these hold:
 *   - its segmentation is >= 0 (it sees a surface: depth <= zfar);
 *   - geom_keep[seg] is set (NULL geom_keep: every geom is kept);
 *   - its world point lies inside box, bounds inclusive, tested on the same fp32 values that are written out (NULL box: no crop).
 * Point of a pixel (world frame, fp32): the camera's world position plus the camera's rotation applied to the pixel's ray, scaled by
 * the pixel's depth: p = pos + (R (cx(i), cy(j), -1)) * depth, with the ray (cx(i), cy(j), -1) -- cx(i) = (i + 0.5 - W/2) * slope,
 * cy(j) = (H/2 - j - 0.5) * slope, slope = tan(fovy/2) / (H/2) -- and the pose (pos, R) exactly those of the ray pass of fsim_render.
 * Candidates: the kept pixels of an env in (camera, row, column) order; pix = cam*H*W + row*W + col.
 * Farthest-point sampling (FPS), K candidates, N = n_points rows:
 *   - row 0 is candidate 0; every candidate starts with dmin = +inf;
 *   - for rows 1 .. min(K, N) - 1: first dmin_k = min(dmin_k, dist2(c_k, previous row)) for every k, then the next row is the
 *     candidate with the largest dmin, the smallest index winning a tie;
 *   - dist2 = ((dx*dx + dy*dy) + dz*dz) in fp32, dx = x_k - x_prev, every product and sum rounded on its own (no fused multiply-add);
 *     the library is built to flush denormals: a squared distance below 2^-126 m^2 is 0 on the device;
 *   - K < N: rows K .. N-1 repeat row 0; K = 0: every row has xyz 0, pseg -1 and pix -1.
 * A sampled row's xyz is bit-identical to the dense map's point at its pix.
 *
 * No side effects: fsim_render_points writes no state, RNG draw, look-ahead shadow or counter.  An env's output depends only on its
 * own record, the camera set and the points settings, never on the batch around it.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP
 * addresses; work is enqueued on the handle's stream.
 */
#ifndef FSIM_POINTS_H
#define FSIM_POINTS_H
#include "fsim_camera.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FSIM_PTS_MAX_PIXELS = 16384, /* n_cam * width * height at render time: two 64 x 64 cameras, or one 128 x 128 */
  FSIM_PTS_MAX_POINTS = 4096   /* n_points */
};

/* Set the points settings.  n_points = 0: dense mode -- the world point of every pixel; n_points > 0: that many points per env by FPS.
 * geom_keep[ngeom] (model geom ids, nonzero = keep; NULL = keep every geom); box[6] = lo xyz, hi xyz in the world frame (NULL = no
 * crop).  Host pointers, copied before return (geom_keep into a small device table of the handle; the image and candidate scratch is
 * allocated by the first fsim_render_points that needs it, and freed by fsim_destroy).  FSIM_EINVAL: n_points outside
 * 0 .. FSIM_PTS_MAX_POINTS, a box bound that is not finite or lo > hi. */
int fsim_set_points(fsim_t *, int n_points, const uint8_t *geom_keep, const float *box);

/* Renders the cameras once and turns the result into points, in one call, for one state: the state fsim_sync leaves, settled exactly
 * as fsim_render settles it (fsim_render's two launches, then one launch in dense mode, two in sampled mode; the call returns without
 * waiting for them).  depth_dev / seg_dev: the camera images, as fsim_render writes them (either may be NULL: the handle's scratch is
 * used).  Dense mode: xyz_dev float [n_envs][n_cam][H][W][3] (every pixel's point, always finite), pseg_dev int32 [n_envs][n_cam][H][W]
 * (model geom id for kept pixels, -1 for all others); pix_dev is not used.  Sampled mode: xyz_dev float [n_envs][N][3], pseg_dev int32
 * [n_envs][N], pix_dev int32 [n_envs][N].  count_dev int32 [n_envs]: the number of kept pixels (K).  FSIM_EINVAL: no points settings
 * (fsim_set_points), no cameras set, n_cam * width * height > FSIM_PTS_MAX_PIXELS, a NULL output. */
int fsim_render_points(fsim_t *, float *depth_dev, int32_t *seg_dev, float *xyz_dev, int32_t *pseg_dev, int32_t *pix_dev,
                       int32_t *count_dev);

#ifdef __cplusplus
}
#endif
#endif
