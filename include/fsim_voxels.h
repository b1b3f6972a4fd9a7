/* fsim_voxels.h -- voxel-grid observations of libfsim.so, binned on the device from the cameras of fsim_camera.h (a C-ABI of its own
 * beside fsim.h, fsim_camera.h and fsim_points.h).
 *
 * Per env: a dx x dy x dz grid over an axis-aligned box of the world frame; every cell holds how many kept camera pixels land in it and
 * which geom the first of them sees.  Fused over all cameras.
 *
 * Kept pixel: the rule of fsim_points.h, with the box required -- its segmentation is >= 0, geom_keep[seg] is set (NULL geom_keep:
 * every geom is kept), and its world point lies inside box, bounds inclusive (lo <= p <= hi on every axis, in fp32).
 * Point of a pixel: bit-identical to the dense map's point of fsim_render_points for that pixel (the same device function computes both).
 * Cell of a kept point p, for each axis a (x, y, z):
 *   - s_a = (float)dims_a / (hi_a - lo_a), in fp32, computed once by the library on the host (IEEE, correctly rounded; the device's
 *     division is not);
 *   - t = (p_a - lo_a) * s_a on the device, each operation rounded on its own (no fused multiply-add);
 *   - i_a = min((int)floorf(t), dims_a - 1): p == hi falls into the last cell, p == lo into cell 0;
 *   - the cell is (i_x * dy + i_y) * dz + i_z.
 *   The library is built to flush denormals: a p_a - lo_a or t below 2^-126 is 0 on the device (it lands in cell 0 either way).
 * count: the number of kept pixels in the cell over all cameras, saturating at 32767; an empty cell has 0.
 * label: the model geom id (the segmentation) of the kept pixel in the cell with the smallest pix = cam*H*W + row*W + col (the
 *   candidate order of fsim_points.h); an empty cell has -1.
 * Both are integer functions of the points: the result does not depend on the order in which the device visits the pixels.
 *
 * No side effects: fsim_render_voxels writes no state, RNG draw, look-ahead shadow or counter.  An env's grid depends only on its own
 * record, the camera set and the voxel settings, never on the batch around it.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_VOXELS_H
#define FSIM_VOXELS_H
#include "fsim_camera.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FSIM_VOX_MAX_DIM = 256,     /* cells along one axis */
  FSIM_VOX_MAX_CELLS = 262144 /* dx * dy * dz: 64^3 */
};

/* Set the voxel settings.  dims[3] = dx, dy, dz (each 1 .. FSIM_VOX_MAX_DIM, product at most FSIM_VOX_MAX_CELLS); box[6] = lo xyz,
 * hi xyz in the world frame (required); geom_keep[ngeom] (model geom ids, nonzero = keep; NULL = keep every geom).  Host pointers,
 * copied before return (geom_keep into a small device table of the handle; the image scratch is allocated by the first
 * fsim_render_voxels that needs it, and freed by fsim_destroy).  FSIM_EINVAL: a NULL dims or box, a dim outside 1 .. FSIM_VOX_MAX_DIM,
 * dx * dy * dz > FSIM_VOX_MAX_CELLS, a box bound that is not finite, lo >= hi on some axis, an extent hi - lo or a scale s_a that is
 * not a finite normal fp32 (a box too thin or too wide for fp32), a model with ngeom > 32767 (labels are int16). */
int fsim_set_voxels(fsim_t *, const int32_t dims[3], const float box[6], const uint8_t *geom_keep);

/* Renders the cameras once and bins the result, in one call, for one state: the state fsim_sync leaves, settled exactly as fsim_render
 * settles it (fsim_render's two launches, then one binning launch; the call returns without waiting for them).  depth_dev / seg_dev:
 * the camera images, as fsim_render writes them (either may be NULL: the handle's scratch is used).  count_dev int16
 * [n_envs][dx][dy][dz] (z fastest), label_dev int16 [n_envs][dx][dy][dz].  FSIM_EINVAL: no voxel settings (fsim_set_voxels), no cameras
 * set, a NULL output. */
int fsim_render_voxels(fsim_t *, float *depth_dev, int32_t *seg_dev, int16_t *count_dev, int16_t *label_dev);

#ifdef __cplusplus
}
#endif
#endif
