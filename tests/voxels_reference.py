"""Reference for the device voxel grids (include/fsim_voxels.h), written from the header's definitions in numpy float32.

``voxelize`` takes a dense map of fsim_render_points (every pixel's world point and its label, -1 for pixels that are not kept) and applies
the header's rule literally: the box test (inclusive), s_a = float32(dims_a) / (float32(hi_a) - float32(lo_a)) rounded once,
t = (p_a - lo_a) * s_a with each float32 operation rounded on its own (numpy does not fuse), i_a = min(floor(t), dims_a - 1), the cell
(i_x * dy + i_y) * dz + i_z, the count saturating at 32767 and the label of the smallest pix.  The device flushes denormals; a
difference p_a - lo_a below 2^-126 m lands in cell 0 either way.
"""

import numpy as np

SATURATE = 32767


def scale(dims, box):
    """s_a = dims_a / (hi_a - lo_a) in float32 (the host-side division of fsim_set_voxels)"""
    b = np.asarray(box, dtype=np.float32).reshape(2, 3)
    return np.asarray(dims, dtype=np.float32) / (b[1] - b[0])


def cells(xyz, dims, box):
    """xyz [K, 3] float32 points inside the box -> int64 [K] linear cell index"""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    b = np.asarray(box, dtype=np.float32).reshape(2, 3)
    d = np.asarray(dims, dtype=np.int64)
    t = (p - b[0]) * scale(dims, box)                                # float32: a subtraction, then a product, each rounded
    i = np.minimum(np.floor(t).astype(np.int64), d - 1)
    return (i[:, 0] * d[1] + i[:, 1]) * d[2] + i[:, 2]


def voxelize(xyz, pseg, dims, box):
    """xyz [..., 3] float32 world points in pix order (camera, row, column), pseg [...] labels (>= 0: kept, -1: not), dims (dx, dy, dz),
    box ((lo x, y, z), (hi x, y, z)) -> (count int16 [dx, dy, dz], label int16 [dx, dy, dz])"""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    g = np.asarray(pseg).reshape(-1)
    b = np.asarray(box, dtype=np.float32).reshape(2, 3)
    d = tuple(int(x) for x in dims)
    n = d[0] * d[1] * d[2]
    kept = np.nonzero((g >= 0) & np.all((p >= b[0]) & (p <= b[1]), axis=1))[0]  # ascending pix
    c = cells(p[kept], d, b)
    count = np.minimum(np.bincount(c, minlength=n), SATURATE).astype(np.int16)
    label = np.full(n, -1, dtype=np.int16)
    first_cell, first = np.unique(c, return_index=True)  # the first occurrence in pix order: the smallest pix of the cell
    label[first_cell] = g[kept[first]]
    return count.reshape(d), label.reshape(d)
