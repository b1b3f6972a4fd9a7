"""Surface-normal and shaded images computed on the device from the cameras (include/fsim_normals.h, csrc/fsim_normals.hpp).

Per pixel: the exact outward normal of the collision surface the pixel sees (world frame, unit length, (0, 0, 0) where it sees nothing)
and / or a Lambert-shaded, colour-by-part RGBA picture of the collision geometry -- something a person can look at, not the reference's
RGB render (the compiled models hold no visual meshes).  The contract -- the surface point, the normal of every geom type and its tie
rules, the shading formula and its rounding -- is the header's.
"""

import numpy as np

from .camera import LABEL_ARENA, LABEL_ROBOT, geom_labels

ARENA_COLOR = (128, 128, 128)
ROBOT_COLOR = (200, 60, 50)
# parts: a fixed table of distinct colours, cycling
PART_COLORS = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (148, 103, 189), (140, 86, 75), (227, 119, 194), (188, 189, 34), (23, 190, 207),
               (174, 199, 232), (255, 187, 120), (152, 223, 138), (197, 176, 213), (196, 156, 148), (247, 182, 210), (219, 219, 141),
               (158, 218, 229))


def default_palette(model):
    """[ngeom, 4] uint8 RGBA by model geom id: the floor and the arena grey, the robot (or cursor) one colour, part k the k-th colour of
    PART_COLORS (cycling); opaque."""
    lab = geom_labels(model)
    pal = np.zeros((len(lab), 4), dtype=np.uint8)
    pal[:, 3] = 255
    pal[lab == LABEL_ARENA, :3] = ARENA_COLOR
    pal[lab == LABEL_ROBOT, :3] = ROBOT_COLOR
    parts = lab >= 0
    pal[parts, :3] = np.asarray(PART_COLORS, dtype=np.uint8)[lab[parts] % len(PART_COLORS)]
    return pal


def _rgba(name, v):
    a = np.asarray(v)
    if a.shape != (4,) or a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.number) or not np.all(np.isfinite(a)) or np.any(a != np.round(a)) \
            or np.any(a < 0) or np.any(a > 255):
        raise ValueError("Normals: %s %r must be four integers 0 .. 255 (RGBA)" % (name, v))
    return tuple(int(x) for x in a)


class Normals:
    """Settings of the normal / shaded images.  normal: add the normal image (float32 xyz per pixel).  shaded: add the shaded RGBA image.
    palette: [ngeom, 4] uint8 RGBA by model geom id, None = default_palette(model) (only the shaded image uses it).  background: RGBA of
    a pixel that sees nothing.  ambient: 0 .. 1, the part of a colour that does not depend on the surface's orientation."""

    def __init__(self, normal=True, shaded=False, palette=None, background=(30, 30, 40, 255), ambient=0.25):
        if not isinstance(normal, (bool, np.bool_)) or not isinstance(shaded, (bool, np.bool_)):
            raise ValueError("Normals: normal and shaded are booleans (got %r, %r)" % (normal, shaded))
        if not normal and not shaded:
            raise ValueError("Normals: neither the normal nor the shaded image is asked for")
        if palette is not None:
            p = np.asarray(palette)
            if p.ndim != 2 or p.shape[1] != 4 or p.dtype == np.bool_ or not np.issubdtype(p.dtype, np.number) or not np.all(np.isfinite(p)) \
                    or np.any(p != np.round(p)) or np.any(p < 0) or np.any(p > 255):
                raise ValueError("Normals: palette must be [ngeom, 4] integers 0 .. 255 (RGBA by model geom id)")
            palette = np.ascontiguousarray(p.astype(np.uint8))
        if isinstance(ambient, (bool, np.bool_)) or not isinstance(ambient, (int, float, np.integer, np.floating)) or not np.isfinite(ambient) or \
                not 0.0 <= ambient <= 1.0:
            raise ValueError("Normals: ambient %r (0 .. 1)" % (ambient,))
        self.normal, self.shaded, self.palette = bool(normal), bool(shaded), palette
        self.background, self.ambient = _rgba("background", background), float(np.float32(ambient))

    def palette_for(self, model):
        """the [ngeom, 4] uint8 palette the library gets for this model (None: normals only)"""
        if not self.shaded:
            return None
        if self.palette is None:
            return default_palette(model)
        if len(self.palette) != model.ngeom:
            raise ValueError("Normals: the palette has %d rows, the model %d geoms" % (len(self.palette), model.ngeom))
        return self.palette

    def __repr__(self):
        return "Normals(normal=%r, shaded=%r, palette=%s, background=%r, ambient=%g)" % (
            self.normal, self.shaded, "None" if self.palette is None else "[%d, 4]" % len(self.palette), self.background, self.ambient)


def check(spec, cameras):
    """Host-side check of the normals settings against a camera list, before any device work."""
    if not isinstance(spec, Normals):
        raise TypeError("normals: a furniture_amd.normals.Normals, not %r" % type(spec).__name__)
    if not cameras:
        raise ValueError("normals needs cameras: the images are derived from theirs (cameras=[Camera(...)])")


def save_ppm(path, rgba):
    """Write an [H, W, 3 or 4] uint8 image as a binary PPM (P6; alpha dropped)."""
    a = np.asarray(rgba)
    if a.ndim != 3 or a.shape[2] not in (3, 4) or a.dtype != np.uint8:
        raise ValueError("save_ppm: an [H, W, 3 or 4] uint8 image, not %s %s" % (a.dtype, a.shape))
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a[:, :, :3]).tobytes())
