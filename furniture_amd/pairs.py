"""Geom-pair distance sensors computed on the device (include/fsim_pairs.h, csrc/fsim_pairs.hpp, csrc/fsim_gjk.hpp).

A PairSensor has two sets of colliding geoms, side a and side b, and a largest distance dmax in metres: MuJoCo's distance / normal /
fromto sensors (mj_geomDistance).  Per sensor the device gives pair_distance (float32 metres between the nearest geom of a and the nearest
geom of b, negative when they overlap; dmax where nothing is within dmax: MuJoCo's distmax convention), pair_geoms (int32 [2]: the model
geom ids of the two, the numbering of camera_segmentation, so furniture_amd.camera.geom_labels applies; (-1, -1) = nothing) and, when asked
for, pair_fromto (float32 [6]: the nearest point on the geom of a, then on the geom of b, world frame) and pair_normal (float32 [3]: the
unit direction from a to b along which the distance is measured; to - from = distance * normal).  The query is geometric: collision masks
are ignored and geoms of one body or of welded bodies are not skipped.  While the cores of two geoms (a sphere's centre, a capsule's axis,
any other geom itself) are apart the distance is exact; once they intersect it is minus the portal depth of the step's own portal
routine, which is never shallower than the true overlap and may be deeper.  The contract is the header's.
"""

import numpy as np

from .camera import MAX_GEOMS
from .rays import mask_bits

MAX_SENSORS = 64         # FSIM_PAIR_MAX_SENSORS
MAX_PAIRS = 4096         # FSIM_PAIR_MAX_PAIRS, per sensor
MAX_TOTAL_PAIRS = 16384  # FSIM_PAIR_MAX_TOTAL, over the set
_PLANE = 0               # mjtGeom


def _side(name, spec):
    """a side as given: a body name, a list of body names, or a list of model geom ids -> ("bodies", [names]) or ("geoms", [ids])"""
    if isinstance(spec, str):
        return "bodies", [spec]
    try:
        items = list(spec)
    except TypeError:
        raise ValueError("PairSensor: %s is a body name, a list of body names or a list of model geom ids (got %r)" % (name, spec))
    if not items:
        raise ValueError("PairSensor: %s is empty" % name)
    if all(isinstance(k, str) for k in items):
        return "bodies", items
    if all(not isinstance(k, (str, bool, np.bool_)) and isinstance(k, (int, np.integer)) for k in items):
        return "geoms", [int(k) for k in items]
    raise ValueError("PairSensor: %s is a body name, a list of body names or a list of model geom ids (got %r)" % (name, spec))


def body_geoms(model, body):
    """[ncg] bool: the colliding geoms (rows of cg_orig) that the model body named ``body`` stands for -- the rule that makes a probe or
    ray sensor blind to the body it is mounted on (furniture_amd.rays.exclude_mask): the colliding geoms whose body mjcf/reduce.py folds
    into the same reduced body, which move rigidly with it; for a body welded to the world (reduced body 0: a cursor, the pedestal) only
    the geoms of the body itself, or the floor would belong to it."""
    A = model.arrays
    names = model.meta["body_names"]
    if body not in names:
        raise ValueError("PairSensor: unknown body %r (model %s + %s)" % (body, model.meta.get("agent"), model.meta.get("furniture_name")))
    b = names.index(body)
    cg_orig = np.asarray(A["cg_orig"]).astype(np.int64)
    gbody = np.asarray(A["geom_bodyid"]).astype(np.int64)[cg_orig]
    red = np.asarray(A["body_red"]).astype(np.int64)
    return gbody == b if red[b] == 0 else red[gbody] == red[b]


def gripper_bodies(model, arm=None):
    """the body names of the model's gripper(s): the bodies that carry a finger collider or the gripper base (Sawyer, Baxter; arm: None =
    every arm, or "right" / "left"), the cursor bodies for the Cursor agent.  As sides of a PairSensor they stand for their colliding
    geoms by body_geoms' rule (the gripper base brings the last arm link it is welded to)."""
    A = model.arrays
    names = model.meta["body_names"]
    cg_orig = np.asarray(A["cg_orig"]).astype(np.int64)
    gbody = np.asarray(A["geom_bodyid"]).astype(np.int64)[cg_orig]
    if "cursor_bodyid" in A and len(np.asarray(A["cursor_bodyid"])):
        return [names[int(b)] for b in np.asarray(A["cursor_bodyid"])]
    finger = np.asarray(A["cg_fingerrole"]) != 0
    out = []
    for b in sorted(set(gbody.tolist())):
        n = names[b]
        if (finger[gbody == b].any() or n.endswith("gripper_base")) and (arm is None or n.startswith(arm[0] + "_") or n.startswith(arm + "_")):
            out.append(n)
    if not out:
        raise ValueError("gripper_bodies: model %s + %s has no gripper%s" % (model.meta.get("agent"), model.meta.get("furniture_name"), "" if arm is None else " on arm %r" % arm))
    return out


class PairSensor:
    """One sensor: the distance between side ``a`` and side ``b``, each a model body name, a list of body names (a body stands for its
    colliding geoms: body_geoms) or a list of model geom ids (the numbering of camera_segmentation; a geom that does not collide is
    refused).  dmax: the largest distance reported, 0 < dmax < inf.  A geom may be on both sides; a pair of a geom with itself, or of
    two planes, is left out."""

    def __init__(self, a, b, dmax=1.0):
        self.a, self.b = _side("a", a), _side("b", b)
        self.dmax = float(dmax)
        if not (self.dmax > 0.0 and np.isfinite(self.dmax)):
            raise ValueError("PairSensor: needs 0 < dmax < inf (got %g)" % self.dmax)

    def side_masks(self, model):
        """([ncg] bool, [ncg] bool): the colliding geoms of side a and of side b"""
        A = model.arrays
        cg_orig = np.asarray(A["cg_orig"]).astype(np.int64)
        ngeom = len(A["geom_bodyid"])
        out = []
        for name, (kind, items) in (("a", self.a), ("b", self.b)):
            mask = np.zeros(len(cg_orig), dtype=bool)
            for k in items:
                if kind == "bodies":
                    mask |= body_geoms(model, k)
                else:
                    if not 0 <= k < ngeom:
                        raise ValueError("PairSensor: side %s names geom %d (the model has %d geoms)" % (name, k, ngeom))
                    if not (cg_orig == k).any():
                        raise ValueError("PairSensor: side %s names geom %d, which does not collide" % (name, k))
                    mask |= cg_orig == k
            if not mask.any():
                raise ValueError("PairSensor: side %s has no colliding geom (%r)" % (name, items))
            out.append(mask)
        return tuple(out)

    def pairs(self, model):
        """[(g1, g2)] colliding-geom indices of the sensor's pairs in the device's order (A-major): g1 != g2, not both planes"""
        ma, mb = self.side_masks(model)
        gtype = np.asarray(model.arrays["geom_type"]).astype(np.int64)[np.asarray(model.arrays["cg_orig"]).astype(np.int64)]
        return [(int(g1), int(g2)) for g1 in np.nonzero(ma)[0] for g2 in np.nonzero(mb)[0] if g1 != g2 and not (gtype[g1] == _PLANE and gtype[g2] == _PLANE)]

    def __repr__(self):
        return "PairSensor(a=%r, b=%r, dmax %g)" % (self.a[1], self.b[1], self.dmax)


class PairSet:
    """The pair sensors of a handle or env, in the style of ProbeSet.  fromto / normal: add pair_fromto / pair_normal to the outputs."""

    def __init__(self, sensors, fromto=False, normal=False):
        self.sensors = [sensors] if isinstance(sensors, PairSensor) else list(sensors)
        for name, v in (("fromto", fromto), ("normal", normal)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("PairSet: %s is a boolean (got %r)" % (name, v))
        self.fromto, self.normal = bool(fromto), bool(normal)
        self.check()

    def check(self):
        """Host-side check of the pair set, before any device work (the pair counts need the model: sensor_table)."""
        for k in self.sensors:
            if not isinstance(k, PairSensor):
                raise TypeError("PairSet: a list of furniture_amd.pairs.PairSensor, not %r" % type(k).__name__)
        if not 1 <= len(self.sensors) <= MAX_SENSORS:
            raise ValueError("PairSet: %d sensors (1 .. %d)" % (len(self.sensors), MAX_SENSORS))

    @property
    def n_sensors(self):
        return len(self.sensors)

    def __repr__(self):
        return "PairSet(%d sensors, fromto=%r, normal=%r)" % (len(self.sensors), self.fromto, self.normal)


def check(spec):
    """Host-side check of a pairs= argument, before any device work."""
    if not isinstance(spec, PairSet):
        raise TypeError("pairs: a furniture_amd.pairs.PairSet, not %r" % type(spec).__name__)
    spec.check()


def sensor_table(model, pair_set):
    """the fsim_pair_sensor_t array of a pair set against a compiled model (checked here first, then again by the library)"""
    from .sim import FsimPairSensor
    check(pair_set)
    ncg = len(model.arrays["cg_orig"])
    if ncg > MAX_GEOMS:
        raise ValueError("pairs: the model has %d colliding geoms (at most %d)" % (ncg, MAX_GEOMS))
    tab = (FsimPairSensor * len(pair_set.sensors))()
    total = 0
    for i, k in enumerate(pair_set.sensors):
        n = len(k.pairs(model))
        if n == 0:
            raise ValueError("pairs: sensor %d has no valid pair (every pair of its sides is a geom with itself or two planes)" % i)
        if n > MAX_PAIRS:
            raise ValueError("pairs: sensor %d has %d pairs (at most %d per sensor)" % (i, n, MAX_PAIRS))
        total += n
        if total > MAX_TOTAL_PAIRS:
            raise ValueError("pairs: more than %d pairs over the set (sensor %d brings it to %d)" % (MAX_TOTAL_PAIRS, i, total))
        t = tab[i]
        t.dmax = k.dmax
        for field, mask in zip((t.a, t.b), k.side_masks(model)):
            field[:] = mask_bits(mask)
    return tab
