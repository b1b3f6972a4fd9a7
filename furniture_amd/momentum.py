"""Centre-of-mass, momentum and energy sensors computed on the device (include/fsim_momentum.h, csrc/fsim_momentum.hpp).

MuJoCo's subtreecom, subtreelinvel, subtreeangmom, mj_jacSubtreeCom and data.energy for every env, of sets of bodies rather than of
subtrees alone: a pure function of qpos and qvel of the env record.  A MomentumSensor is a set of model bodies (names or model body ids),
each with its kinematic subtree unless subtree=False -- connected furniture parts are joined by welds, not by the tree, so "the table so
far" is a list of parts.  Per sensor the device gives mom_com (float32 [3], the set's centre of mass, world frame), mom_linvel (float32
[3], its velocity; the linear momentum is this times masses()) and mom_angmom (float32 [3], the angular momentum about that centre of
mass, world frame) and, with jacobian=True, mom_jac (float32 [3, nv]: mom_linvel = mom_jac @ qvel, exact zeros in the columns of dofs
that move none of the set's bodies); per env, with energy=True, mom_energy (float32 [2]: the potential energy of the bodies that move,
then the kinetic energy with the armature in it).  A body without a joint of its own was folded into its moving ancestor when the model
was compiled and stands for that compiled body with everything folded into it.  The contract is the header's.
"""

import numpy as np

MAX_SENSORS = 64  # FSIM_MOM_MAX_SENSORS
MAX_BODIES = 32   # reduced bodies the device pass holds
MAX_NV = 128      # dofs the device pass holds
SENSOR_KEYS = ("mom_com", "mom_linvel", "mom_angmom")
JAC_KEYS = ("mom_jac",)
ENERGY_KEYS = ("mom_energy",)
OUT_FIELDS = ("com", "linvel", "angmom", "jac", "energy")  # fsim_momentum_out_t


class MomentumSensor:
    """One sensor: the set of model bodies ``bodies`` (a name, a model body id, or a list of them), each with its kinematic subtree when
    ``subtree`` is true (one boolean for all, or one per body)."""

    def __init__(self, bodies, subtree=True):
        if isinstance(bodies, (str, int, np.integer)) and not isinstance(bodies, (bool, np.bool_)):
            bodies = [bodies]
        try:
            bodies = list(bodies)
        except TypeError:
            raise TypeError("MomentumSensor: bodies is a body name, a model body id or a list of them, not %r" % type(bodies).__name__)
        if not bodies:
            raise ValueError("MomentumSensor: an empty set of bodies")
        for b in bodies:
            if isinstance(b, (bool, np.bool_)) or not isinstance(b, (str, int, np.integer)):
                raise TypeError("MomentumSensor: a body is a name or a model body id, not %r" % (b,))
            if not isinstance(b, str) and int(b) < 0:
                raise ValueError("MomentumSensor: a negative body id (%d)" % int(b))
        if isinstance(subtree, (bool, np.bool_)):
            subtree = [bool(subtree)] * len(bodies)
        else:
            if not isinstance(subtree, (list, tuple, np.ndarray)) or len(subtree) != len(bodies) or not all(isinstance(v, (bool, np.bool_)) for v in subtree):
                raise ValueError("MomentumSensor: subtree is a boolean or one boolean per body (got %r)" % (subtree,))
        self.bodies = [b if isinstance(b, str) else int(b) for b in bodies]
        self.subtree = [bool(v) for v in subtree]

    def resolve(self, model):
        """[(model body id, subtree)]; refuses an unknown body and a body that does not move"""
        names = model.meta["body_names"]
        red = np.asarray(model.arrays["body_red"]).astype(np.int64)
        out = []
        for b, sub in zip(self.bodies, self.subtree):
            if isinstance(b, str):
                if b not in names:
                    raise ValueError("MomentumSensor: unknown body %r" % b)
                b = names.index(b)
            if not 0 <= b < len(red):
                raise ValueError("MomentumSensor: body %d is out of range (the model has %d bodies)" % (b, len(red)))
            if red[b] <= 0:
                raise ValueError("MomentumSensor: body %r does not move (it is fixed in the world)" % names[b])
            out.append((b, sub))
        return out

    def __repr__(self):
        return "MomentumSensor(%r, subtree=%r)" % (self.bodies, self.subtree if len(set(self.subtree)) > 1 else self.subtree[0])


class MomentumSet:
    """The momentum sensors of a handle or env, in the style of WrenchSet.  jacobian: add mom_jac; energy: add mom_energy."""

    def __init__(self, sensors, jacobian=False, energy=False):
        self.sensors = [sensors] if isinstance(sensors, MomentumSensor) else list(sensors)
        for name, v in (("jacobian", jacobian), ("energy", energy)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("MomentumSet: %s is a boolean (got %r)" % (name, v))
        self.jacobian, self.energy = bool(jacobian), bool(energy)
        self.check()

    def check(self):
        """Host-side check of the set, before any device work (the names need the model: sensor_table)."""
        for k in self.sensors:
            if not isinstance(k, MomentumSensor):
                raise TypeError("MomentumSet: a list of furniture_amd.momentum.MomentumSensor, not %r" % type(k).__name__)
        if not 1 <= len(self.sensors) <= MAX_SENSORS:
            raise ValueError("MomentumSet: %d sensors (1 .. %d)" % (len(self.sensors), MAX_SENSORS))

    @property
    def n_sensors(self):
        return len(self.sensors)

    def keys(self):
        """the output keys, in the order of fsim_momentum_out_t"""
        return list(SENSOR_KEYS) + (list(JAC_KEYS) if self.jacobian else []) + (list(ENERGY_KEYS) if self.energy else [])

    def __repr__(self):
        return "MomentumSet(%d sensors, jacobian=%r, energy=%r)" % (len(self.sensors), self.jacobian, self.energy)


def check(spec):
    """Host-side check of a momenta= argument, before any device work."""
    if not isinstance(spec, MomentumSet):
        raise TypeError("momenta: a furniture_amd.momentum.MomentumSet, not %r" % type(spec).__name__)
    spec.check()


def sensor_table(model, momentum_set):
    """(adr [S + 1], bodies, subtree) int32 arrays of fsim_set_momenta for a momentum set against a compiled model (checked here first,
    then again by the library)"""
    check(momentum_set)
    nr = int(np.asarray(model.arrays["rdims"])[0])
    if nr > MAX_BODIES:
        raise ValueError("momenta: the model has %d reduced bodies (at most %d)" % (nr, MAX_BODIES))
    if model.nv > MAX_NV:
        raise ValueError("momenta: the model has nv = %d (at most %d)" % (model.nv, MAX_NV))
    adr, bodies, subtree = [0], [], []
    for i, k in enumerate(momentum_set.sensors):
        for b, sub in k.resolve(model):
            bodies.append(b)
            subtree.append(int(sub))
        adr.append(len(bodies))
    tab = tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (adr, bodies, subtree))
    for i, mask in enumerate(body_masks(model, tab)):
        if not sum(float(np.asarray(model.arrays["r_mass"], dtype=np.float64)[r]) for r in range(nr) if (mask >> r) & 1) > 0:
            raise ValueError("momenta: the bodies of sensor %d (%r) have zero total mass" % (i, momentum_set.sensors[i]))
    return tab


def body_masks(model, tab):
    """[S] Python ints: bit r set when reduced body r belongs to the sensor -- the listed bodies and, with subtree, every model body
    below them, each through body_red; a body counts once however often it is covered"""
    adr, bodies, subtree = tab
    A = model.arrays
    red = np.asarray(A["body_red"]).astype(np.int64)
    parent = np.asarray(A["body_parentid"]).astype(np.int64)
    masks = []
    for i in range(len(adr) - 1):
        mask = 0
        for b, sub in zip(bodies[adr[i]:adr[i + 1]], subtree[adr[i]:adr[i + 1]]):
            mask |= 1 << int(red[b])
            if sub:
                for d in range(int(b) + 1, len(red)):
                    up = d
                    while up > b:
                        up = int(parent[up])
                    if up == b and red[d] > 0:
                        mask |= 1 << int(red[d])
        masks.append(mask)
    return masks


def masses(model, momentum_set):
    """[S] float64: the mass of every sensor's set, a constant of the model (mom_linvel times it is the set's linear momentum)"""
    mass = np.asarray(model.arrays["body_mass"], dtype=np.float64)
    red = np.asarray(model.arrays["body_red"]).astype(np.int64)
    return np.array([sum(mass[b] for b in range(1, len(red)) if red[b] > 0 and (mask >> int(red[b])) & 1)
                     for mask in body_masks(model, sensor_table(model, momentum_set))], dtype=np.float64)


def moving_bodies(model, names=None):
    """the model body ids with a joint of their own, of the bodies ``names`` (all bodies when None)"""
    jointed = sorted(set(int(b) for b in np.asarray(model.arrays["dof_bodyid"])))
    if names is None:
        return jointed
    ids = set(model.meta["body_names"].index(n) for n in names)
    return [b for b in jointed if b in ids]


def part_sensors(model):
    """[MomentumSensor]: one per furniture part, in the order of the model's parts"""
    return [MomentumSensor(p, subtree=False) for p in model.meta["part_names"]]


def all_parts_sensor(model):
    """MomentumSensor: every furniture part together -- the furniture's centre of mass and momentum"""
    return MomentumSensor(list(model.meta["part_names"]), subtree=False)


def robot_sensor(model):
    """MomentumSensor: everything of the robot that moves (every jointed body that is not a furniture part); None for the Cursor agent,
    whose cursors do not move by joints"""
    names = model.meta["body_names"]
    parts = set(names.index(p) for p in model.meta["part_names"])
    ids = [b for b in moving_bodies(model) if b not in parts]
    return MomentumSensor(ids, subtree=False) if ids else None
