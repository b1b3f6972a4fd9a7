"""What-if clearance queries computed on the device (include/fsim_clearance.h, csrc/fsim_clearance.hpp).

A ClearanceSet lists hinge / slide dofs (an arm's joints, a whole tree, both arms of a Baxter), pair sensors (furniture_amd.pairs.PairSensor)
and, optionally, carry rules.  FSim.clearance(cand) / env.clearance(cand) then answer, for every env and each of K candidate values of
those dofs, what FSim.pair_distance would answer with the same sensors if the env's qpos held the candidate there: clearance_distance
(float32 [n, K, S]), clearance_geoms (int32 [n, K, S, 2]), clearance_valid (uint8 [n, K]: 0 where a candidate held a value that is not finite
and the env's own value was used instead) and, when asked for, clearance_fromto (float32 [n, K, S, 6]) and clearance_normal (float32
[n, K, S, 3]).  The env records are read and never written; joint ranges are not applied.  A carry rule (part, carrier body) moves the part
rigidly with the carrier -- a held leg with the gripper -- in the envs whose carry_mask byte has the rule's bit set.  The contract is the
header's; per pair and per sensor it is that of furniture_amd.pairs.
"""

import numpy as np

from . import pairs
from .pairs import PairSensor, body_geoms

MAX_DOFS = 32            # FSIM_CLR_MAX_DOFS
MAX_CANDIDATES = 1024    # FSIM_CLR_MAX_CANDIDATES, per env and call
MAX_CARRY = 8            # FSIM_CLR_MAX_CARRY
DEFAULT_SCRATCH_ROWS = 32768
_FREE, _SLIDE, _HINGE = 0, 2, 3  # mjtJoint


def _is_int(k):
    return not isinstance(k, (bool, np.bool_)) and isinstance(k, (int, np.integer))


class ClearanceSet:
    """The clearance set of a handle or env.  dofs: the dof indices (model.arm_dofadr, model.arrays["grip_dofadr"], ...) of hinge or slide
    joints, distinct, in the order of a candidate's columns.  sensors: a PairSensor or a list of them.  carry: a list of (part name,
    carrier body name) rules; rule r is bit r of an env's carry_mask byte.  max_candidates: the largest K of a call.  scratch_rows: pose
    rows of the device scratch (0: min(n_envs * max_candidates, 32768)); a call runs floor(scratch_rows / K) envs per pair of launches.
    fromto / normal: add clearance_fromto / clearance_normal to the outputs."""

    def __init__(self, dofs, sensors, carry=(), max_candidates=64, scratch_rows=0, fromto=False, normal=False):
        try:
            self.dofs = list(dofs)
        except TypeError:
            raise ValueError("ClearanceSet: dofs is a list of dof indices (got %r)" % (dofs,))
        self.sensors = [sensors] if isinstance(sensors, PairSensor) else list(sensors)
        try:
            self.carry = [tuple(r) for r in carry]
        except TypeError:
            raise ValueError("ClearanceSet: carry is a list of (part name, carrier body name) (got %r)" % (carry,))
        for name, v in (("fromto", fromto), ("normal", normal)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("ClearanceSet: %s is a boolean (got %r)" % (name, v))
        self.max_candidates, self.scratch_rows = max_candidates, scratch_rows
        self.fromto, self.normal = bool(fromto), bool(normal)
        self.check()

    def check(self):
        """Host-side check of the set, before any device work (what needs the model: clearance_tables)."""
        if not self.dofs:
            raise ValueError("ClearanceSet: no dofs listed (a candidate needs at least one hinge or slide joint; the Cursor agent has none)")
        if not all(_is_int(d) for d in self.dofs):
            raise ValueError("ClearanceSet: dofs is a list of dof indices (got %r)" % (self.dofs,))
        self.dofs = [int(d) for d in self.dofs]
        if len(self.dofs) > MAX_DOFS:
            raise ValueError("ClearanceSet: %d dofs (1 .. %d)" % (len(self.dofs), MAX_DOFS))
        if len(set(self.dofs)) != len(self.dofs):
            raise ValueError("ClearanceSet: a dof is listed twice (%r)" % (self.dofs,))
        for k in self.sensors:
            if not isinstance(k, PairSensor):
                raise TypeError("ClearanceSet: sensors is a list of furniture_amd.pairs.PairSensor, not %r" % type(k).__name__)
        if not 1 <= len(self.sensors) <= pairs.MAX_SENSORS:
            raise ValueError("ClearanceSet: %d sensors (1 .. %d)" % (len(self.sensors), pairs.MAX_SENSORS))
        if len(self.carry) > MAX_CARRY:
            raise ValueError("ClearanceSet: %d carry rules (0 .. %d)" % (len(self.carry), MAX_CARRY))
        for r in self.carry:
            if len(r) != 2 or not all(isinstance(n, str) for n in r):
                raise ValueError("ClearanceSet: a carry rule is (part name, carrier body name) (got %r)" % (r,))
        if len(set(r[0] for r in self.carry)) != len(self.carry):
            raise ValueError("ClearanceSet: a part is carried by two rules (%r)" % (self.carry,))
        if not _is_int(self.max_candidates) or not 1 <= self.max_candidates <= MAX_CANDIDATES:
            raise ValueError("ClearanceSet: max_candidates %r (1 .. %d)" % (self.max_candidates, MAX_CANDIDATES))
        if not _is_int(self.scratch_rows) or (self.scratch_rows != 0 and self.scratch_rows < self.max_candidates):
            raise ValueError("ClearanceSet: scratch_rows %r (0, or at least max_candidates = %d)" % (self.scratch_rows, self.max_candidates))

    @property
    def n_sensors(self):
        return len(self.sensors)

    @property
    def n_dofs(self):
        return len(self.dofs)

    def shapes(self, K):
        """{key: (shape, dtype name)} of a call with K candidates per env (without the n_envs dimension)"""
        s = self.n_sensors
        out = {"clearance_distance": ((K, s), "float32"), "clearance_geoms": ((K, s, 2), "int32"), "clearance_valid": ((K,), "uint8")}
        if self.fromto:
            out["clearance_fromto"] = ((K, s, 6), "float32")
        if self.normal:
            out["clearance_normal"] = ((K, s, 3), "float32")
        return out

    def __repr__(self):
        return "ClearanceSet(%d dofs, %d sensors, %d carry rules, max_candidates %d)" % (len(self.dofs), len(self.sensors), len(self.carry), self.max_candidates)


def check(spec):
    """Host-side check of a clearance= argument, before any device work."""
    if not isinstance(spec, ClearanceSet):
        raise TypeError("clearance: a furniture_amd.clearance.ClearanceSet, not %r" % type(spec).__name__)
    spec.check()


def clearance_tables(model, spec):
    """(int32 dofs, the fsim_pair_sensor_t array, the fsim_clr_carry_t array or None) of a clearance set against a compiled model
    (checked here first, then again by the library)"""
    from .sim import FsimClrCarry
    check(spec)
    A = model.arrays
    names = model.meta["body_names"]
    nv = len(A["dof_bodyid"])
    jtype = np.asarray(A["jnt_type"]).astype(np.int64)[np.asarray(A["dof_jntid"]).astype(np.int64)]
    for j, d in enumerate(spec.dofs):
        if not 0 <= d < nv:
            raise ValueError("clearance: dof %d (column %d) is out of range (the model has %d dofs)" % (d, j, nv))
        if jtype[d] not in (_SLIDE, _HINGE):
            raise ValueError("clearance: dof %d (column %d) is not the dof of a hinge or slide joint (a free joint's dofs cannot be candidates)" % (d, j))
    tab = pairs.sensor_table(model, pairs.PairSet(spec.sensors))
    carry = None
    if spec.carry:
        red = np.asarray(A["body_red"]).astype(np.int64)
        carry = (FsimClrCarry * len(spec.carry))()
        for r, (part, carrier) in enumerate(spec.carry):
            if part not in model.meta["part_names"]:
                raise ValueError("clearance: carry rule %d: %r is not a furniture part (%s)" % (r, part, ", ".join(model.meta["part_names"])))
            if carrier not in names:
                raise ValueError("clearance: carry rule %d: unknown carrier body %r" % (r, carrier))
            if red[names.index(carrier)] == red[names.index(part)]:
                raise ValueError("clearance: carry rule %d: the carrier body %r belongs to the part it carries" % (r, carrier))
            carry[r].part_body, carry[r].carrier_body = names.index(part), names.index(carrier)
    return np.ascontiguousarray(spec.dofs, dtype=np.int32), tab, carry


def _part_geoms(model):
    """[ncg] bool: the colliding geoms on furniture parts"""
    return np.asarray(model.arrays["cg_partid"]) >= 0


def _world_geoms(model):
    """[ncg] bool: the colliding geoms of the world body itself (the floor) -- not those of the bodies welded to it, the robot's own base
    (pedestal, arm base, head), which its first link touches for good"""
    A = model.arrays
    return np.asarray(A["geom_bodyid"]).astype(np.int64)[np.asarray(A["cg_orig"]).astype(np.int64)] == 0


def _ids(model, mask):
    cg_orig = np.asarray(model.arrays["cg_orig"]).astype(np.int64)
    return [int(g) for g in cg_orig[mask]]


def robot_clearance_sensors(model, dmax=1.0):
    """One PairSensor: the robot against everything it could hit.  Side a: the colliding geoms of the robot's moving bodies (every jointed
    body that is not a furniture part -- the body rule of furniture_amd.momentum.robot_sensor --, each standing for the geoms that move
    with it: furniture_amd.pairs.body_geoms).  Side b: every colliding geom on a furniture part and the geoms of the world body (the
    floor), without the robot's own base.  Self-collision of the arm is out of scope: a product of two sides cannot leave out the pairs
    of adjacent links, which touch for good.  A part the gripper holds is at distance <= 0 from it: give it a sensor of its own
    (carried_sensor) and leave its geoms out of this one where that matters."""
    from .momentum import moving_bodies
    names = model.meta["body_names"]
    parts = set(names.index(p) for p in model.meta["part_names"])
    bodies = [b for b in moving_bodies(model) if b not in parts]
    if not bodies:
        raise ValueError("robot_clearance_sensors: model %s + %s has no jointed robot body (the Cursor agent's cursors do not move by joints)"
                         % (model.meta.get("agent"), model.meta.get("furniture_name")))
    a = np.zeros(len(model.arrays["cg_orig"]), dtype=bool)
    for b in bodies:
        a |= body_geoms(model, names[b])
    return PairSensor(_ids(model, a), _ids(model, _part_geoms(model) | _world_geoms(model)), dmax=dmax)


def carried_sensor(model, part, dmax=1.0):
    """One PairSensor: the furniture part named ``part`` (the geoms that move with it) against the other parts and the world body's
    geoms -- what a part the gripper carries (a carry rule of the ClearanceSet) could hit.  The robot is on neither side: the gripper
    that holds the part touches it, and self-collision is out of scope as in robot_clearance_sensors."""
    if part not in model.meta["part_names"]:
        raise ValueError("carried_sensor: %r is not a furniture part (%s)" % (part, ", ".join(model.meta["part_names"])))
    a = body_geoms(model, part)
    return PairSensor(_ids(model, a), _ids(model, (_part_geoms(model) | _world_geoms(model)) & ~a), dmax=dmax)
