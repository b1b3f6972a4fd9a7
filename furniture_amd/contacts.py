"""Contact-force and touch sensors computed on the device (include/fsim_contacts.h, csrc/fsim_contacts.hpp).

MuJoCo's sim.forward() followed by reading the contact forces (mj_contactForce, the touch sensor) for every env: a pure function of the
env record, evaluated at the record's state.  A ContactSensor has two sets of colliding geoms, side a and side b (b = None: every
colliding geom not in a).  Per sensor the device gives contact_force (float32 [3]: the net world-frame force that b exerts on a,
newtons), contact_touch (float32: the sum of the normal force magnitudes, never negative) and contact_count (int32: the listed contacts
between the sides, MuJoCo's ncon: within margin, whether or not they carry force); per env contact_status (int32, bit 0: contacts were
dropped, bit 1: the solve is not to be trusted) and, with contacts=True, the contact list itself, fsim_max_contacts rows per env in the
order of contact_geoms: con_geoms (int32 [C, 2], model geom ids, -1 behind the list), con_pos, con_normal (from geom 1 to geom 2),
con_dist, con_force (on geom 2's body) and con_fn.  Weld and joint-limit forces are not reported.  The contract is the header's.
"""

import numpy as np

from .pairs import _side, body_geoms

MAX_SENSORS = 64  # FSIM_CON_MAX_SENSORS
MAX_SLOTS = 64    # FSIM_CON_MAX_SLOTS
SENSOR_KEYS = ("contact_force", "contact_touch", "contact_count", "contact_status")
LIST_KEYS = ("con_geoms", "con_pos", "con_normal", "con_dist", "con_force", "con_fn")


def _named(name, spec):
    try:
        return _side(name, spec)
    except ValueError as e:  # (pairs._side speaks of its own class)
        raise ValueError(str(e).replace("PairSensor", "ContactSensor"))


class ContactSensor:
    """One sensor: the contacts between side ``a`` and side ``b``, each a model body name, a list of body names (a body stands for its
    colliding geoms: furniture_amd.pairs.body_geoms; gripper_bodies(model) is such a list) or a list of model geom ids (the numbering of
    camera_segmentation; a geom that does not collide is refused).  b = None: every colliding geom that is not in a.  The sides must
    not overlap."""

    def __init__(self, a, b=None):
        self.a = _named("a", a)
        self.b = None if b is None else _named("b", b)

    def _mask(self, model, name, side):
        A = model.arrays
        cg_orig = np.asarray(A["cg_orig"]).astype(np.int64)
        ngeom = len(A["geom_bodyid"])
        kind, items = side
        mask = np.zeros(len(cg_orig), dtype=bool)
        for k in items:
            if kind == "bodies":
                try:
                    mask |= body_geoms(model, k)
                except ValueError as e:
                    raise ValueError(str(e).replace("PairSensor", "ContactSensor"))
            else:
                if not 0 <= k < ngeom:
                    raise ValueError("ContactSensor: side %s names geom %d (the model has %d geoms)" % (name, k, ngeom))
                if not (cg_orig == k).any():
                    raise ValueError("ContactSensor: side %s names geom %d, which does not collide" % (name, k))
                if mask[cg_orig == k].any():
                    raise ValueError("ContactSensor: side %s lists geom %d twice" % (name, k))
                mask |= cg_orig == k
        if not mask.any():
            raise ValueError("ContactSensor: side %s has no colliding geom (%r)" % (name, items))
        return mask

    def side_masks(self, model):
        """([ncg] bool, [ncg] bool): the colliding geoms of side a and of side b (b = None: the complement of a)"""
        ma = self._mask(model, "a", self.a)
        if self.b is None:
            return ma, ~ma
        mb = self._mask(model, "b", self.b)
        if (ma & mb).any():
            g = int(np.asarray(model.arrays["cg_orig"])[np.nonzero(ma & mb)[0][0]])
            raise ValueError("ContactSensor: geom %d is on side a and on side b" % g)
        return ma, mb

    def __repr__(self):
        return "ContactSensor(a=%r, b=%r)" % (self.a[1], None if self.b is None else self.b[1])


class ContactSet:
    """The contact sensors of a handle or env, in the style of PairSet.  contacts: add the contact list (the con_* keys) to the outputs."""

    def __init__(self, sensors, contacts=False):
        self.sensors = [sensors] if isinstance(sensors, ContactSensor) else list(sensors)
        if not isinstance(contacts, (bool, np.bool_)):
            raise ValueError("ContactSet: contacts is a boolean (got %r)" % (contacts,))
        self.contacts = bool(contacts)
        self.check()

    def check(self):
        """Host-side check of the set, before any device work (the geoms need the model: sensor_table)."""
        for k in self.sensors:
            if not isinstance(k, ContactSensor):
                raise TypeError("ContactSet: a list of furniture_amd.contacts.ContactSensor, not %r" % type(k).__name__)
        if not 1 <= len(self.sensors) <= MAX_SENSORS:
            raise ValueError("ContactSet: %d sensors (1 .. %d)" % (len(self.sensors), MAX_SENSORS))

    @property
    def n_sensors(self):
        return len(self.sensors)

    def keys(self):
        """the output keys, in the order of fsim_contact_out_t"""
        return list(SENSOR_KEYS) + (list(LIST_KEYS) if self.contacts else [])

    def __repr__(self):
        return "ContactSet(%d sensors, contacts=%r)" % (len(self.sensors), self.contacts)


def check(spec):
    """Host-side check of a contacts= argument, before any device work."""
    if not isinstance(spec, ContactSet):
        raise TypeError("contacts: a furniture_amd.contacts.ContactSet, not %r" % type(spec).__name__)
    spec.check()


def sensor_table(model, contact_set):
    """the fsim_contact_sensor_t array of a contact set against a compiled model (checked here first, then again by the library); the
    geom-id lists it points to are kept alive by the array's ``keep`` attribute"""
    from .sim import FsimContactSensor
    import ctypes
    check(contact_set)
    cg_orig = np.asarray(model.arrays["cg_orig"]).astype(np.int32)
    tab = (FsimContactSensor * len(contact_set.sensors))()
    tab.keep = []
    for i, k in enumerate(contact_set.sensors):
        ma, mb = k.side_masks(model)
        ids_a = np.ascontiguousarray(cg_orig[ma])
        ids_b = np.ascontiguousarray(cg_orig[mb]) if k.b is not None else np.zeros(0, dtype=np.int32)
        if k.b is None and not mb.any():
            raise ValueError("contacts: sensor %d: side a holds every colliding geom, nothing is left for side b" % i)
        tab.keep += [ids_a, ids_b]
        t = tab[i]
        t.a = ids_a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        t.b = ids_b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if len(ids_b) else None
        t.na, t.nb = len(ids_a), len(ids_b)
    return tab


def part_sensors(model):
    """[ContactSensor]: one sensor per furniture part, in the order of the model's parts, each against everything else -- the floor, the
    robot or the cursors, the other parts.  Their contact_force is the net contact force on every part: the net-contact-force tensor."""
    return [ContactSensor(p) for p in model.meta["part_names"]]
