"""Mass-matrix, inverse-inertia and bias-force tensors, computed on the device (include/fsim_dynamics.h, csrc/fsim_dynamics.hpp).

The dynamics half of a user-side operational-space controller, tau = J^T Lambda a* + bias with Lambda = (J M^-1 J^T)^-1, next to the
Jacobians of furniture_amd.frames: MuJoCo's mj_fullM, mj_solveM and data.qfrc_bias for every env.  A Dynamics names the dofs the outputs
are restricted to and which outputs are wanted: dyn_mass (float32 [K, K]: M[dofs][:, dofs], the joint-space inertia with the armature on
its diagonal), dyn_minv (float32 [K, K]: the inverse of the WHOLE M restricted to dofs, so that J M^-1 J^T of a Jacobian supported on dofs
is exact), dyn_bias (float32 [K]: qfrc_bias[dofs], Coriolis, centrifugal and gravity forces) and dyn_gravity (float32 [K]: the same at
qvel = 0).  The contract is the header's.
"""

import numpy as np

MAX_NV = 128      # FSIM_DYN_MAX_NV
MAX_BODIES = 32   # reduced bodies the device pass holds
OUTPUTS = ("mass", "inverse", "bias", "gravity")
KEYS = dict(mass="dyn_mass", inverse="dyn_minv", bias="dyn_bias", gravity="dyn_gravity")


class Dynamics:
    """The dynamics tensors of a handle or env.  dofs: the dof indices the outputs are restricted to, distinct, in any order (None: all
    dofs of the model, in order); mass / inverse / bias / gravity: add dyn_mass / dyn_minv / dyn_bias / dyn_gravity to the outputs."""

    def __init__(self, dofs=None, mass=True, inverse=False, bias=True, gravity=False):
        if dofs is not None:
            try:
                arr = np.asarray(dofs)
            except (TypeError, ValueError):
                raise ValueError("Dynamics: dofs is a list of dof indices (got %r)" % (dofs,))
            if arr.ndim == 1 and arr.size == 0:
                raise ValueError("Dynamics: an empty dof list (None selects every dof)")
            if arr.ndim != 1 or arr.dtype.kind not in "iu":
                raise ValueError("Dynamics: dofs is a list of dof indices (got %r)" % (dofs,))
            dofs = [int(d) for d in arr]
        self.dofs = dofs
        for name, v in (("mass", mass), ("inverse", inverse), ("bias", bias), ("gravity", gravity)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("Dynamics: %s is a boolean (got %r)" % (name, v))
        self.mass, self.inverse, self.bias, self.gravity = bool(mass), bool(inverse), bool(bias), bool(gravity)
        self.check()

    def check(self):
        """Host-side check of the selection, before any device work (the range of the indices needs the model: dof_table)."""
        if not (self.mass or self.inverse or self.bias or self.gravity):
            raise ValueError("Dynamics: no output (mass, inverse, bias and gravity all False)")
        if self.dofs is not None:
            if len(self.dofs) < 1:
                raise ValueError("Dynamics: an empty dof list (None selects every dof)")
            if min(self.dofs) < 0:
                raise ValueError("Dynamics: dof %d is negative" % min(self.dofs))
            if len(set(self.dofs)) != len(self.dofs):
                raise ValueError("Dynamics: dof %d is listed twice" % next(d for i, d in enumerate(self.dofs) if d in self.dofs[:i]))

    def keys(self):
        """the output keys asked for, in the order of the C-ABI's pointers"""
        return [KEYS[k] for k in OUTPUTS if getattr(self, k)]

    def __repr__(self):
        return "Dynamics(dofs=%s, mass=%r, inverse=%r, bias=%r, gravity=%r)" % ("None" if self.dofs is None else "[%d dofs]" % len(self.dofs),
                                                                                self.mass, self.inverse, self.bias, self.gravity)


def check(spec):
    """Host-side check of a dynamics= argument, before any device work."""
    if not isinstance(spec, Dynamics):
        raise TypeError("dynamics: a furniture_amd.dynamics.Dynamics, not %r" % type(spec).__name__)
    spec.check()


def dof_table(model, spec):
    """the int32 dof list of a Dynamics against a compiled model (checked here first, then again by the library)"""
    check(spec)
    nr = int(np.asarray(model.arrays["rdims"])[0])
    if nr > MAX_BODIES:
        raise ValueError("dynamics: the model has %d reduced bodies (at most %d)" % (nr, MAX_BODIES))
    if model.nv > MAX_NV:
        raise ValueError("dynamics: the model has nv = %d (at most %d)" % (model.nv, MAX_NV))
    if model.nv < 1:
        raise ValueError("dynamics: the model has no dofs")
    dofs = list(range(model.nv)) if spec.dofs is None else spec.dofs
    if len(dofs) > model.nv:
        raise ValueError("dynamics: %d dofs (1 .. nv = %d)" % (len(dofs), model.nv))
    if max(dofs) >= model.nv:
        raise ValueError("dynamics: dof %d is out of range (the model has nv = %d)" % (max(dofs), model.nv))
    return np.ascontiguousarray(dofs, dtype=np.int32)


def arm_dofs(model):
    """[dofs of arm 0, dofs of arm 1, ...]: the dof indices of the robot's arm joints (without the gripper's), one int32 array per arm in
    the robot's joint order -- one of seven for Sawyer, two for Baxter, none ([]) for the Cursor agent."""
    adr = np.asarray(model.arrays["arm_dofadr"], dtype=np.int32)
    narm = len(np.asarray(model.arrays["eef_siteid"]))
    if narm == 0 or len(adr) == 0:
        return []
    if len(adr) % narm:
        raise ValueError("arm_dofs: %d arm joints on %d arms" % (len(adr), narm))
    per = len(adr) // narm
    return [adr[k * per:(k + 1) * per].copy() for k in range(narm)]


def tree_dofs(model, dof):
    """all dofs of the kinematic tree that holds ``dof``, in order (int32): an arm's dofs with its gripper's -- for Baxter, both arms --,
    or the six dofs of a free part.  dyn_minv over a whole tree is the inverse of that tree's block of M."""
    tree = np.asarray(model.arrays["dof_tree"])
    dof = int(dof)
    if not 0 <= dof < model.nv:
        raise ValueError("tree_dofs: dof %d is out of range (the model has nv = %d)" % (dof, model.nv))
    return np.nonzero(tree == tree[dof])[0].astype(np.int32)
