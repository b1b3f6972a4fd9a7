"""Reference mass matrix, inverse inertia and bias forces for the device's dynamics tensors (include/fsim_dynamics.h), in float64.

It builds on the oracle (oracle/oracle_sim.py) and shares no code with the device path: from an OracleSim set to a given qpos / qvel with
tests.flow_reference.set_state, M = full_M(), Minv = numpy's inverse of it, bias = data.qfrc_bias, and gravity = qfrc_bias after a second
forward() at qvel = 0.  tests/test_dynamics.py validates these four against finite differences of the potential and the kinetic energy and
against the body Jacobians.
"""

import numpy as np

from tests.flow_reference import set_state

# the cases of tests/test_dynamics_gpu.py (those of tests/test_frames_gpu.py: the last has nv = 91 and a body on bit 31 of the masks)
MODELS = [("Sawyer", "table_lack_0825"), ("Baxter", "desk_mikael_1064"), ("Cursor", "toy_table"), ("Baxter", "table_liden_0921")]
SEED = 21
# What fp32 does to M^-1 whatever the algorithm: the measure `minv` of numpy's inverse of M rounded to float32 against Minv, the largest
# over the random-state cases of each model (computed and checked by tests/test_dynamics.py::test_what_fp32_alone_does_to_the_inverse)
MINV_FLOOR_OF = {"table_lack_0825": 2.810e-7, "desk_mikael_1064": 1.672e-7, "toy_table": 4.013e-8, "table_liden_0921": 9.351e-8}
MINV_FLOOR = max(MINV_FLOOR_OF.values())


def n_envs(furniture):
    return 2 if furniture == "table_liden_0921" else 4


def random_states(model, n, seed=SEED):
    """[n, nq], [n, nv] float64 holding float32 values (what the device's record holds): the recipe of tests/test_frames_gpu.py --
    every part turned by a random unit quaternion and shifted, every joint uniform within its limits, qvel uniform(-1, 1)"""
    from tests.test_frames_gpu import _random_states
    qpos, qvel = _random_states(model, n, seed=seed)
    return qpos.astype(np.float32).astype(np.float64), qvel.astype(np.float32).astype(np.float64)


def q2m(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def evaluate(osim, model, qpos, qvel, cursor=None):
    """dict of M [nv, nv], Minv [nv, nv], bias [nv], gravity [nv] at (qpos, qvel); the oracle is left at (qpos, qvel)"""
    qpos, qvel = np.asarray(qpos, dtype=np.float64), np.asarray(qvel, dtype=np.float64)
    set_state(osim, model, qpos, np.zeros_like(qvel), cursor)
    gravity = np.array(osim.data.qfrc_bias, dtype=np.float64)
    set_state(osim, model, qpos, qvel, cursor)
    M = osim.full_M()
    return dict(M=M, Minv=np.linalg.inv(M), bias=np.array(osim.data.qfrc_bias, dtype=np.float64), gravity=gravity)


def tree_blocks(model):
    """[dofs of tree 0, dofs of tree 1, ...]"""
    tree = np.asarray(model.arrays["dof_tree"])
    return [np.nonzero(tree == t)[0] for t in range(int(tree.max()) + 1)] if len(tree) else []


def structural_mask(model):
    """[nv, nv] bool: the entries of M that can be non-zero -- both dofs in one kinematic tree and the reduced body of one an
    ancestor-or-self of the other's"""
    A = model.arrays
    anc = np.asarray(A["r_ancmask"]).astype(np.int64) & 0xffffffff
    dofb = np.asarray(A["dof_rbody"]).astype(np.int64)
    up = ((anc[dofb][:, None] >> dofb[None, :]) & 1).astype(bool)  # up[i, j]: body(j) is an ancestor-or-self of body(i)
    return up | up.T


def tree_mask(model):
    """[nv, nv] bool: both dofs in one kinematic tree"""
    tree = np.asarray(model.arrays["dof_tree"])
    return tree[:, None] == tree[None, :]


def measures(model, ref, dofs, mass=None, minv=None, bias=None, gravity=None):
    """The error measures of one env's outputs over the selection ``dofs`` against the reference ``ref``: mass, bias and gravity as the
    largest absolute error divided by the largest reference magnitude of that quantity in the env (over all dofs); minv as the largest,
    over its entries, of the absolute error divided by the largest |Minv| entry of the entry's own tree."""
    d = np.asarray(dofs, dtype=np.int64)
    out = {}
    if mass is not None:
        out["mass"] = np.abs(np.asarray(mass, dtype=np.float64) - ref["M"][np.ix_(d, d)]).max() / np.abs(ref["M"]).max()
    for key, got in (("bias", bias), ("gravity", gravity)):
        if got is not None:
            out[key] = np.abs(np.asarray(got, dtype=np.float64) - ref[key][d]).max() / max(np.abs(ref[key]).max(), 1e-300)
    if minv is not None:
        out["minv"] = (np.abs(np.asarray(minv, dtype=np.float64) - ref["Minv"][np.ix_(d, d)]) / minv_scale(model, ref["Minv"])[np.ix_(d, d)]).max()
    return out


def minv_scale(model, Minv):
    """[nv, nv]: for every entry, the largest |Minv| entry of the row dof's tree (Minv is zero across trees)"""
    tree = np.asarray(model.arrays["dof_tree"])
    per = np.array([np.abs(Minv[np.ix_(tree == t, tree == t)]).max() for t in range(int(tree.max()) + 1)])
    return np.broadcast_to(per[tree][:, None], Minv.shape)
