"""Mass-matrix, inverse-inertia and bias-force tensors, the parts that run without a GPU: the float64 reference tests/dynamics_reference.py
against finite differences of the potential and the kinetic energy and against the body Jacobians, what fp32 alone does to M^-1 (the floor
tests/test_dynamics_gpu.py measures the device against), Dynamics validation, the dof table, the helpers, the refusals and the C-ABI of
include/fsim_dynamics.h (tests/test_dynamics_gpu.py runs the device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.dynamics import MAX_NV, Dynamics, arm_dofs, check, dof_table, tree_dofs
from furniture_amd.mjcf.model import load_compiled
from oracle.oracle_sim import OracleSim
from tests import dynamics_reference as dref
from tests.flow_reference import advance, set_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = dref.MODELS
# Central differences in float64.  Steps and tolerances were picked here, on the CPU, each tolerance about 10 x the residual measured
# over the four models (every test prints its own):
FD_H = 1e-5         # step of dV/dq: a hinge angle in rad, a slide or a free translation in m
GRAVITY_TOL = 6e-9  # |gravity - dV/dq| / max|gravity|: measured 5.6e-10 (Sawyer + table_lack_0825); truncation h^2 / 6 = 2e-11, the rest is the rounding of V over h
ASSEMBLY_TOL = 2e-14  # |M - sum_b (m Jp^T Jp + Jr^T I Jr) - diag(armature)| / max|M|: measured 2.1e-15 (Sawyer + table_lack_0825): two float64 evaluations of one quantity
SPD_SYM_TOL = 0.0   # full_M fills both triangles from one value
POWER_H = 1e-5      # time step of d/dt (v^T M v) along advance(qpos, v, +-h)
POWER_TOL = 3e-10   # |v^T (bias - gravity) - 1/2 d/dt (v^T M v)| / sum_ij |v_i M_ij v_j|: measured 2.3e-11 (Baxter + desk_mikael_1064)


@pytest.fixture(scope="module", params=MODELS, ids=[f for _, f in MODELS])
def case(request):
    """the reference of every state of the GPU file's random-state cases (the float32-rounded states the device holds)"""
    agent, furniture = request.param
    m = load_compiled(agent, furniture)
    qpos, qvel = dref.random_states(m, dref.n_envs(furniture))
    osim = OracleSim(m)
    refs = [dref.evaluate(osim, m, qpos[e], qvel[e]) for e in range(len(qpos))]
    yield dict(m=m, tag=furniture, qpos=qpos, qvel=qvel, refs=refs, osim=osim)
    osim.close()


def _potential(osim, m, qpos):
    set_state(osim, m, qpos, np.zeros(m.nv))
    g = np.asarray(m.arrays["opt"], dtype=np.float64)[1:4]
    return -float((np.asarray(m.arrays["body_mass"], dtype=np.float64)[:, None] * np.asarray(osim.data.xipos) * g[None, :]).sum())


def test_gravity_is_the_gradient_of_the_potential_energy(case):
    """gravity = dV/dq with V(q) = -sum_b m_b g . xipos_b, along each hinge and slide dof and the three translations of each free joint"""
    m, osim = case["m"], case["osim"]
    A = m.arrays
    worst, n = 0.0, 0
    for e in range(len(case["qpos"])):
        qpos, ref = case["qpos"][e], case["refs"][e]
        for jt, qa, da in zip(np.asarray(A["jnt_type"]), np.asarray(A["jnt_qposadr"]), np.asarray(A["jnt_dofadr"])):
            for k in range(3 if jt == 0 else 1):
                qp, qm = qpos.copy(), qpos.copy()
                qp[int(qa) + k] += FD_H
                qm[int(qa) + k] -= FD_H
                fd = (_potential(osim, m, qp) - _potential(osim, m, qm)) / (2 * FD_H)
                worst = max(worst, abs(fd - ref["gravity"][int(da) + k]) / np.abs(ref["gravity"]).max())
                n += 1
    print("%s measured: gravity against dV/dq over %d dofs: %.3e" % (case["tag"], n, worst))
    assert n >= 2 * 12 and worst <= GRAVITY_TOL


def test_mass_matrix_is_symmetric_positive_definite(case):
    for ref in case["refs"]:
        M = ref["M"]
        assert np.abs(M - M.T).max() <= SPD_SYM_TOL
        assert np.linalg.eigvalsh(M).min() > 0
        assert (M[~dref.structural_mask(case["m"])] == 0).all()  # zero across trees and across branches
        assert (ref["Minv"][~dref.tree_mask(case["m"])] == 0).all()


def test_mass_matrix_is_the_sum_of_the_bodies_kinetic_energies(case):
    """M = sum_b (m_b Jp^T Jp + Jr^T I_b Jr) + diag(armature), from body_jac at xipos"""
    m, osim = case["m"], case["osim"]
    A = m.arrays
    mass, inertia = np.asarray(A["body_mass"], dtype=np.float64), np.asarray(A["body_inertia"], dtype=np.float64).reshape(-1, 3)
    iquat = np.asarray(A["body_iquat"], dtype=np.float64).reshape(-1, 4)
    worst = 0.0
    for e in range(len(case["qpos"])):
        set_state(osim, m, case["qpos"][e], case["qvel"][e])
        M = np.diag(np.asarray(A["dof_armature"], dtype=np.float64))
        for b in range(1, m.nbody):
            if mass[b] == 0 and not inertia[b].any():
                continue
            jp, jr = osim.body_jac(b, np.array(osim.data.xipos[b]))
            R = np.asarray(osim.data.xmat[b]).reshape(3, 3) @ dref.q2m(iquat[b])
            M = M + mass[b] * jp.T @ jp + jr.T @ (R @ np.diag(inertia[b]) @ R.T) @ jr
        worst = max(worst, np.abs(M - case["refs"][e]["M"]).max() / np.abs(case["refs"][e]["M"]).max())
    print("%s measured: M against the bodies' kinetic energies: %.3e" % (case["tag"], worst))
    assert worst <= ASSEMBLY_TOL


def test_coriolis_power_is_half_the_rate_of_the_kinetic_energy_form(case):
    """The passivity of the Coriolis term: with c = bias - gravity, M' - 2 C is skew, so v^T c = 1/2 v^T M' v, M' = d/dt M(q(t)) along the
    motion q(t) = advance(qpos, v, t) at constant v (then d/dt (1/2 v^T M v) = v^T M v' + v^T c is the power balance v^T (tau - gravity))."""
    m, osim = case["m"], case["osim"]
    worst = 0.0
    for e in range(len(case["qpos"])):
        qpos, v, ref = case["qpos"][e], case["qvel"][e], case["refs"][e]
        form = []
        for h in (POWER_H, -POWER_H):
            set_state(osim, m, advance(m, qpos, v, h), v)
            form.append(v @ osim.full_M() @ v)
        rate = (form[0] - form[1]) / (2 * POWER_H)
        scale = np.abs(v[:, None] * ref["M"] * v[None, :]).sum()
        worst = max(worst, abs(v @ (ref["bias"] - ref["gravity"]) - 0.5 * rate) / scale)
    print("%s measured: v^T (bias - gravity) against 1/2 d/dt (v^T M v): %.3e" % (case["tag"], worst))
    assert worst <= POWER_TOL


def test_what_fp32_alone_does_to_the_inverse(case):
    """The floor of the device's minv measure: numpy's inverse of M rounded to float32, against Minv, on the random-state cases of
    tests/test_dynamics_gpu.py.  dref.MINV_FLOOR is the largest of these over the four models, written there beside the measured values."""
    m = case["m"]
    vals = [dref.measures(m, ref, np.arange(m.nv), minv=np.linalg.inv(ref["M"].astype(np.float32)))["minv"] for ref in case["refs"]]
    print("%s measured: fp32 floor of minv: %s (MINV_FLOOR %.3e)" % (case["tag"], " ".join("%.3e" % v for v in vals), dref.MINV_FLOOR))
    assert max(vals) == pytest.approx(dref.MINV_FLOOR_OF[case["tag"]], rel=0.25)  # (LAPACK builds may differ in what they round)
    assert max(dref.MINV_FLOOR_OF.values()) == dref.MINV_FLOOR


# ---- Dynamics, the dof table and the helpers -------------------------------------------------------------------------------------------
def test_dynamics_validation():
    for kw, msg in [(dict(dofs=[]), "empty"), (dict(dofs=[0, 1, 0]), "dof 0 is listed twice"), (dict(dofs=[1, -2]), "negative"), (dict(dofs=[0.5]), "dof indices"),
                    (dict(dofs="abc"), "dof indices"), (dict(dofs=[[0, 1]]), "dof indices"), (dict(mass=1), "boolean"), (dict(gravity="yes"), "boolean"),
                    (dict(mass=False, bias=False), "no output")]:
        with pytest.raises(ValueError, match=msg):
            Dynamics(**kw)
    d = Dynamics()
    assert d.dofs is None and d.mass and d.bias and not d.inverse and not d.gravity and d.keys() == ["dyn_mass", "dyn_bias"]
    d = Dynamics(dofs=np.array([3, 1, 2]), mass=False, inverse=True, bias=False, gravity=True)
    assert d.dofs == [3, 1, 2] and d.keys() == ["dyn_minv", "dyn_gravity"] and "3 dofs" in repr(d)
    with pytest.raises(TypeError, match="Dynamics"):
        check([0, 1, 2])
    d.dofs.append(3)  # check() looks again
    with pytest.raises(ValueError, match="dof 3 is listed twice"):
        check(d)


def test_dof_table():
    m = load_compiled("Sawyer", "table_lack_0825")
    t = dof_table(m, Dynamics())
    assert t.dtype == np.int32 and t.flags["C_CONTIGUOUS"] and t.tolist() == list(range(m.nv)) and m.nv == 39
    assert dof_table(m, Dynamics(dofs=[6, 0, 38])).tolist() == [6, 0, 38]  # the caller's order
    with pytest.raises(ValueError, match="dof 39 is out of range"):
        dof_table(m, Dynamics(dofs=[0, 39]))
    with pytest.raises(TypeError, match="Dynamics"):
        dof_table(m, [0, 1])

    class _Big:  # the caps: no shipped model is beyond them
        nv = MAX_NV + 1
        arrays = dict(rdims=np.array([20]))
    with pytest.raises(ValueError, match="nv = 129"):
        dof_table(_Big, Dynamics())
    _Big.nv, _Big.arrays = 30, dict(rdims=np.array([33]))
    with pytest.raises(ValueError, match="33 reduced bodies"):
        dof_table(_Big, Dynamics())


def test_arm_and_tree_dofs():
    s = load_compiled("Sawyer", "table_lack_0825")
    arms = arm_dofs(s)
    assert len(arms) == 1 and arms[0].tolist() == list(range(7)) and arms[0].dtype == np.int32
    assert tree_dofs(s, 3).tolist() == list(range(9))  # the arm with its two finger joints
    assert tree_dofs(s, 9).tolist() == list(range(9, 15)) and tree_dofs(s, 38).tolist() == list(range(33, 39))  # free parts
    b = load_compiled("Baxter", "desk_mikael_1064")
    arms = arm_dofs(b)
    assert len(arms) == 2 and all(len(a) == 7 for a in arms) and not set(arms[0].tolist()) & set(arms[1].tolist())
    names = b.meta["joint_names"] if "joint_names" in b.meta else None
    trees = [tree_dofs(b, int(a[0])) for a in arms]
    assert all(set(a.tolist()) <= set(t.tolist()) and len(t) == 9 for a, t in zip(arms, trees)) and not set(trees[0].tolist()) & set(trees[1].tolist())
    assert names is None or all(("right" in names[int(np.asarray(b.arrays["dof_jntid"])[d])]) == ("right" in names[int(np.asarray(b.arrays["dof_jntid"])[arms[k][0]])])
                                for k in range(2) for d in arms[k])
    c = load_compiled("Cursor", "toy_table")
    assert arm_dofs(c) == [] and tree_dofs(c, 7).tolist() == list(range(6, 12))
    with pytest.raises(ValueError, match="out of range"):
        tree_dofs(c, c.nv)
    # a tree's dofs are exactly the dofs M couples
    for m in (s, b, c):
        tm = dref.tree_mask(m)
        for d in (0, m.nv - 1):
            assert np.array_equal(np.nonzero(tm[d])[0], tree_dofs(m, d))


def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = Dynamics(dofs=[0, 1, 2])
    with pytest.raises(TypeError, match="Dynamics"):
        FurnitureBatchEnv("Sawyer", 1, dynamics=[0, 1, 2])
    with pytest.raises(NotImplementedError, match="dynamics= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, dynamics=spec)
    with pytest.raises(NotImplementedError, match="dynamics= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(dynamics=spec))

    class _Handle:  # a handle with a dof selection and nothing else
        cameras, points, voxels, normals, flow, rays, probes, pairs, frames, dyn = None, None, None, None, None, None, None, None, None, spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="dynamics tensors"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------
OTHER_HEADERS = ("fsim.h", "fsim_camera.h", "fsim_points.h", "fsim_voxels.h", "fsim_normals.h", "fsim_flow.h", "fsim_rays.h", "fsim_probes.h", "fsim_pairs.h", "fsim_frames.h")


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_dynamics_header_symbols_are_exported():
    assert sim.DYN_SYMBOLS == ["fsim_set_dynamics", "fsim_dynamics"]
    assert sorted(_declared("fsim_dynamics.h")) == sorted(sim.DYN_SYMBOLS)
    lists = [n for n in dir(sim) if n.endswith("_SYMBOLS") and n != "DYN_SYMBOLS"]
    assert len(lists) >= 10 and {"EXPORTED_SYMBOLS", "FRAME_SYMBOLS", "FLOW_SYMBOLS"} <= set(lists)
    assert not set(sim.DYN_SYMBOLS) & set().union(*[set(getattr(sim, n)) for n in lists])
    others = [h for h in sorted(os.listdir(os.path.join(ROOT, "include"))) if h.endswith(".h") and h != "fsim_dynamics.h"]  # every other header, later ones too
    assert set(OTHER_HEADERS) <= set(others)
    assert not set(sim.DYN_SYMBOLS) & set().union(*[_declared(h) for h in others])
    lib = ctypes.CDLL(sim.build())
    for n in sim.DYN_SYMBOLS:
        assert hasattr(lib, n), n


def test_dynamics_header_is_plain_c11(tmp_path):
    src = tmp_path / "use_dynamics.c"
    src.write_text('#include <stdio.h>\n#include "fsim_dynamics.h"\n'
                   "int use(fsim_t *s, const int32_t *d, float *o) { return fsim_set_dynamics(s, 1, d) + fsim_dynamics(s, o, 0, 0, 0); }\n"
                   'int main(void) { printf("%d", FSIM_DYN_MAX_NV); return 0; }\n')
    stub = tmp_path / "stub.c"
    stub.write_text('#include "fsim_dynamics.h"\nint fsim_set_dynamics(fsim_t *s, int a, const int32_t *k) { (void)s; (void)k; return a; }\n'
                    "int fsim_dynamics(fsim_t *s, float *a, float *b, float *c, float *d) { (void)s; (void)a; (void)b; (void)c; (void)d; return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", str(src), str(stub), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == MAX_NV == 128
