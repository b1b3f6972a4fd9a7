"""Flow / velocity images, the parts that run without a GPU: Flow validation, the refusals, the exported C-ABI of include/fsim_flow.h and
the float64 reference (tests/flow_reference.py) against central finite differences of the oracle's forward kinematics
(tests/test_flow_gpu.py runs the device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from furniture_amd import sim
from furniture_amd.camera import Camera
from furniture_amd.flow import Flow, check
from furniture_amd.mjcf.model import load_compiled
from oracle.oracle_sim import OracleSim
from tests import camera_reference as cref
from tests import flow_reference as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- Flow -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(flow=False, velocity=False), dict(flow=1), dict(velocity="yes"), dict(flow=None), dict(flow=True, velocity=0)])
def test_flow_validation(kw):
    with pytest.raises(ValueError):
        Flow(**kw)


def test_flow_accepts():
    s = Flow()
    assert s.flow and not s.velocity and repr(s) == "Flow(flow=True, velocity=False)"
    s = Flow(flow=False, velocity=np.bool_(True))
    assert not s.flow and s.velocity is True
    s = Flow(velocity=True)
    assert s.flow and s.velocity


def test_check_against_cameras():
    with pytest.raises(ValueError, match="needs cameras"):
        check(Flow(), None)
    with pytest.raises(ValueError, match="needs cameras"):
        check(Flow(), [])
    with pytest.raises(TypeError):
        check(dict(flow=True), [Camera((0, 0, 1))])
    check(Flow(velocity=True), [Camera((0, 0, 1), width=256, height=256)] * 8)  # no pixel cap


# ---- refusals (before any device work) ------------------------------------------------------------------------------------------
def test_refusals():
    from furniture_amd.dist import step_wait_and_gather
    from furniture_amd.envs import FurnitureBatchEnv
    from furniture_amd.mixed import FurnitureMixedBatchEnv
    from furniture_amd.vec_env import FurnitureVecEnv
    spec = Flow(velocity=True)
    with pytest.raises(ValueError, match="needs cameras"):
        FurnitureBatchEnv("Sawyer", 1, flow=spec)
    with pytest.raises(TypeError, match="Flow"):
        FurnitureBatchEnv("Sawyer", 1, cameras=[Camera((0, 0, 1))], flow=True)
    with pytest.raises(NotImplementedError, match="flow= is not supported by the mixed"):
        FurnitureMixedBatchEnv("Sawyer", ["table_lack_0825", "chair_agne_0010"], 4, flow=spec)
    with pytest.raises(NotImplementedError, match="flow= is not supported by the VecEnv"):
        FurnitureVecEnv("FurnitureSawyerEnv", 2, env_kwargs=dict(flow=spec))

    class _Handle:  # a handle with flow settings and nothing else
        cameras, points, voxels, normals, flow = None, None, None, None, spec

        def sync(self):
            raise AssertionError("refused before the sync")
    with pytest.raises(NotImplementedError, match="flow / velocity images"):
        step_wait_and_gather(_Handle(), None, None, None)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------
def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(fsim_\w+)\s*\(", src))


def test_flow_header_symbols_are_exported():
    assert sim.FLOW_SYMBOLS == ["fsim_render_flow"]
    assert sorted(_declared("fsim_flow.h")) == sorted(sim.FLOW_SYMBOLS)
    others = set(sim.EXPORTED_SYMBOLS) | set(sim.CAMERA_SYMBOLS) | set(sim.POINTS_SYMBOLS) | set(sim.VOXELS_SYMBOLS) | set(sim.NORMALS_SYMBOLS)
    assert not set(sim.FLOW_SYMBOLS) & others
    assert not set(sim.FLOW_SYMBOLS) & set().union(*[_declared(h) for h in ("fsim.h", "fsim_camera.h", "fsim_points.h", "fsim_voxels.h", "fsim_normals.h")])
    lib = ctypes.CDLL(sim.build())
    for n in sim.FLOW_SYMBOLS:
        assert hasattr(lib, n), n


def test_flow_header_is_plain_c11(tmp_path):
    src = tmp_path / "use_flow.c"
    src.write_text('#include "fsim_flow.h"\nint use(fsim_t *s, float *f) { return fsim_render_flow(s, 0, 0, f, 0); }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-c", str(src), "-I" + os.path.join(ROOT, "include"),
                           "-o", str(tmp_path / "use_flow.o")])


def test_flow_header_states_the_contract():
    src = open(os.path.join(ROOT, "include", "fsim_flow.h")).read()
    flat = " ".join(re.sub(r"(?m)^\s*/?\*+\s?", "", src).split())  # the comment's text without its leading stars
    for s in ("cx = (i + 0.5 - width / 2) s", "cy = (height / 2 - (j + 0.5)) s", "w = (R_b axis) qvel about the anchor x_b + R_b jpos",
              "v(x_b) = qvel[0:3], w = R_b qvel[3:6]", "Reduced body 0 (the world) has twist exactly 0", "contributes no velocity",
              "u = v_g + w_g x (q - pos_g)", "X' = R_c^T (u - v_c - w_c x (q - p_c))", "flow[0] = (X'_x - cx d') / (d s)",
              "flow[1] = -(X'_y - cy d') / (d s)", "flow[2] = d'", "seg == -1 gives (0, 0, 0) in both outputs", "per second of simulated time"):
        assert s in flat, s


# ---- the reference against finite differences -----------------------------------------------------------------------------------------
# Central differences of the oracle's forward kinematics with step FD_H: the truncation error is h^2 / 6 times a third derivative, the
# rounding error about 1e-16 / h.  Measured with this state and these cameras, in the measures of flow_reference.measures (largest over the
# hit pixels): velocity 3.7e-9, image-plane flow 1.0e-8, depth rate 2.7e-9 at h = 1e-4; 100 x those at h = 1e-3 and 0.09 x at h = 3e-5,
# i.e. truncation alone down to there.  The step is 1e-4 and the tolerance 10 x the largest value measured at it.
FD_H, FD_TOL = 1e-4, 1e-7
FW, FH = 24, 18


def _project(X, s):
    """camera-frame point -> (column, row, depth) as continuous pixel coordinates"""
    d = -X[..., 2]
    return np.stack([X[..., 0] / (d * s) + FW / 2.0 - 0.5, FH / 2.0 - 0.5 - X[..., 1] / (d * s), d], axis=-1)


def test_reference_matches_finite_differences():
    from tests.test_camera_gpu import _cameras
    m = load_compiled("Sawyer", "table_lack_0825")
    rng = np.random.RandomState(3)
    qpos = np.asarray(m.arrays["qpos0"], dtype=np.float64).copy()
    a = int(m.part_qposadr[1])
    quat = rng.normal(size=4)
    qpos[a + 3:a + 7] = quat / np.linalg.norm(quat)  # one part turned away from the identity: body-frame and world-frame spin differ
    qpos[a + 2] += 0.15
    qvel = rng.uniform(-1, 1, m.nv)
    cams = _cameras(m, qpos, "right_hand", FW, FH)
    osim = OracleSim(m)
    fref.set_state(osim, m, qpos, qvel)
    geoms = cref.model_geoms(m, osim.data.geom_xpos, osim.data.geom_xmat)
    depth, seg, frames = [], [], []
    for cam in cams:
        _, p, R = fref.camera_pose(osim, m, cam)
        d, s = cref.render(p, R, cam.fovy, FW, FH, cam.znear, cam.zfar, geoms)
        depth.append(d), seg.append(s)
        q = p + cref.pixel_rays(R, cam.fovy, FW, FH) * d[..., None]
        local = np.zeros_like(q)  # the material point, fixed in its geom's frame
        for g in np.unique(s[s >= 0]):
            Rg = np.asarray(osim.data.geom_xmat[g], dtype=np.float64).reshape(3, 3)
            local[s == g] = (q[s == g] - np.asarray(osim.data.geom_xpos[g])) @ Rg
        frames.append(local)
    depth, seg = np.stack(depth), np.stack(seg)
    ref = fref.render(osim, m, qpos, qvel, cams, depth, seg)
    proj, world = [], []
    for sign in (1.0, -1.0):
        fref.set_state(osim, m, fref.advance(m, qpos, qvel, sign * FD_H), qvel)
        pj, wd = np.zeros((2, FH, FW, 3)), np.zeros((2, FH, FW, 3))
        for c, cam in enumerate(cams):
            _, p, R = fref.camera_pose(osim, m, cam)
            for g in np.unique(seg[c][seg[c] >= 0]):
                mask = seg[c] == g
                Rg = np.asarray(osim.data.geom_xmat[g], dtype=np.float64).reshape(3, 3)
                wd[c][mask] = np.asarray(osim.data.geom_xpos[g]) + frames[c][mask] @ Rg.T
            hit = seg[c] >= 0
            pj[c][hit] = _project((wd[c][hit] - p) @ R, ref["slope"][c])
        proj.append(pj), world.append(wd)
    osim.close()
    fd_flow, fd_vel = (proj[0] - proj[1]) / (2 * FD_H), (world[0] - world[1]) / (2 * FD_H)
    hit = seg >= 0
    body_red = np.asarray(m.arrays["body_red"])[np.asarray(m.arrays["geom_bodyid"])]
    wrist_rb = np.asarray(m.arrays["body_red"])[cams[1].body_id(m)]
    assert hit[0].sum() > 200 and hit[1].sum() > 200
    assert (hit[1] & (body_red[np.maximum(seg[1], 0)] != wrist_rb)).sum() > 20  # the wrist camera sees more than its own hand
    assert len(np.unique(seg[hit])) >= 8
    ms = fref.measures(ref, fd_flow, fd_vel)
    worst = {k: float(v[hit].max()) for k, v in ms.items()}
    print("finite differences at h = %g:" % FD_H, worst)
    assert (ref["flow"][~hit] == 0).all() and (ref["velocity"][~hit] == 0).all()
    assert np.abs(ref["flow"][hit]).max() > 1.0 and np.abs(ref["velocity"][hit]).max() > 0.1
    for k, v in worst.items():
        assert v <= FD_TOL, (k, v)
