"""ctypes binding to libfsim.so (the C-ABI in include/fsim.h).

torch is used only as the device-memory allocator / stream plumbing: every pointer that
crosses the boundary is ``tensor.data_ptr()``.  There is NO CPU fallback: if the HIP
library is missing or no GPU is visible, construction raises.
"""

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_LIBPATH = os.environ.get("FSIM_LIB", os.path.join(_CSRC, "libfsim.so"))
_LIB = None

INFO_DIM = 17
INFO_SUBTASK1, INFO_SUBTASK2 = 15, 16
INFO_DENSE_PHASE = 13
INFO_EPISODE_REWARD_F = 14
DENSE_STATEW = 27  # FSIM_DENSE_STATEW; ED_* of csrc/fsim_dense.hpp (subtask, phase, flags, fine-aligned, 4 x vec3, 11 prev values)
INFO_OVERFLOW = 12  # bits 0-1: this launch, bits 8-9: sticky (include/fsim.h)
E_OVERFLOW, E_NITER, E_MW_STEPS, E_EPISODE_COUNT = 6, 35, 36, 37  # words of env_block (csrc/fsim_model.hpp E_*)
INFO_NUM_CONNECTED, INFO_SUCCESS, INFO_FAIL, INFO_LAST_SITE1, INFO_LAST_SITE2, INFO_EPISODE_LENGTH = range(6)
INFO_CONNECTED_THIS_STEP, INFO_NEEDS_TABLE, INFO_SUCCESS_REWARD_F, INFO_TOUCH_REWARD_F, INFO_PICK_REWARD_F, INFO_CTRL_PENALTY_F = range(6, 12)
N_NOISE = 101  # _initialize_robot_pos draws per reset (furniture.py:1580, 1606-1611)


class FsimConfig(ctypes.Structure):
    _fields_ = [
        ("control_type", ctypes.c_int32), ("n_substeps", ctypes.c_int32), ("max_episode_steps", ctypes.c_int32),
        ("discrete_grip", ctypes.c_int32), ("rescale_actions", ctypes.c_int32), ("auto_align", ctypes.c_int32),
        ("num_connect_steps", ctypes.c_int32), ("auto_reset", ctypes.c_int32), ("solver_iterations", ctypes.c_int32),
        ("reset_robot_after_attach", ctypes.c_int32),
        ("solver_tolerance", ctypes.c_float),
        ("alignment_pos_dist", ctypes.c_float), ("alignment_rot_dist_up", ctypes.c_float),
        ("alignment_rot_dist_forward", ctypes.c_float), ("alignment_project_dist", ctypes.c_float),
        ("ctrl_penalty_coef", ctypes.c_float), ("unstable_penalty_coef", ctypes.c_float), ("success_reward", ctypes.c_float),
        ("touch_reward", ctypes.c_float), ("pick_reward", ctypes.c_float),
        ("furn_xyz_rand", ctypes.c_float), ("furn_rot_rand", ctypes.c_float), ("agent_xyz_rand", ctypes.c_float),
        ("move_speed", ctypes.c_float), ("rotate_speed", ctypes.c_float), ("cursor_boundary", ctypes.c_float),
        ("dense_reward", ctypes.c_int32), ("obs_bf16", ctypes.c_int32),
        ("multi_wave", ctypes.c_int32), ("lookahead_reset", ctypes.c_int32), ("overflow_restep", ctypes.c_int32),
    ]


MULTI_WAVE = {"auto": 0, "off": 1, "rule": 2, "all": 3}  # fsim_config_t::multi_wave


class StatePtrs(ctypes.Structure):
    _names = ["qpos", "qvel", "qacc_warmstart", "qfrc_bias", "ctrl", "qfrc_applied", "xfrc_applied", "eq_data", "eq_active",
              "geom_contype", "geom_conaffinity", "group", "qacc", "xpos", "xquat", "ncon", "contact_geoms", "solver_iters", "cursor", "dense", "env_block"]
    _fields_ = [(n, ctypes.c_void_p) for n in _names]


class FsimRaySensor(ctypes.Structure):
    """fsim_ray_sensor_t (include/fsim_rays.h)"""
    _fields_ = [("body", ctypes.c_int32), ("pos", ctypes.c_float * 3), ("quat", ctypes.c_float * 4), ("tmin", ctypes.c_float), ("tmax", ctypes.c_float),
                ("first_ray", ctypes.c_int32), ("n_rays", ctypes.c_int32), ("exclude", ctypes.c_uint32 * 3)]


class FsimProbeSensor(ctypes.Structure):
    """fsim_probe_sensor_t (include/fsim_probes.h)"""
    _fields_ = [("body", ctypes.c_int32), ("pos", ctypes.c_float * 3), ("quat", ctypes.c_float * 4), ("dmax", ctypes.c_float),
                ("first_probe", ctypes.c_int32), ("n_probes", ctypes.c_int32), ("exclude", ctypes.c_uint32 * 3)]


class FsimPairSensor(ctypes.Structure):
    """fsim_pair_sensor_t (include/fsim_pairs.h)"""
    _fields_ = [("a", ctypes.c_uint32 * 3), ("b", ctypes.c_uint32 * 3), ("dmax", ctypes.c_float)]


class FsimClrCarry(ctypes.Structure):
    """fsim_clr_carry_t (include/fsim_clearance.h)"""
    _fields_ = [("part_body", ctypes.c_int32), ("carrier_body", ctypes.c_int32)]


class FsimFrame(ctypes.Structure):
    """fsim_frame_t (include/fsim_frames.h)"""
    _fields_ = [("body", ctypes.c_int32), ("pos", ctypes.c_float * 3), ("quat", ctypes.c_float * 4)]


class FsimFrameSensor(ctypes.Structure):
    """fsim_frame_sensor_t (include/fsim_frames.h)"""
    _fields_ = [("frame", FsimFrame), ("ref", FsimFrame)]


class FsimContactSensor(ctypes.Structure):
    """fsim_contact_sensor_t (include/fsim_contacts.h)"""
    _fields_ = [("a", ctypes.POINTER(ctypes.c_int32)), ("b", ctypes.POINTER(ctypes.c_int32)), ("na", ctypes.c_int32), ("nb", ctypes.c_int32)]


CONTACT_OUT_FIELDS = ("force", "touch", "count", "status", "con_geoms", "con_pos", "con_normal", "con_dist", "con_force", "con_fn")


class FsimContactOut(ctypes.Structure):
    """fsim_contact_out_t (include/fsim_contacts.h): device pointers, None = not asked for"""
    _fields_ = [(k, ctypes.c_void_p) for k in CONTACT_OUT_FIELDS]


class FsimWrenchSensor(ctypes.Structure):
    """fsim_wrench_sensor_t (include/fsim_wrench.h)"""
    _fields_ = [("body", ctypes.c_int32), ("pos", ctypes.c_float * 3), ("quat", ctypes.c_float * 4)]


WRENCH_OUT_FIELDS = ("force", "torque", "accel", "angacc", "external", "qacc", "qfrc_constraint", "status")


class FsimWrenchOut(ctypes.Structure):
    """fsim_wrench_out_t (include/fsim_wrench.h): device pointers, None = not asked for"""
    _fields_ = [(k, ctypes.c_void_p) for k in WRENCH_OUT_FIELDS]


MOMENTUM_OUT_FIELDS = ("com", "linvel", "angmom", "jac", "energy")


class FsimMomentumOut(ctypes.Structure):
    """fsim_momentum_out_t (include/fsim_momentum.h): device pointers, None = not asked for"""
    _fields_ = [(k, ctypes.c_void_p) for k in MOMENTUM_OUT_FIELDS]


def library_path():
    return _LIBPATH


def build(force=False, verbose=False):
    """Compile libfsim.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".hpp"))]
    srcs += [os.path.join(os.path.dirname(_HERE), "include", h) for h in ("fsim.h", "fsim_camera.h", "fsim_points.h", "fsim_voxels.h", "fsim_normals.h", "fsim_flow.h", "fsim_rays.h", "fsim_probes.h", "fsim_pairs.h", "fsim_frames.h", "fsim_dynamics.h", "fsim_contacts.h", "fsim_wrench.h", "fsim_momentum.h", "fsim_clearance.h")]
    # the host helper is a library of its own with its own staleness: a checkout that has libfsim.so but no (or an old) libfsim_host.so
    # must not silently run the 100x slower Python sampler
    host_so, host_c = os.path.join(_CSRC, "libfsim_host.so"), os.path.join(_CSRC, "fsim_host.c")
    if force or not os.path.exists(host_so) or os.path.getmtime(host_c) > os.path.getmtime(host_so):
        try:
            build_host(verbose)
        except (OSError, subprocess.CalledProcessError) as e:  # optional: no gcc / no OpenMP -> the Python sampler (same stream, slower)
            import warnings
            warnings.warn("furniture_amd: libfsim_host.so could not be built (%s); reset tables will be drawn by the per-env Python loop" % e)
    if not force and os.path.exists(_LIBPATH) and all(os.path.getmtime(s) <= os.path.getmtime(_LIBPATH) for s in srcs):
        return _LIBPATH
    # (max-ilp: one wavefront per env has no other wave to hide latency behind, so the machine scheduler is asked to interleave
    #  independent chains rather than to minimise register pressure; +1.5 % on the benchmark, same register / scratch budget.
    #  -fno-optimize-sibling-calls: ONE tail call of an out-of-line device function is enough for the compiler to give up treating
    #  that function as "all callers known" -- it then saves its 113 callee-saved VGPRs to scratch on every call, 29 KB per wave.
    #  Without tail calls every local function drops its callee-saved area: 55 -> 33 KB of HBM traffic per env-step, DESIGN_HISTORY.md 6c)
    cmd = hipcc_command(_LIBPATH)
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return _LIBPATH


def hipcc_command(out, defines=()):
    """The one hipcc line that builds the library (``defines``: -D options of an opt-in variant, e.g. FSIM_MFMA_HESSIAN -- __graft_entry__.build()
    builds that one beside the default library so that the GPU suite can run it through the same C-ABI session)."""
    return ["hipcc", "--offload-arch=gfx950", "-O3", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-fgpu-flush-denormals-to-zero", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value",
            "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-fno-optimize-sibling-calls"] + ["-D" + d for d in defines] + ["-o", out, os.path.join(_CSRC, "fsim.hip")]


def build_variant(name, defines, force=False):
    """libfsim_<name>.so: the library with opt-in compile-time paths switched on (never loaded by the package itself)."""
    out = os.path.join(_CSRC, "libfsim_%s.so" % name)
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".hpp"))]
    if force or not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs):
        subprocess.check_call(hipcc_command(out, defines))
    return out


def build_host(verbose=False):
    """libfsim_host.so: plain-C host helper of the env layer (the reference's reset-time RNG stream for a whole batch per call)."""
    # (-ffp-contract=off: low + (high - low) * u rounds twice, as NumPy's uniform does -- gcc's default may fuse it where the target has an FMA)
    cmd = ["gcc", "-O2", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC", "-o", os.path.join(_CSRC, "libfsim_host.so"), os.path.join(_CSRC, "fsim_host.c"), "-lm"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIBPATH):
            raise RuntimeError(
                "libfsim.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                "furniture_amd has no CPU fallback for the hot path")
        import torch  # noqa: F401  -- first: torch must bind ITS HIP runtime before libfsim.so pulls in /opt/rocm's (else
        #                             torch.cuda.is_available() turns False in this process)
        L = ctypes.CDLL(_LIBPATH)
        L.fsim_last_error.restype = ctypes.c_char_p
        L.fsim_default_config.argtypes = [ctypes.POINTER(FsimConfig)]
        L.fsim_create.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.POINTER(FsimConfig),
                                  ctypes.POINTER(ctypes.c_void_p)]
        L.fsim_destroy.argtypes = [ctypes.c_void_p]
        L.fsim_destroy.restype = None
        L.fsim_dims.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int32)] * 7
        L.fsim_stream.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        L.fsim_sync.argtypes = [ctypes.c_void_p]
        L.fsim_physics_step.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.fsim_physics_forward.argtypes = [ctypes.c_void_p]
        L.fsim_get_state.argtypes = [ctypes.c_void_p, ctypes.POINTER(StatePtrs)]
        L.fsim_set_state.argtypes = [ctypes.c_void_p, ctypes.POINTER(StatePtrs)]
        L.fsim_max_contacts.argtypes = [ctypes.c_void_p]
        L.fsim_env_block_words.argtypes = [ctypes.c_void_p]
        L.fsim_kernel_variant.argtypes = [ctypes.c_void_p]
        L.fsim_tables_needed.argtypes = [ctypes.c_void_p]
        L.fsim_replay_is_aligned.argtypes = [ctypes.c_int] + [ctypes.c_float] * 4 + [ctypes.c_int] + [ctypes.c_void_p] * 8
        L.fsim_replay_try_connect.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
        L.fsim_replay_touch_scan.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
        L.fsim_kernel_variant.restype = ctypes.c_char_p
        L.fsim_step_kernel.argtypes = [ctypes.c_void_p]
        L.fsim_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        L.fsim_step_kernel.restype = ctypes.c_char_p
        L.fsim_lookahead_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_overflow_resteps.argtypes = [ctypes.c_void_p]
        L.fsim_overflow_resteps.restype = ctypes.c_int64
        L.fsim_set_reset_tables.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.fsim_reset.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_set_attach_noise.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_set_init_state.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_step.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 5
        L.fsim_set_max_episode_steps.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.fsim_kernel_time_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
        L.fsim_set_dense_reward.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.fsim_set_preassembled.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.fsim_dense_replay.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + \
            [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_set_cameras.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_render.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_set_points.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_render_points.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 6
        L.fsim_set_voxels.argtypes = [ctypes.c_void_p] * 4
        L.fsim_render_voxels.argtypes = [ctypes.c_void_p] * 5
        L.fsim_set_normals.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float]
        L.fsim_render_normals.argtypes = [ctypes.c_void_p] * 5
        L.fsim_render_flow.argtypes = [ctypes.c_void_p] * 5
        L.fsim_set_rays.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_cast_rays.argtypes = [ctypes.c_void_p] * 4
        L.fsim_set_probes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_probe_distance.argtypes = [ctypes.c_void_p] * 4
        L.fsim_set_pairs.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.fsim_pair_distance.argtypes = [ctypes.c_void_p] * 5
        L.fsim_set_frames.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.fsim_frame_state.argtypes = [ctypes.c_void_p] * 5
        L.fsim_set_dynamics.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.fsim_dynamics.argtypes = [ctypes.c_void_p] * 5
        L.fsim_set_contacts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.fsim_contact_forces.argtypes = [ctypes.c_void_p, ctypes.POINTER(FsimContactOut)]
        L.fsim_set_wrenches.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.fsim_wrenches.argtypes = [ctypes.c_void_p, ctypes.POINTER(FsimWrenchOut)]
        L.fsim_set_momenta.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.fsim_momenta.argtypes = [ctypes.c_void_p, ctypes.POINTER(FsimMomentumOut)]
        L.fsim_set_clearance.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.fsim_clearance.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 7
        _LIB = L
    return _LIB


EXPORTED_SYMBOLS = [
    "fsim_last_error", "fsim_default_config", "fsim_create", "fsim_destroy", "fsim_dims", "fsim_stream", "fsim_sync",
    "fsim_physics_step", "fsim_physics_forward", "fsim_get_state", "fsim_set_state", "fsim_max_contacts",
    "fsim_set_reset_tables", "fsim_reset", "fsim_step", "fsim_kernel_time_ms", "fsim_set_dense_reward", "fsim_dense_replay",
    "fsim_env_block_words", "fsim_set_max_episode_steps", "fsim_kernel_variant",
    "fsim_step_kernel", "fsim_lookahead_stats", "fsim_overflow_resteps",
    "fsim_replay_is_aligned", "fsim_replay_try_connect", "fsim_replay_touch_scan", "fsim_set_init_state", "fsim_tables_needed", "fsim_set_preassembled", "fsim_set_attach_noise",
    "fsim_read",
]
# the camera entry points: a header of their own (include/fsim_camera.h), exported by the same library
CAMERA_SYMBOLS = ["fsim_set_cameras", "fsim_render"]
# the point-cloud entry points: a header of their own (include/fsim_points.h), exported by the same library
POINTS_SYMBOLS = ["fsim_set_points", "fsim_render_points"]
# the voxel-grid entry points: a header of their own (include/fsim_voxels.h), exported by the same library
VOXELS_SYMBOLS = ["fsim_set_voxels", "fsim_render_voxels"]
# the normal / shaded image entry points: a header of their own (include/fsim_normals.h), exported by the same library
NORMALS_SYMBOLS = ["fsim_set_normals", "fsim_render_normals"]
# the flow / velocity image entry point: a header of its own (include/fsim_flow.h), exported by the same library
FLOW_SYMBOLS = ["fsim_render_flow"]
# the ray-sensor entry points: a header of their own (include/fsim_rays.h), exported by the same library
RAY_SYMBOLS = ["fsim_set_rays", "fsim_cast_rays"]
# the distance-probe entry points: a header of their own (include/fsim_probes.h), exported by the same library
PROBE_SYMBOLS = ["fsim_set_probes", "fsim_probe_distance"]
# the geom-pair distance entry points: a header of their own (include/fsim_pairs.h), exported by the same library
PAIR_SYMBOLS = ["fsim_set_pairs", "fsim_pair_distance"]
# the frame-sensor entry points: a header of their own (include/fsim_frames.h), exported by the same library
FRAME_SYMBOLS = ["fsim_set_frames", "fsim_frame_state"]
# the dynamics-tensor entry points: a header of their own (include/fsim_dynamics.h), exported by the same library
DYN_SYMBOLS = ["fsim_set_dynamics", "fsim_dynamics"]
# the contact-force entry points: a header of their own (include/fsim_contacts.h), exported by the same library
CONTACT_SYMBOLS = ["fsim_set_contacts", "fsim_contact_forces"]
# the wrench-sensor entry points: a header of their own (include/fsim_wrench.h), exported by the same library
WRENCH_SYMBOLS = ["fsim_set_wrenches", "fsim_wrenches"]
# the momentum-sensor entry points: a header of their own (include/fsim_momentum.h), exported by the same library
MOMENTUM_SYMBOLS = ["fsim_set_momenta", "fsim_momenta"]
# the clearance-query entry points: a header of their own (include/fsim_clearance.h), exported by the same library
CLEARANCE_SYMBOLS = ["fsim_set_clearance", "fsim_clearance"]


def preassembled_rows(model, preassembled):
    """(ids, connector pairs, angles) of fsim_set_preassembled for the reference's `preassembled` list.  With a recipe, row i holds
    the connector-table indices of site_recipe[i]'s site2 and site1 -- the reset calls _connect(site2_id, site1_id)
    (furniture.py:1546-1554) -- and the recipe's angle (NaN: none)."""
    ids = np.ascontiguousarray([int(x) for x in preassembled], dtype=np.int32)
    if not model.meta.get("has_recipe"):
        return ids, None, None
    sites = list(model.meta["site_names"])
    conn = [int(x) for x in model.conn_siteid]
    pairs, angles = np.zeros((len(ids), 2), dtype=np.int32), np.full(len(ids), np.nan, dtype=np.float32)
    for r, i in enumerate(ids):
        row = model.meta["site_recipe"][int(i)]
        pairs[r] = [conn.index(sites.index(row[1])), conn.index(sites.index(row[0]))]
        if len(row) == 3:
            angles[r] = float(row[2])
    return ids, pairs, angles


def default_config():
    c = FsimConfig()
    lib().fsim_default_config(ctypes.byref(c))
    return c


class FsimError(RuntimeError):
    pass


def dense_replay(coef, subtasks, n_pre, obs0, obs, ac, connected, device=0):
    """fsim_dense_replay: the device reward state machine alone on recorded sensor values (parity hook).
    -> (reward float32 [T], flags int32 [T, 4] = done, success, phase, subtask)."""
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    coef, subtasks, obs0, obs, ac = f32(coef), f32(subtasks), f32(obs0), f32(obs), f32(ac)
    connected = np.ascontiguousarray(connected, dtype=np.uint8)
    T, nsub = len(ac), len(subtasks)
    assert obs.shape == (T, nsub, 40) and obs0.shape == (nsub, 40)
    rew, flags = np.zeros(T, np.float32), np.zeros((T, 4), np.int32)
    rc = lib().fsim_dense_replay(device, coef.ctypes.data, len(coef), subtasks.ctypes.data, nsub, int(n_pre), obs0.ctypes.data,
                                 obs.ctypes.data, ac.ctypes.data, ac.shape[1], connected.ctypes.data, T, rew.ctypes.data,
                                 flags.ctypes.data)
    if rc:
        raise FsimError("fsim_dense_replay rc=%d: %s" % (rc, lib().fsim_last_error().decode()))
    return rew, flags


def replay_is_aligned(p1, R1, p2, R2, nang, angles, pos_dist=0.1, rot_up=0.9, rot_fwd=0.9, proj_dist=0.3, device=0):
    """The device's _is_aligned on recorded site poses (include/fsim.h: fsim_replay_is_aligned) -> (ok [n] bool, target_quat [n, 4])."""
    f = lambda a, sh: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(sh))
    n = len(nang)
    p1, R1, p2, R2, ang = f(p1, (n, 3)), f(R1, (n, 9)), f(p2, (n, 3)), f(R2, (n, 9)), f(angles, (n, 4))
    na = np.ascontiguousarray(np.asarray(nang, dtype=np.int32))
    ok, tq = np.zeros(n, dtype=np.int32), np.zeros((n, 4), dtype=np.float32)
    rc = lib().fsim_replay_is_aligned(int(device), pos_dist, rot_up, rot_fwd, proj_dist, n, p1.ctypes.data, R1.ctypes.data, p2.ctypes.data,
                                      R2.ctypes.data, na.ctypes.data, ang.ctypes.data, ok.ctypes.data, tq.ctypes.data)
    if rc != 0:
        raise FsimError("fsim_replay_is_aligned rc=%d: %s" % (rc, lib().fsim_last_error().decode()))
    return ok.astype(bool), tq


class FSim:
    """One handle = n_envs environments of one compiled model on one GPU."""

    def __init__(self, model, n_envs, device=0, config=None):
        import torch

        if not torch.cuda.is_available():
            raise FsimError("no ROCm device visible: furniture_amd's hot path has no CPU fallback")
        self.torch = torch
        self.cm = model
        self.n_envs = int(n_envs)
        self.device = torch.device("cuda", device)
        self.cfg = config if config is not None else default_config()
        blob = model.to_blob()
        h = ctypes.c_void_p()
        rc = lib().fsim_create(blob, len(blob), self.n_envs, device, ctypes.byref(self.cfg), ctypes.byref(h))
        if rc:
            raise FsimError("fsim_create rc=%d: %s" % (rc, lib().fsim_last_error().decode()))
        self._h = h
        d = [ctypes.c_int32() for _ in range(7)]
        self._chk(lib().fsim_dims(self._h, *[ctypes.byref(x) for x in d]))
        self.nq, self.nv, self.nu, self.dof_action, self.obs_dim, self.info_dim, self.stride = [x.value for x in d]
        self.max_contacts = lib().fsim_max_contacts(self._h)
        self.kernel_variant = lib().fsim_kernel_variant(self._h).decode()
        self.step_kernel = lib().fsim_step_kernel(self._h).decode()  # the launch structure fsim_config_t::multi_wave resolved to
        st = ctypes.c_void_p()
        self._chk(lib().fsim_stream(self._h, ctypes.byref(st)))
        # the handle's HIP stream as a torch stream: work enqueued under `with torch.cuda.stream(sim.torch_stream)` (an RCCL
        # collective, a copy) runs behind the step kernel without a host synchronisation
        self.torch_stream = torch.cuda.ExternalStream(st.value, device=self.device)
        self.env_block_words = lib().fsim_env_block_words(self._h)
        st = ctypes.c_void_p()
        self._chk(lib().fsim_stream(self._h, ctypes.byref(st)))
        self.stream_ptr = st.value

    def set_dense_reward(self, coef, subtasks):
        """Upload the dense-reward tables (furniture_amd.dense.pack_dense)."""
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        subtasks = np.ascontiguousarray(subtasks, dtype=np.float32)
        self._chk(lib().fsim_set_dense_reward(self._h, coef.ctypes.data, len(coef), subtasks.ctypes.data, len(subtasks)))

    def set_preassembled(self, preassembled, num_connects=None, welds=False):
        """config.preassembled / set_subtask (furniture.py:163, 204-207): weld ids (furniture without a recipe) or recipe step
        indices (with one) that every following reset starts from; num_connects as in config.num_connects.  welds=True: the list
        holds weld ids whatever the furniture (config.assembled: all of them)."""
        if welds:  # weld ids as they are: no recipe lookup (a furniture may have more welds than recipe steps)
            ids, pairs, angles = np.ascontiguousarray(list(preassembled), dtype=np.int32), None, None
        else:
            ids, pairs, angles = preassembled_rows(self.cm, preassembled)
        self._chk(lib().fsim_set_preassembled(self._h, len(ids), ids.ctypes.data, pairs.ctypes.data if pairs is not None else None,
                                              angles.ctypes.data if angles is not None else None, -1 if num_connects is None else int(num_connects)))

    def _chk(self, rc):
        if rc:
            raise FsimError("fsim rc=%d: %s" % (rc, lib().fsim_last_error().decode()))

    # -- raw physics -------------------------------------------------------
    def physics_step(self, n=1):
        self._chk(lib().fsim_physics_step(self._h, int(n)))

    def physics_forward(self):
        self._chk(lib().fsim_physics_forward(self._h))

    def sync(self):
        self._chk(lib().fsim_sync(self._h))

    _shapes = None

    def _field_shapes(self):
        m = self.cm
        return dict(qpos=(m.nq, "f"), qvel=(m.nv, "f"), qacc_warmstart=(m.nv, "f"), qfrc_bias=(m.nv, "f"), ctrl=(m.nu, "f"),
                    qfrc_applied=(m.nv, "f"), xfrc_applied=(6 * m.nparts, "f"), eq_data=(7 * m.neq, "f"), eq_active=(m.neq, "i"),
                    geom_contype=(m.ngeom, "i"), geom_conaffinity=(m.ngeom, "i"), group=(m.nparts, "i"), qacc=(m.nv, "f"),
                    xpos=(3 * m.nbody, "f"), xquat=(4 * m.nbody, "f"), ncon=(1, "i"), contact_geoms=(2 * self.max_contacts, "i"),
                    solver_iters=(1, "i"), cursor=(8, "f"), dense=(DENSE_STATEW, "f"), env_block=(self.env_block_words, "i"))

    def get_state(self, *names):
        """dict name -> torch tensor [n_envs, dim] (device)."""
        torch = self.torch
        shapes = self._field_shapes()
        names = names or [n for n in shapes if (n != "cursor" or self.cm.meta.get("agent") == "Cursor")
                          and (n != "dense" or self.cfg.dense_reward)]
        out, p = {}, StatePtrs()
        for n in names:
            dim, kind = shapes[n]
            # zero-filled (geom_contype / geom_conaffinity only receive their colliding-geom entries); the fill runs on torch's
            # stream, the copies on the handle's: the synchronize below orders them
            t = torch.zeros((self.n_envs, dim), dtype=torch.float32 if kind == "f" else torch.int32, device=self.device)
            out[n] = t
            setattr(p, n, t.data_ptr() if dim else None)
        torch.cuda.current_stream(self.device).synchronize()
        self._chk(lib().fsim_get_state(self._h, ctypes.byref(p)))
        self.sync()
        return out

    def set_state(self, **fields):
        torch = self.torch
        shapes = self._field_shapes()
        p, keep = StatePtrs(), []
        for n, v in fields.items():
            dim, kind = shapes[n]
            t = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v)
            t = t.to(device=self.device, dtype=torch.float32 if kind == "f" else torch.int32).reshape(-1, dim)
            if t.shape[0] == 1 and self.n_envs > 1:
                t = t.expand(self.n_envs, dim)
            t = t.contiguous()
            assert t.shape == (self.n_envs, dim), (n, t.shape)
            keep.append(t)
            setattr(p, n, t.data_ptr() if dim else None)
        torch.cuda.synchronize(self.device)
        self._chk(lib().fsim_set_state(self._h, ctypes.byref(p)))
        self.sync()

    # -- env hot path ------------------------------------------------------
    def set_reset_tables(self, part_qpos, robot_noise=None, mask=None):
        pq = np.ascontiguousarray(part_qpos, dtype=np.float32).reshape(self.n_envs, -1)
        rn = None
        n_noise = 0
        if robot_noise is not None:
            rn = np.ascontiguousarray(robot_noise, dtype=np.float32).reshape(self.n_envs, -1)
            n_noise = rn.shape[1] // max(1, len(self.cm.arm_qposadr))
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._chk(lib().fsim_set_reset_tables(self._h, None if mk is None else mk.ctypes.data, pq.ctypes.data,
                                              None if rn is None else rn.ctypes.data, n_noise))

    def set_attach_noise(self, noise, mask=None):
        """config.reset_robot_after_attach: the joint noise [n, narm joints] each env's NEXT attach re-poses the arm with
        (include/fsim.h: fsim_set_attach_noise)"""
        nz = np.ascontiguousarray(noise, dtype=np.float32).reshape(self.n_envs, -1)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._chk(lib().fsim_set_attach_noise(self._h, None if mk is None else mk.ctypes.data, nz.ctypes.data))

    def set_init_state(self, qpos=None, qvel=None, mask=None):
        """set_init_qpos for the masked envs (None = all); qpos None clears it (include/fsim.h: fsim_set_init_state)"""
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=np.uint8))
        if qpos is None:
            self._chk(lib().fsim_set_init_state(self._h, None if mk is None else mk.ctypes.data, None, None))
            return
        q = np.ascontiguousarray(np.broadcast_to(np.asarray(qpos, dtype=np.float32).reshape(-1, self.nq), (self.n_envs, self.nq)))
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(qvel, dtype=np.float32).reshape(-1, self.nv), (self.n_envs, self.nv)))
        self._chk(lib().fsim_set_init_state(self._h, None if mk is None else mk.ctypes.data, q.ctypes.data, v.ctypes.data))

    def reset(self, mask=None, obs=None):
        self._chk(lib().fsim_reset(self._h, None if mask is None else mask.data_ptr(), None if obs is None else obs.data_ptr()))

    def step(self, action, obs, reward, done, info):
        """Enqueue one FurnitureEnv.step() of every env on the handle's stream (asynchronous).  sync() before the next step():
        the counter tables_needed() reads lives in host memory and is cleared when a step is enqueued, so a second step enqueued
        without a sync in between loses the first one's reset notifications."""
        self._chk(lib().fsim_step(self._h, action.data_ptr(), obs.data_ptr(), reward.data_ptr(), done.data_ptr(), info.data_ptr()))

    def read_into(self, host_tensor, dev_tensor):
        """fsim_read: copy a device tensor into a (pinned) host tensor of the same size on the handle's transfer stream; complete on return"""
        nbytes = dev_tensor.numel() * dev_tensor.element_size()
        assert host_tensor.numel() * host_tensor.element_size() == nbytes and dev_tensor.is_contiguous() and host_tensor.is_contiguous()
        self._chk(lib().fsim_read(self._h, host_tensor.data_ptr(), dev_tensor.data_ptr(), nbytes))
        return host_tensor

    def tables_needed(self):
        """envs that consumed their reset table in the last step (valid after sync())"""
        return int(lib().fsim_tables_needed(self._h))

    def lookahead_stats(self):
        """fsim_lookahead_stats: dict(enabled, units (reset substeps run by look-ahead jobs), swapped, inline, jobs_per_launch, units_per_job) -- valid after sync()"""
        out = (ctypes.c_int64 * 6)()
        self._chk(lib().fsim_lookahead_stats(self._h, out))
        return dict(zip(("enabled", "units", "swapped", "inline", "jobs_per_launch", "units_per_job"), [int(x) for x in out]))

    def overflow_resteps(self):
        """fsim_overflow_resteps: env-steps repeated with a 64-slot layout because the step kernel's 48 contact slots did not hold them"""
        return int(lib().fsim_overflow_resteps(self._h))

    def set_max_episode_steps(self, n):
        self._chk(lib().fsim_set_max_episode_steps(self._h, int(n)))
        self.cfg.max_episode_steps = int(n)

    # -- env-logic replay hooks (include/fsim.h: fsim_replay_*) ------------------------------------------
    def replay_try_connect(self, part12, group, used, aligned, step_in, num_connect_steps):
        i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32))
        part12, group, used, step_in = i32(part12), i32(group), i32(used), i32(step_in)
        al = np.ascontiguousarray(np.asarray(aligned, dtype=np.uint8))
        n = len(step_in)
        out = np.zeros((n, 5), dtype=np.int32)
        self._chk(lib().fsim_replay_try_connect(self._h, n, int(num_connect_steps), part12.ctypes.data, group.ctypes.data, used.ctypes.data,
                                                al.ctypes.data, step_in.ctypes.data, out.ctypes.data))
        return out

    def replay_touch_scan(self, ncon, geoms, script):
        i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32))
        ncon, geoms = i32(ncon), i32(geoms)
        sc = np.ascontiguousarray(np.asarray(script, dtype=np.uint8))
        n, maxc = len(ncon), geoms.shape[1]
        masks, tried = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 4), dtype=np.int32)
        self._chk(lib().fsim_replay_touch_scan(self._h, n, maxc, ncon.ctypes.data, geoms.ctypes.data, sc.ctypes.data, masks.ctypes.data, tried.ctypes.data))
        return masks, tried

    # -- depth / segmentation cameras (include/fsim_camera.h, furniture_amd/camera.py) --------------------------------------
    cameras = None

    def set_cameras(self, cams):
        """Replace the handle's camera set (a list of furniture_amd.camera.Camera); validated by the library."""
        from .camera import camera_table, hull_plane_table
        cams = list(cams)
        tab = camera_table(self.cm, cams)
        planes, adr, num = hull_plane_table(self.cm)
        self._chk(lib().fsim_set_cameras(self._h, len(cams), tab.ctypes.data, len(planes), planes.ctypes.data if len(planes) else None,
                                         adr.ctypes.data, num.ctypes.data))
        self.cameras = cams

    def render(self, depth=True, segmentation=True, out=None):
        """Depth (float32, metres along the optical axis) and segmentation (int32 model geom id, -1 = nothing) images of every env from
        every camera, [n_envs, n_cam, H, W] device tensors (None for the one not asked for) of the state sync() leaves.  out: a
        (depth, segmentation) pair of tensors to render into instead of new ones.  Ordered with torch's current stream both ways."""
        torch = self.torch
        if not self.cameras:
            raise FsimError("render: no cameras set (FSim.set_cameras)")
        if not (depth or segmentation):
            raise ValueError("render: neither depth nor segmentation asked for")
        shape = (self.n_envs,) + self._image_shape()
        d, s = out if out is not None else (None, None)
        if depth and d is None:
            d = torch.empty(shape, dtype=torch.float32, device=self.device)
        if segmentation and s is None:
            s = torch.empty(shape, dtype=torch.int32, device=self.device)
        d, s = (d if depth else None), (s if segmentation else None)
        for t, dt in ((d, torch.float32), (s, torch.int32)):
            assert t is None or (tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous()), "render: out tensor of the wrong shape / type"
        self._sensor_call(lib().fsim_render, d.data_ptr() if d is not None else None, s.data_ptr() if s is not None else None)
        return d, s

    def _image_shape(self):
        """(C, H, W) of one env's images"""
        return (len(self.cameras), self.cameras[0].height, self.cameras[0].width)

    def _render_derived(self, name, fn, keys, want, images, out):
        """The part render_points / render_voxels / render_normals / render_flow share.  want: {key: (shape, dtype)} of the outputs (without the n_envs
        dimension), to which images=True adds the two images; out: a dict of tensors to write into (a missing key: a new tensor).  Calls
        fn(handle, depth, segmentation, *keys' tensors), NULL for a key that is not in want -> dict of tensors."""
        torch = self.torch
        if images:
            want = dict(want, camera_depth=(self._image_shape(), torch.float32), camera_segmentation=(self._image_shape(), torch.int32))
        res = {}
        for k, (shape, dt) in want.items():
            t = out.get(k) if out is not None else None
            if t is None:
                t = torch.empty((self.n_envs,) + shape, dtype=dt, device=self.device)
            assert tuple(t.shape) == (self.n_envs,) + shape and t.dtype == dt and t.is_contiguous(), "%s: out[%r] of the wrong shape / type" % (name, k)
            res[k] = t
        self._sensor_call(fn, *self._ptrs(res, ("camera_depth", "camera_segmentation") + keys))
        return res

    # -- point clouds from the cameras (include/fsim_points.h, furniture_amd/points.py) ------------------------------------------
    points = None

    def set_points(self, spec):
        """Set the point-cloud settings (a furniture_amd.points.PointCloud); checked on the host first, then by the library."""
        from .points import PointCloud, geom_keep
        if not isinstance(spec, PointCloud):
            raise TypeError("set_points: a furniture_amd.points.PointCloud, not %r" % type(spec).__name__)
        keep = np.ascontiguousarray(geom_keep(self.cm, spec.include), dtype=np.uint8)
        box = None if spec.box is None else np.ascontiguousarray(spec.box, dtype=np.float32).reshape(6)
        self._chk(lib().fsim_set_points(self._h, spec.n_points, keep.ctypes.data, None if box is None else box.ctypes.data))
        self.points = spec

    def points_shapes(self):
        """{key: (shape, dtype)} of render_points' outputs (without the n_envs dimension); dense mode has no point_cloud_pixel"""
        torch = self.torch
        n = self.points.n_points
        per = self._image_shape() if n == 0 else (n,)
        out = {"point_cloud": (per + (3,), torch.float32), "point_cloud_segmentation": (per, torch.int32), "point_cloud_count": ((), torch.int32)}
        if n > 0:
            out["point_cloud_pixel"] = ((n,), torch.int32)
        return out

    def render_points(self, images=False, out=None):
        """Render the cameras once and turn the images into points (include/fsim_points.h), for the state sync() leaves -> dict of device
        tensors: point_cloud (float32 world xyz), point_cloud_segmentation (int32 model geom id, -1 = none), point_cloud_count (int32 [n]:
        the kept pixels), in sampled mode point_cloud_pixel (int32 cam*H*W + row*W + col, -1 = none), and with images=True camera_depth /
        camera_segmentation [n, C, H, W] as FSim.render gives them.  out: a dict of such tensors to write into instead of new ones.
        Ordered with torch's current stream both ways."""
        if self.points is None:
            raise FsimError("render_points: no point-cloud settings (FSim.set_points)")
        if not self.cameras:
            raise FsimError("render_points: no cameras set (FSim.set_cameras)")
        return self._render_derived("render_points", lib().fsim_render_points, ("point_cloud", "point_cloud_segmentation", "point_cloud_pixel",
                                                                                "point_cloud_count"), self.points_shapes(), images, out)

    # -- voxel grids from the cameras (include/fsim_voxels.h, furniture_amd/voxels.py) ----------------------------------------------
    voxels = None

    def set_voxels(self, spec):
        """Set the voxel-grid settings (a furniture_amd.voxels.VoxelGrid); checked on the host first, then by the library."""
        from .points import geom_keep
        from .voxels import VoxelGrid
        if not isinstance(spec, VoxelGrid):
            raise TypeError("set_voxels: a furniture_amd.voxels.VoxelGrid, not %r" % type(spec).__name__)
        keep = np.ascontiguousarray(geom_keep(self.cm, spec.include), dtype=np.uint8)
        dims = np.ascontiguousarray(spec.dims, dtype=np.int32)
        box = np.ascontiguousarray(spec.box, dtype=np.float32).reshape(6)
        self._chk(lib().fsim_set_voxels(self._h, dims.ctypes.data, box.ctypes.data, keep.ctypes.data))
        self.voxels = spec

    def voxels_shapes(self):
        """{key: (shape, dtype)} of render_voxels' outputs (without the n_envs dimension)"""
        torch = self.torch
        return {"voxel_count": (self.voxels.dims, torch.int16), "voxel_segmentation": (self.voxels.dims, torch.int16)}

    def render_voxels(self, images=False, out=None):
        """Render the cameras once and bin the images into the voxel grid (include/fsim_voxels.h), for the state sync() leaves -> dict of
        device tensors [n, dx, dy, dz] (z fastest): voxel_count (int16 kept pixels per cell, saturating at 32767) and voxel_segmentation
        (int16 model geom id of the cell's first kept pixel in (camera, row, column) order, -1 = empty), and with images=True
        camera_depth / camera_segmentation [n, C, H, W] as FSim.render gives them.  out: a dict of such tensors to write into instead of
        new ones.  Ordered with torch's current stream both ways."""
        if self.voxels is None:
            raise FsimError("render_voxels: no voxel settings (FSim.set_voxels)")
        if not self.cameras:
            raise FsimError("render_voxels: no cameras set (FSim.set_cameras)")
        return self._render_derived("render_voxels", lib().fsim_render_voxels, ("voxel_count", "voxel_segmentation"), self.voxels_shapes(), images, out)

    # -- normal / shaded images from the cameras (include/fsim_normals.h, furniture_amd/normals.py) ----------------------------------
    normals = None

    def set_normals(self, spec):
        """Set the normal / shaded image settings (a furniture_amd.normals.Normals); checked on the host first, then by the library."""
        from .normals import Normals
        if not isinstance(spec, Normals):
            raise TypeError("set_normals: a furniture_amd.normals.Normals, not %r" % type(spec).__name__)
        pal = spec.palette_for(self.cm)
        bg = np.ascontiguousarray(spec.background, dtype=np.uint8)
        self._chk(lib().fsim_set_normals(self._h, pal.ctypes.data if pal is not None else None, bg.ctypes.data, spec.ambient))
        self.normals = spec

    def normals_shapes(self):
        """{key: (shape, dtype)} of render_normals' outputs (without the n_envs dimension)"""
        torch = self.torch
        img = self._image_shape()
        out = {}
        if self.normals.normal:
            out["camera_normal"] = (img + (3,), torch.float32)
        if self.normals.shaded:
            out["camera_shaded"] = (img + (4,), torch.uint8)
        return out

    def render_normals(self, images=False, out=None):
        """Render the cameras once and derive the normal and / or shaded image (include/fsim_normals.h), for the state sync() leaves ->
        dict of device tensors: camera_normal (float32 [n, C, H, W, 3], the world-frame unit outward normal of the surface the pixel
        sees, (0, 0, 0) where it sees nothing) and / or camera_shaded (uint8 [n, C, H, W, 4], RGBA), as the settings ask, and with
        images=True camera_depth / camera_segmentation [n, C, H, W] as FSim.render gives them.  out: a dict of such tensors to write
        into instead of new ones.  Ordered with torch's current stream both ways."""
        if self.normals is None:
            raise FsimError("render_normals: no normals settings (FSim.set_normals)")
        if not self.cameras:
            raise FsimError("render_normals: no cameras set (FSim.set_cameras)")
        return self._render_derived("render_normals", lib().fsim_render_normals, ("camera_normal", "camera_shaded"), self.normals_shapes(), images, out)

    # -- flow / velocity images from the cameras (include/fsim_flow.h, furniture_amd/flow.py) ------------------------------------------
    flow = None

    def set_flow(self, spec):
        """Set the flow / velocity image settings (a furniture_amd.flow.Flow).  Host only: the library has no settings for them."""
        from .flow import Flow
        if not isinstance(spec, Flow):
            raise TypeError("set_flow: a furniture_amd.flow.Flow, not %r" % type(spec).__name__)
        self.flow = spec

    def flow_shapes(self):
        """{key: (shape, dtype)} of render_flow's outputs (without the n_envs dimension)"""
        torch = self.torch
        img = self._image_shape()
        out = {}
        if self.flow.flow:
            out["camera_flow"] = (img + (3,), torch.float32)
        if self.flow.velocity:
            out["camera_velocity"] = (img + (3,), torch.float32)
        return out

    def render_flow(self, images=False, out=None):
        """Render the cameras once and derive the flow and / or velocity image (include/fsim_flow.h), for the state sync() leaves -> dict
        of device tensors: camera_flow (float32 [n, C, H, W, 3]: columns / s to the right, rows / s downward, depth rate in m/s of the
        material point the pixel sees) and / or camera_velocity (float32 [n, C, H, W, 3]: that point's world-frame velocity in m/s), as the
        settings ask, (0, 0, 0) where the pixel sees nothing, and with images=True camera_depth / camera_segmentation [n, C, H, W] as
        FSim.render gives them.  out: a dict of such tensors to write into instead of new ones.  Ordered with torch's current stream both
        ways."""
        if self.flow is None:
            raise FsimError("render_flow: no flow settings (FSim.set_flow)")
        if not self.cameras:
            raise FsimError("render_flow: no cameras set (FSim.set_cameras)")
        return self._render_derived("render_flow", lib().fsim_render_flow, ("camera_flow", "camera_velocity"), self.flow_shapes(), images, out)

    # -- what the state-sensor families below share (rays, probes, pairs, frames, dynamics, contacts, wrenches, momenta) ------------------
    def _set_sensors(self, fn, attr, spec, cls, install):
        """The part the set_X of these families share.  None clears the library's set (n = 0: it ignores the other arguments) and the attribute;
        anything but a `cls` is refused; install() builds the tables and hands them to fn, and only then is the spec stored."""
        if spec is None:
            self._chk(fn(self._h, *[0 if t is ctypes.c_int else None for t in fn.argtypes[1:]]))
        else:
            if not isinstance(spec, cls):
                raise TypeError("%s: a %s.%s, not %r" % (fn.__name__[len("fsim_"):], cls.__module__, cls.__name__, type(spec).__name__))
            install()
        setattr(self, attr, spec)

    def _sensor_outputs(self, name, want, out):
        """The output tensors of one sensor call.  want: {key: (shape, dtype)} as the family's X_shapes() gives it; out: None (a new tensor
        per key) or a dict of tensors to write into, whose keys alone are computed -> {key: tensor}."""
        torch = self.torch
        if out is not None:
            if not out or any(k not in want for k in out):
                raise ValueError("%s: out holds %s (of %s)" % (name, sorted(out), sorted(want)))
            want = {k: want[k] for k in want if k in out}
        res = {}
        for k, (shape, dt) in want.items():
            t = out[k] if out is not None else torch.empty((self.n_envs,) + shape, dtype=dt, device=self.device)
            if tuple(t.shape) != (self.n_envs,) + shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:  # (a raw pointer goes to the kernel)
                raise ValueError("%s: out[%r] is not a contiguous %s tensor of shape %s on %s" % (name, k, dt, (self.n_envs,) + shape, self.device))
            res[k] = t
        return res

    def _sensor_call(self, fn, *args):
        """fn(handle, *args) on the handle's stream, ordered with torch's current stream both ways"""
        cur = self.torch.cuda.current_stream(self.device)
        self.torch_stream.wait_stream(cur)  # (the outputs may be memory torch's stream has just released)
        self._chk(fn(self._h, *args))
        cur.wait_stream(self.torch_stream)

    @staticmethod
    def _ptrs(res, keys):
        """the device pointers of res's tensors in the library's argument order, None for a key that is not computed"""
        return [res[k].data_ptr() if k in res else None for k in keys]

    # -- ray-cast range sensors and lidar (include/fsim_rays.h, furniture_amd/rays.py) ---------------------------------------------------
    rays = None

    def set_rays(self, ray_set):
        """Replace the handle's ray set (a furniture_amd.rays.RaySet; None clears it); checked on the host first, then by the library.
        Independent of the cameras: neither needs nor disturbs the other."""
        from .camera import hull_plane_table
        from .rays import RaySet, sensor_table

        def install():
            tab, dirs = sensor_table(self.cm, ray_set)
            planes, adr, num = hull_plane_table(self.cm)
            self._chk(lib().fsim_set_rays(self._h, len(tab), ctypes.addressof(tab), len(dirs), dirs.ctypes.data, len(planes),
                                          planes.ctypes.data if len(planes) else None, adr.ctypes.data, num.ctypes.data))
        self._set_sensors(lib().fsim_set_rays, "rays", ray_set, RaySet, install)

    def ray_shapes(self):
        """{key: (shape, dtype)} of cast_rays' outputs (without the n_envs dimension)"""
        torch = self.torch
        if self.rays is None:
            raise FsimError("ray_shapes: no rays set (FSim.set_rays)")
        r = self.rays.n_rays
        out = {"ray_distance": ((r,), torch.float32), "ray_geom": ((r,), torch.int32)}
        if self.rays.normal:
            out["ray_normal"] = ((r, 3), torch.float32)
        return out

    def sensor_slices(self):
        """{sensor index: slice of the ray dimension of cast_rays' outputs}"""
        if self.rays is None:
            raise FsimError("sensor_slices: no rays set (FSim.set_rays)")
        return self.rays.sensor_slices()

    def cast_rays(self, out=None):
        """Cast every ray of the ray set in every env (include/fsim_rays.h), for the state sync() leaves -> dict of device tensors:
        ray_distance (float32 [n, R], metres along the ray, -1 = nothing hit), ray_geom (int32 [n, R], model geom id as in
        camera_segmentation, -1 = nothing hit) and, when the ray set asks for it, ray_normal (float32 [n, R, 3], the world-frame outward
        unit normal at the hit point, (0, 0, 0) = nothing hit).  out: a dict of such tensors to write into instead of new ones; a key
        that is there alone is cast alone.  Ordered with torch's current stream both ways."""
        if self.rays is None:
            raise FsimError("cast_rays: no rays set (FSim.set_rays)")
        res = self._sensor_outputs("cast_rays", self.ray_shapes(), out)
        self._sensor_call(lib().fsim_cast_rays, *self._ptrs(res, ("ray_distance", "ray_geom", "ray_normal")))
        return res

    # -- signed-distance proximity probes (include/fsim_probes.h, furniture_amd/probes.py) ------------------------------------------------
    probes = None

    def set_probes(self, probe_set):
        """Replace the handle's probe set (a furniture_amd.probes.ProbeSet; None clears it); checked on the host first, then by the
        library.  Independent of the cameras and the rays: needs and disturbs neither."""
        from .camera import hull_plane_table
        from .probes import ProbeSet, sensor_table

        def install():
            tab, pts = sensor_table(self.cm, probe_set)
            planes, adr, num = hull_plane_table(self.cm)
            self._chk(lib().fsim_set_probes(self._h, len(tab), ctypes.addressof(tab), len(pts), pts.ctypes.data, len(planes),
                                            planes.ctypes.data if len(planes) else None, adr.ctypes.data, num.ctypes.data))
        self._set_sensors(lib().fsim_set_probes, "probes", probe_set, ProbeSet, install)

    def probe_shapes(self):
        """{key: (shape, dtype)} of probe_distance's outputs (without the n_envs dimension)"""
        torch = self.torch
        if self.probes is None:
            raise FsimError("probe_shapes: no probes set (FSim.set_probes)")
        p = self.probes.n_probes
        out = {"probe_distance": ((p,), torch.float32), "probe_geom": ((p,), torch.int32)}
        if self.probes.gradient:
            out["probe_gradient"] = ((p, 3), torch.float32)
        return out

    def probe_distance(self, out=None):
        """The signed distance of every probe of the probe set in every env (include/fsim_probes.h), for the state sync() leaves -> dict
        of device tensors: probe_distance (float32 [n, P], metres to the nearest surface, negative inside a solid, dmax = nothing within
        dmax), probe_geom (int32 [n, P], model geom id as in camera_segmentation, -1 = nothing) and, when the probe set asks for it,
        probe_gradient (float32 [n, P, 3], the world-frame unit gradient of the distance, (0, 0, 0) = nothing).  out: a dict of such
        tensors to write into instead of new ones; a key that is there alone is computed alone.  Ordered with torch's current stream
        both ways."""
        if self.probes is None:
            raise FsimError("probe_distance: no probes set (FSim.set_probes)")
        res = self._sensor_outputs("probe_distance", self.probe_shapes(), out)
        self._sensor_call(lib().fsim_probe_distance, *self._ptrs(res, ("probe_distance", "probe_geom", "probe_gradient")))
        return res

    # -- geom-pair distance sensors (include/fsim_pairs.h, furniture_amd/pairs.py) ---------------------------------------------------------
    pairs = None

    def set_pairs(self, pair_set):
        """Replace the handle's pair set (a furniture_amd.pairs.PairSet; None clears it); checked on the host first, then by the
        library.  Independent of the cameras, the rays and the probes: needs and disturbs none of them."""
        from .pairs import PairSet, sensor_table

        def install():
            tab = sensor_table(self.cm, pair_set)
            self._chk(lib().fsim_set_pairs(self._h, len(tab), ctypes.addressof(tab)))
        self._set_sensors(lib().fsim_set_pairs, "pairs", pair_set, PairSet, install)

    def pair_shapes(self):
        """{key: (shape, dtype)} of pair_distance's outputs (without the n_envs dimension)"""
        torch = self.torch
        if self.pairs is None:
            raise FsimError("pair_shapes: no pair set (FSim.set_pairs)")
        k = self.pairs.n_sensors
        out = {"pair_distance": ((k,), torch.float32), "pair_geoms": ((k, 2), torch.int32)}
        if self.pairs.fromto:
            out["pair_fromto"] = ((k, 6), torch.float32)
        if self.pairs.normal:
            out["pair_normal"] = ((k, 3), torch.float32)
        return out

    def pair_distance(self, out=None):
        """The distance of every sensor of the pair set in every env (include/fsim_pairs.h), for the state sync() leaves -> dict of
        device tensors: pair_distance (float32 [n, S], metres between the nearest geoms of the sensor's two sides, negative when they
        overlap, dmax = nothing within dmax), pair_geoms (int32 [n, S, 2], the model geom ids of the two as in camera_segmentation,
        -1 = nothing) and, when the pair set asks for them, pair_fromto (float32 [n, S, 6], the nearest points: on side a, then on side b)
        and pair_normal (float32 [n, S, 3], the unit direction from a to b; (0, 0, 0) = nothing).  out: a dict of such tensors to write
        into instead of new ones; a key that is there alone is computed alone.  Ordered with torch's current stream both ways."""
        if self.pairs is None:
            raise FsimError("pair_distance: no pair set (FSim.set_pairs)")
        res = self._sensor_outputs("pair_distance", self.pair_shapes(), out)
        self._sensor_call(lib().fsim_pair_distance, *self._ptrs(res, ("pair_distance", "pair_geoms", "pair_fromto", "pair_normal")))
        return res

    # -- what-if clearance queries (include/fsim_clearance.h, furniture_amd/clearance.py) -------------------------------------------------
    clearance_set = None

    def set_clearance(self, spec):
        """Replace the handle's clearance set (a furniture_amd.clearance.ClearanceSet; None clears it); checked on the host first, then by
        the library.  Independent of the pair set and of every sensor family: needs and disturbs none of them."""
        from .clearance import ClearanceSet, clearance_tables

        def install():
            dofs, tab, carry = clearance_tables(self.cm, spec)
            self._chk(lib().fsim_set_clearance(self._h, len(dofs), dofs.ctypes.data, len(tab), ctypes.addressof(tab), len(carry) if carry is not None else 0,
                                               ctypes.addressof(carry) if carry is not None else None, spec.max_candidates, spec.scratch_rows))
        self._set_sensors(lib().fsim_set_clearance, "clearance_set", spec, ClearanceSet, install)

    def clearance_shapes(self, K):
        """{key: (shape, dtype)} of clearance's outputs for K candidates per env (without the n_envs dimension)"""
        if self.clearance_set is None:
            raise FsimError("clearance_shapes: no clearance set (FSim.set_clearance)")
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= self.clearance_set.max_candidates:
            raise ValueError("clearance: K = %r candidates (1 .. max_candidates = %d)" % (K, self.clearance_set.max_candidates))
        return {k: (sh, getattr(self.torch, dt)) for k, (sh, dt) in self.clearance_set.shapes(int(K)).items()}

    def clearance(self, cand, carry_mask=None, out=None):
        """The clearance of K candidate configurations per env (include/fsim_clearance.h), for the state sync() leaves.  cand: a contiguous
        float32 device tensor [n, K, D], D the dofs of the clearance set in its order; carry_mask: None (nothing is carried) or a
        contiguous uint8 device tensor [n], bit r = carry rule r -> dict of device tensors: clearance_distance (float32 [n, K, S]),
        clearance_geoms (int32 [n, K, S, 2]), clearance_valid (uint8 [n, K], 0 = the candidate held a value that is not finite, and the
        env's own value stood in for it) and, when the set asks for them, clearance_fromto (float32 [n, K, S, 6]) and clearance_normal
        (float32 [n, K, S, 3]), each what pair_distance would give with the set's sensors if the env's qpos held the candidate.  Writes
        no state.  out: a dict of such tensors to write into instead of new ones; a key that is there alone is computed alone (at least
        one besides clearance_valid).  Ordered with torch's current stream both ways."""
        torch = self.torch
        spec = self.clearance_set
        if spec is None:
            raise FsimError("clearance: no clearance set (FSim.set_clearance)")
        if not isinstance(cand, torch.Tensor) or cand.dtype != torch.float32 or cand.dim() != 3 or cand.shape[0] != self.n_envs or cand.shape[2] != spec.n_dofs \
                or not cand.is_contiguous() or cand.device != self.device:
            raise ValueError("clearance: cand is not a contiguous float32 tensor of shape (%d, K, %d) on %s" % (self.n_envs, spec.n_dofs, self.device))
        K = int(cand.shape[1])
        if carry_mask is not None and (not isinstance(carry_mask, torch.Tensor) or carry_mask.dtype != torch.uint8 or tuple(carry_mask.shape) != (self.n_envs,)
                                       or not carry_mask.is_contiguous() or carry_mask.device != self.device):
            raise ValueError("clearance: carry_mask is not a contiguous uint8 tensor of shape (%d,) on %s" % (self.n_envs, self.device))
        res = self._sensor_outputs("clearance", self.clearance_shapes(K), out)
        if all(k == "clearance_valid" for k in res):
            raise ValueError("clearance: out holds clearance_valid alone (at least one of the distance, geoms, fromto and normal outputs)")
        self._sensor_call(lib().fsim_clearance, K, cand.data_ptr(), carry_mask.data_ptr() if carry_mask is not None else None,
                          *self._ptrs(res, ("clearance_distance", "clearance_geoms", "clearance_fromto", "clearance_normal", "clearance_valid")))
        return res

    # -- body and site frame sensors with their Jacobians (include/fsim_frames.h, furniture_amd/frames.py) --------------------------------
    frames = None

    def set_frames(self, frame_set):
        """Replace the handle's frame set (a furniture_amd.frames.FrameSet; None clears it); checked on the host first, then by the
        library.  Independent of the cameras, the rays, the probes and the pairs: needs and disturbs none of them."""
        from .frames import FrameSet, sensor_table

        def install():
            tab = sensor_table(self.cm, frame_set)
            self._chk(lib().fsim_set_frames(self._h, len(tab), ctypes.addressof(tab)))
        self._set_sensors(lib().fsim_set_frames, "frames", frame_set, FrameSet, install)

    def frame_shapes(self):
        """{key: (shape, dtype)} of frame_state's outputs (without the n_envs dimension)"""
        torch = self.torch
        if self.frames is None:
            raise FsimError("frame_shapes: no frame set (FSim.set_frames)")
        k = self.frames.n_sensors
        out = {"frame_pos": ((k, 3), torch.float32), "frame_quat": ((k, 4), torch.float32)}
        if self.frames.velocity:
            out["frame_vel"] = ((k, 6), torch.float32)
        if self.frames.jacobian:
            out["frame_jac"] = ((k, 6, self.cm.nv), torch.float32)
        return out

    def frame_state(self, out=None):
        """The state of every sensor of the frame set in every env (include/fsim_frames.h), for the state sync() leaves -> dict of device
        tensors: frame_pos (float32 [n, S, 3], the frame's origin in its reference frame, metres), frame_quat (float32 [n, S, 4], wxyz,
        its orientation in the reference frame) and, when the frame set asks for them, frame_vel (float32 [n, S, 6], the time derivative
        of frame_pos and the relative angular velocity, in the reference frame) and frame_jac (float32 [n, S, 6, nv], frame_vel =
        frame_jac @ qvel).  out: a dict of such tensors to write into instead of new ones; a key that is there alone is computed alone.
        Ordered with torch's current stream both ways."""
        if self.frames is None:
            raise FsimError("frame_state: no frame set (FSim.set_frames)")
        res = self._sensor_outputs("frame_state", self.frame_shapes(), out)
        self._sensor_call(lib().fsim_frame_state, *self._ptrs(res, ("frame_pos", "frame_quat", "frame_vel", "frame_jac")))
        return res

    # -- mass-matrix, inverse-inertia and bias-force tensors (include/fsim_dynamics.h, furniture_amd/dynamics.py) -------------------------
    dyn = None

    def set_dynamics(self, spec):
        """Replace the handle's dynamics selection (a furniture_amd.dynamics.Dynamics; None clears it); checked on the host first, then
        by the library.  Independent of the cameras, the rays, the probes, the pairs and the frames: needs and disturbs none of them."""
        from .dynamics import Dynamics, dof_table

        def install():
            tab = dof_table(self.cm, spec)
            self._chk(lib().fsim_set_dynamics(self._h, len(tab), tab.ctypes.data))
            self._dyn_k = len(tab)
        self._set_sensors(lib().fsim_set_dynamics, "dyn", spec, Dynamics, install)

    def dynamics_shapes(self):
        """{key: (shape, dtype)} of dynamics' outputs (without the n_envs dimension)"""
        torch = self.torch
        if self.dyn is None:
            raise FsimError("dynamics_shapes: no dof selection (FSim.set_dynamics)")
        k = self._dyn_k
        shapes = dict(dyn_mass=(k, k), dyn_minv=(k, k), dyn_bias=(k,), dyn_gravity=(k,))
        return {key: (shapes[key], torch.float32) for key in self.dyn.keys()}

    def dynamics(self, out=None):
        """The dynamics tensors of every env (include/fsim_dynamics.h), for the state sync() leaves -> dict of device tensors, those the
        Dynamics asks for: dyn_mass (float32 [n, K, K], M[dofs][:, dofs]), dyn_minv (float32 [n, K, K], the inverse of the whole M
        restricted to dofs), dyn_bias (float32 [n, K], qfrc_bias[dofs]) and dyn_gravity (float32 [n, K], the same at qvel = 0).  out: a
        dict of such tensors to write into instead of new ones; a key that is there alone is computed alone.  Ordered with torch's
        current stream both ways."""
        if self.dyn is None:
            raise FsimError("dynamics: no dof selection (FSim.set_dynamics)")
        res = self._sensor_outputs("dynamics", self.dynamics_shapes(), out)
        self._sensor_call(lib().fsim_dynamics, *self._ptrs(res, ("dyn_mass", "dyn_minv", "dyn_bias", "dyn_gravity")))
        return res

    # -- contact-force and touch sensors (include/fsim_contacts.h, furniture_amd/contacts.py) -------------------------------------------
    contacts = None

    def set_contacts(self, contact_set):
        """Replace the handle's contact sensors (a furniture_amd.contacts.ContactSet; None clears them); checked on the host first, then
        by the library.  Independent of the cameras, the rays, the probes, the pairs, the frames and the dynamics tensors."""
        from .contacts import MAX_SLOTS, ContactSet, sensor_table

        def install():
            if self.max_contacts > MAX_SLOTS:
                raise ValueError("contacts: the handle has %d contact slots (the contact-force pass serves at most %d)" % (self.max_contacts, MAX_SLOTS))
            tab = sensor_table(self.cm, contact_set)
            self._chk(lib().fsim_set_contacts(self._h, len(tab), ctypes.cast(tab, ctypes.c_void_p)))
        self._set_sensors(lib().fsim_set_contacts, "contacts", contact_set, ContactSet, install)

    def contact_shapes(self):
        """{key: (shape, dtype)} of contact_forces' outputs (without the n_envs dimension)"""
        torch = self.torch
        if self.contacts is None:
            raise FsimError("contact_shapes: no sensor set (FSim.set_contacts)")
        s, c, f, i = self.contacts.n_sensors, self.max_contacts, torch.float32, torch.int32
        shapes = dict(contact_force=((s, 3), f), contact_touch=((s,), f), contact_count=((s,), i), contact_status=((), i),
                      con_geoms=((c, 2), i), con_pos=((c, 3), f), con_normal=((c, 3), f), con_dist=((c,), f), con_force=((c, 3), f), con_fn=((c,), f))
        return {key: shapes[key] for key in self.contacts.keys()}

    def contact_forces(self, out=None):
        """The contact forces of every env (include/fsim_contacts.h), for the state sync() leaves -> dict of device tensors:
        contact_force (float32 [n, S, 3], the net world force side b exerts on side a), contact_touch (float32 [n, S], the sum of the
        normal forces), contact_count (int32 [n, S], listed contacts), contact_status (int32 [n], bit 0 contacts dropped, bit 1 solve not
        to be trusted) and, with the set's contacts=True, con_geoms (int32 [n, C, 2]), con_pos, con_normal, con_force (float32 [n, C, 3]),
        con_dist and con_fn (float32 [n, C]).  out: a dict of such tensors to write into instead of new ones; a key that is there alone
        is computed alone.  Reads the env records and writes nothing else.  Ordered with torch's current stream both ways."""
        if self.contacts is None:
            raise FsimError("contact_forces: no sensor set (FSim.set_contacts)")
        res = self._sensor_outputs("contact_forces", self.contact_shapes(), out)
        keys = [f if f.startswith("con_") else "contact_" + f for f in CONTACT_OUT_FIELDS]
        self._sensor_call(lib().fsim_contact_forces, ctypes.byref(FsimContactOut(*self._ptrs(res, keys))))
        return res

    # -- force-torque, accelerometer and joint-load sensors (include/fsim_wrench.h, furniture_amd/wrench.py) ------------------------------
    wrench_set = None

    def set_wrenches(self, wrench_set):
        """Replace the handle's wrench sensors (a furniture_amd.wrench.WrenchSet; None clears them); checked on the host first, then by the
        library.  Independent of every other sensor family."""
        from .wrench import MAX_SLOTS, WrenchSet, sensor_table

        def install():
            if self.max_contacts > MAX_SLOTS:
                raise ValueError("wrenches: the handle has %d contact slots (the wrench pass serves at most %d)" % (self.max_contacts, MAX_SLOTS))
            tab = sensor_table(self.cm, wrench_set)
            self._chk(lib().fsim_set_wrenches(self._h, len(tab), ctypes.cast(tab, ctypes.c_void_p)))
        self._set_sensors(lib().fsim_set_wrenches, "wrench_set", wrench_set, WrenchSet, install)

    def wrench_shapes(self):
        """{key: (shape, dtype)} of wrenches' outputs (without the n_envs dimension)"""
        torch = self.torch
        if self.wrench_set is None:
            raise FsimError("wrench_shapes: no sensor set (FSim.set_wrenches)")
        s, f, i = self.wrench_set.n_sensors, torch.float32, torch.int32
        shapes = dict(wrench_force=((s, 3), f), wrench_torque=((s, 3), f), wrench_accel=((s, 3), f), wrench_angacc=((s, 3), f),
                      wrench_external=((s, 6), f), wrench_qacc=((self.nv,), f), wrench_qfrc_constraint=((self.nv,), f), wrench_status=((), i))
        return {key: shapes[key] for key in self.wrench_set.keys()}

    def wrenches(self, out=None):
        """The wrench sensors of every env (include/fsim_wrench.h), for the state sync() leaves -> dict of device tensors: wrench_force,
        wrench_torque, wrench_accel, wrench_angacc (float32 [n, S, 3], sensor frame), wrench_status (int32 [n]) and, with the set's
        external=True, wrench_external (float32 [n, S, 6], world frame), with joint=True wrench_qacc and wrench_qfrc_constraint (float32
        [n, nv]).  out: a dict of such tensors to write into instead of new ones; a key that is there alone is computed alone.  Reads the
        env records and writes nothing else.  Ordered with torch's current stream both ways."""
        if self.wrench_set is None:
            raise FsimError("wrenches: no sensor set (FSim.set_wrenches)")
        res = self._sensor_outputs("wrenches", self.wrench_shapes(), out)
        self._sensor_call(lib().fsim_wrenches, ctypes.byref(FsimWrenchOut(*self._ptrs(res, ["wrench_" + f for f in WRENCH_OUT_FIELDS]))))
        return res

    # -- centre-of-mass, momentum and energy sensors (include/fsim_momentum.h, furniture_amd/momentum.py) --------------------------------
    momenta_set = None

    def set_momenta(self, momentum_set):
        """Replace the handle's momentum sensors (a furniture_amd.momentum.MomentumSet; None clears them); checked on the host first, then
        by the library.  Independent of the cameras and of every other sensor family."""
        from .momentum import MomentumSet, sensor_table

        def install():
            adr, bodies, subtree = sensor_table(self.cm, momentum_set)
            self._chk(lib().fsim_set_momenta(self._h, len(adr) - 1, adr.ctypes.data, bodies.ctypes.data, subtree.ctypes.data))
        self._set_sensors(lib().fsim_set_momenta, "momenta_set", momentum_set, MomentumSet, install)

    def momentum_shapes(self):
        """{key: (shape, dtype)} of momenta's outputs (without the n_envs dimension)"""
        torch = self.torch
        if self.momenta_set is None:
            raise FsimError("momentum_shapes: no sensor set (FSim.set_momenta)")
        s, f = self.momenta_set.n_sensors, torch.float32
        shapes = dict(mom_com=((s, 3), f), mom_linvel=((s, 3), f), mom_angmom=((s, 3), f), mom_jac=((s, 3, self.nv), f), mom_energy=((2,), f))
        return {key: shapes[key] for key in self.momenta_set.keys()}

    def momenta(self, out=None):
        """The momentum sensors of every env (include/fsim_momentum.h), for the state sync() leaves -> dict of device tensors: mom_com,
        mom_linvel, mom_angmom (float32 [n, S, 3], world frame) and, with the set's jacobian=True, mom_jac (float32 [n, S, 3, nv]), with
        energy=True mom_energy (float32 [n, 2], potential then kinetic).  out: a dict of tensors to write into, whose keys alone are
        computed.  One launch on the handle's stream; reads the env records, writes nothing but the outputs."""
        if self.momenta_set is None:
            raise FsimError("momenta: no sensor set (FSim.set_momenta)")
        res = self._sensor_outputs("momenta", self.momentum_shapes(), out)
        self._sensor_call(lib().fsim_momenta, ctypes.byref(FsimMomentumOut(*self._ptrs(res, ["mom_" + f for f in MOMENTUM_OUT_FIELDS]))))
        return res

    def kernel_time_ms(self):
        ms, n = ctypes.c_double(), ctypes.c_int32()
        self._chk(lib().fsim_kernel_time_ms(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def close(self):
        if getattr(self, "_h", None):
            lib().fsim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
