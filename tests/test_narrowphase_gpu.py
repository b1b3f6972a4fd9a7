"""The collision narrow phase of the device (furniture_amd/csrc/fsim_collide.hpp), pair by pair: its own templates, compiled into the test
tool tests/narrowphase_probe.hip and called with a recording emitter, one lane per case, one launch per pair type.

 - against the fp64 checker's osim_narrowphase: the same contact count wherever the fp32 control build of the checker has the fp64 count;
   contacts matched by nearest position (the device builds the box-box manifold in another order); dist, normal and position within a
   multiple of what fp32 arithmetic alone does to the checker (tests/test_narrowphase.py, part (c)): 8 x for the closed-form types (the device
   contracts to FMA and orders np_plane_box / np_box_box differently; floor: 16 ulp of 1 m), 4 x for the portal pairs (dist and normal only:
   their position, like the vertices np_plane_mesh picks, is checked by containment);
 - against the independent reference, with the assertions the checker itself has to meet (test_narrowphase.check_against_reference);
 - the early-outs of fs_collide (np_capsule_gap, np_cyl_cyl_separated, np_cyl_box_separated, stage 2 of the broadphase: fs_stage2_near)
   never reject a pair that touches.  What they reject among the pairs that do not touch is printed, not asserted."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import narrowphase_cases as nc
from tests import test_narrowphase as T
from tests.collide_reference import MESH

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_MAXC, NP_CASEW, NP_CONW = 16, 36, 8


def _tool():
    """tests/libnarrowphase_probe.so: built by __graft_entry__.build(); compiled on the spot (hipcc, a few seconds, the library's own flags) in a
    tree that does not have it or has an older one than its source or the headers it includes"""
    from tests import narrowphase_tool
    if narrowphase_tool.stale():
        subprocess.check_call(narrowphase_tool.probe_command())
    L = ctypes.CDLL(narrowphase_tool.LIBRARY)
    L.np_probe_contacts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.np_probe_pretests.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.np_probe_maxcon.argtypes = [ctypes.c_void_p]
    return L


def pack(sets):
    """the case records of narrowphase_probe.hip for a list of case sets, concatenated"""
    rec, typ = [], []
    for cs in sets:
        A, B, n = cs["A"], cs["B"], len(cs["A"])
        rec.append(np.concatenate([A.pos, A.R.reshape(n, 9), A.size, B.pos, B.R.reshape(n, 9), B.size, cs["margin"][:, None], nc.rbound(A)[:, None], nc.rbound(B)[:, None],
                                   np.zeros((n, NP_CASEW - 33))], axis=1))
        typ.append(np.tile(np.array([cs["pt"], cs["t1"], cs["t2"]], dtype=np.int32), (n, 1)))
    return np.ascontiguousarray(np.concatenate(rec), dtype=np.float32), np.ascontiguousarray(np.concatenate(typ), dtype=np.int32)


def device_contacts(tool, sets, mesh=1):
    """one launch (mesh: np_mpr<., true>, the generic kernels' / np_mpr<., false>, the specialised kernels') -> per set (count (N,), contacts (N, 16, 7) float64 in the checker's layout, inactive slots dropped)"""
    rec, typ = pack(sets)
    n = len(rec)
    verts = np.ascontiguousarray(nc.hull_vertices(), dtype=np.float32) if any(MESH in (cs["t1"], cs["t2"]) for cs in sets) else np.zeros((0, 3), dtype=np.float32)
    out, cnt = np.zeros((n, NP_MAXC, NP_CONW), dtype=np.float32), np.zeros(n, dtype=np.int32)
    rc = tool.np_probe_contacts(rec.ctypes.data, typ.ctypes.data, n, verts.ctypes.data if len(verts) else None, len(verts), out.ctypes.data, cnt.ctypes.data, mesh)
    assert rc == 0, "np_probe_contacts: HIP error %d" % rc
    assert cnt.min() >= 0
    con, num = np.zeros((n, NP_MAXC, 7)), np.zeros(n, dtype=np.int32)
    for i in np.nonzero(cnt > 0)[0]:
        live = out[i, :cnt[i]][out[i, :cnt[i], 0] > 0.5]
        num[i] = len(live)
        con[i, :len(live)] = live[:, 1:]
    res, i0 = [], 0
    for cs in sets:
        res.append((num[i0:i0 + len(cs["A"])], con[i0:i0 + len(cs["A"])]))
        i0 += len(cs["A"])
    return res


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.mark.parametrize("name", list(nc.KINDS))
def test_device_pairs_match_the_checker_and_the_reference(name, tool):
    pt, t1, t2, portal, modes = nc.KINDS[name]
    sets = [nc.case_set(name, mode) for mode in modes]
    by_position = not portal and name != "plane_mesh"
    if portal:
        tol_d, tol_n, tol_p = max(4 * T.FP32_DIST_PORTAL, T.ULP16), max(4 * T.FP32_NORMAL_PORTAL, T.ULP16), None
    else:
        tol_d, tol_n, tol_p = max(8 * T.FP32_DIST_CLOSED, T.ULP16), max(8 * T.FP32_NORMAL_CLOSED, T.ULP16), max(8 * T.FP32_POS_CLOSED, T.ULP16)
    # the portal routine exists twice: np_mpr<., true> in the generic kernels, np_mpr<., false> in the kernels specialised for one model
    for mesh in ((1, 0) if portal and MESH not in (t1, t2) else (1,)):
        for cs, (cnt, con) in zip(sets, device_contacts(tool, sets, mesh)):
            where = "%s/%s%s" % (name, cs["mode"], "" if mesh else " (np_mpr without the hull branch)")
            c64, k64 = T.checker(cs)
            c32, _ = T.checker(cs, np.float32)
            same = c32 == c64
            bad = np.nonzero(same & (cnt != c64))[0]
            assert len(bad) == 0, "%s: contact count differs from the fp64 checker at cases %s: device %s, checker %s" % (where, bad[:8], cnt[bad[:8]], c64[bad[:8]])
            dev, _ = T.compare_builds(cs, np.where(same, c64, 0), k64, np.where(same, cnt, 0), con)
            print("%s: device vs fp64 checker: dist %.3e (allowed %.3e) normal %.3e (%.3e) position %.3e (%s); fp32 control count differs in %d cases"
                  % (where, dev[0], tol_d, dev[1], tol_n, dev[2], "%.3e" % tol_p if by_position else "by containment", int((~same).sum())))
            assert dev[0] <= tol_d and dev[1] <= tol_n, (where, dev)
            if by_position:
                assert dev[2] <= tol_p, (where, dev)
            # the independent reference: what the checker has to meet on the same set, widened by the device bound above; positions get a
            # geometric tolerance only
            ref = T.REF_GAP_ERR + T.REF_SAMPLING_ERR + tol_d
            lo = (T.PORTAL_OVER_FP64[name, cs["mode"]] if portal else T.CHECKER_GAP_ERR) + ref + (T.box_box_slack(cs["gap"]) if name == "box_box" else 0.0)
            o, u = T.check_against_reference(cs, cnt, con, lo, (T.PORTAL_UNDER_FP64 if portal else T.CHECKER_GAP_ERR) + ref, max(8 * T.FP32_POS_CLOSED, T.ULP16), "device")
            print("%s: device deepest dist below the true gap by at most %.3e, above it by at most %.3e" % (where, o, u))


def test_device_maxcon_table_is_the_one_the_tests_use(tool):
    tab = np.zeros(12, dtype=np.int32)
    assert tool.np_probe_maxcon(tab.ctypes.data) == 0 and tab.tolist() == T.FS_PAIR_MAXCON


def test_early_outs_never_reject_a_touching_pair(tool):
    sets = [nc.case_set(name, mode) for name, mode in nc.all_sets()]
    rec, typ = pack(sets)
    n = len(rec)
    verdict, capgap = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
    rc = tool.np_probe_pretests(rec.ctypes.data, typ.ctypes.data, n, verdict.ctypes.data, capgap.ctypes.data)
    assert rc == 0, "np_probe_pretests: HIP error %d" % rc
    touch = np.concatenate([cs["touch"] for cs in sets])
    margin = np.concatenate([cs["margin"] for cs in sets])
    label = np.concatenate([np.full(len(cs["A"]), i) for i, cs in enumerate(sets)])
    names = {1: "np_capsule_gap", 2: "np_cyl_cyl_separated", 4: "np_cyl_box_separated", 8: "stage 2 of the broadphase"}
    for bit, what in names.items():
        applies = np.isin(typ[:, 0], {1: (8,), 2: (8,), 4: (7,), 8: tuple(range(12))}[bit]) & (typ[:, 1] != 0 if bit == 8 else True)
        bad = np.nonzero(applies & touch & ((verdict & bit) != 0))[0]
        assert len(bad) == 0, "%s says 'separated' for touching pairs: %s" % (what, [(sets[label[i]]["name"], sets[label[i]]["mode"], int(i)) for i in bad[:6]])
        far = applies & ~touch
        print("%s rejects %d of %d pairs that do not touch (%.1f %%)" % (what, int(((verdict & bit) != 0)[far].sum()), int(far.sum()), 100.0 * ((verdict & bit) != 0)[far].mean() if far.any() else 0.0))
    cc = (typ[:, 0] == 8) & touch
    assert (capgap[cc] <= margin[cc]).all(), "np_capsule_gap - r1 - r2 exceeds the margin on touching cylinders: %s" % capgap[cc][capgap[cc] > margin[cc]][:6]
