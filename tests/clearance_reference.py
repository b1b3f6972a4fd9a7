"""float64 reference of the clearance queries (include/fsim_clearance.h): the oracle's state is set to the candidate, carried parts are
placed by the header's formula X_part' = X_carrier(candidate) o X_carrier(record)^-1 o X_part(record) in float64, the colliding geoms come
from the oracle and the gaps from tests/collide_reference.py, as tests/test_pairs_gpu._reference_gaps takes them.

Its own check (check_carry_is_rigid): under carry the gap between the carrier's geoms and the part's geoms is the same for every
candidate to 1e-9 -- the part moves rigidly with the carrier."""
import numpy as np

from tests import camera_reference as cref
from tests import collide_reference as cr


def dof_addresses(m, dofs):
    """the qpos address of each listed dof"""
    return np.asarray(m.arrays["dof_qposadr"]).astype(np.int64)[np.asarray(dofs, dtype=np.int64)]


def candidate_qpos(m, qpos, dofs, cand):
    """the env's qpos (float64 [nq]) with the candidate's finite values at the listed dofs -> (qpos, valid)"""
    q = np.asarray(qpos, dtype=np.float64).copy()
    c = np.asarray(cand, dtype=np.float64)
    ok = np.isfinite(c)
    q[dof_addresses(m, dofs)[ok]] = c[ok]
    return q, bool(ok.all())


def _body_pose(osim, b):
    return np.array(osim.data.xpos[b], dtype=np.float64), np.array(osim.data.xmat[b], dtype=np.float64).reshape(3, 3)


def carried_geoms(m, part):
    """[ncg] bool: the colliding geoms that move with the part named ``part`` (those folded into its reduced body)"""
    A = m.arrays
    red = np.asarray(A["body_red"]).astype(np.int64)
    gbody = np.asarray(A["geom_bodyid"]).astype(np.int64)[np.asarray(A["cg_orig"]).astype(np.int64)]
    return red[gbody] == red[m.meta["body_names"].index(part)]


def geoms_at(osim, m, qpos, dofs, cand, carry=()):
    """the colliding geoms (tests.camera_reference.model_geoms, hull vertices attached) of one env at one candidate.  qpos: the env's
    record, float64 [nq]; carry: the (part name, carrier body name) rules whose mask bit is set."""
    names = m.meta["body_names"]
    before = {}
    if carry:
        osim.data.qpos[:] = qpos
        osim.forward()
        before = {c: _body_pose(osim, names.index(c)) for _, c in carry}
    q, _ = candidate_qpos(m, qpos, dofs, cand)
    osim.data.qpos[:] = q
    osim.forward()
    geoms = cref.model_geoms(m, np.array(osim.data.geom_xpos, dtype=np.float64), np.array(osim.data.geom_xmat, dtype=np.float64))  # (copies: the oracle's arrays move on)
    for part, carrier in carry:
        p0, R0 = before[carrier]
        p1, R1 = _body_pose(osim, names.index(carrier))
        RT = R1 @ R0.T  # X_carrier(candidate) o X_carrier(record)^-1, a world transform: the part's geoms are at their record poses
        pT = p1 - RT @ p0
        for k in np.nonzero(carried_geoms(m, part))[0]:
            g = geoms[int(k)]
            g["pos"], g["mat"] = RT @ g["pos"] + pT, RT @ g["mat"]
    A = m.arrays
    for g in geoms:
        if g["type"] == cr.MESH:
            a, n = int(A["geom_meshadr"][g["id"]]), int(A["geom_meshnum"][g["id"]])
            g["verts"] = np.asarray(A["mesh_vert"], dtype=np.float64).reshape(-1, 3)[a:a + n]
    return geoms


def check_carry_is_rigid(m, gaps_of, geoms_per_candidate, part, carrier, tol=1e-9):
    """gaps_of(geoms, pairs) -> {(g1, g2): gap} (tests.test_pairs_gpu._reference_gaps).  Over the candidates' geom lists, the gap of every
    (carrier geom, part geom) pair is constant within tol -> the largest spread."""
    A = m.arrays
    red = np.asarray(A["body_red"]).astype(np.int64)
    gbody = np.asarray(A["geom_bodyid"]).astype(np.int64)[np.asarray(A["cg_orig"]).astype(np.int64)]
    cb = m.meta["body_names"].index(carrier)
    on_c = np.nonzero(gbody == cb if red[cb] == 0 else red[gbody] == red[cb])[0]
    on_p = np.nonzero(carried_geoms(m, part))[0]
    pairs = [(int(a), int(b)) for a in on_c for b in on_p]
    assert pairs, "the carrier %r or the part %r has no colliding geom" % (carrier, part)
    rows = np.array([[gaps_of(geoms, pairs)[p] for p in pairs] for geoms in geoms_per_candidate])
    spread = float((rows.max(0) - rows.min(0)).max())
    assert spread <= tol, "carried part %r moves against its carrier %r: the gaps vary by %.3e over the candidates" % (part, carrier, spread)
    return spread


def composition_error_fp32(osim, m, qpos, dofs, cands, carry):
    """The carried-pose composition restated in numpy float32 from float64 body poses rounded to float32, against the float64 one ->
    the largest displacement (metres) it gives any carried geom's position over the candidates.  Quaternion form, as on the device."""
    names = m.meta["body_names"]
    f = np.float32

    def qmul(a, b):
        return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], dtype=a.dtype)

    def qrot(q, v):
        u = q[1:]
        t = (2 * np.cross(u, v)).astype(q.dtype)
        return (v + q[0] * t + np.cross(u, t)).astype(q.dtype)

    def conj(q):
        return np.array([q[0], -q[1], -q[2], -q[3]], dtype=q.dtype)

    def pose(b, dt):
        return np.array(osim.data.xpos[b], dtype=dt), np.array(osim.data.xquat[b], dtype=dt)

    def compose(pc0, qc0, pp0, qp0, pc1, qc1):
        qi = conj(qc0)
        prel, qrel = qrot(qi, pp0 - pc0), qmul(qi, qp0)
        p, q = pc1 + qrot(qc1, prel), qmul(qc1, qrel)
        return p, (q / np.sqrt((q * q).sum(dtype=q.dtype))).astype(q.dtype)
    worst = 0.0
    A = m.arrays
    gbody = np.asarray(A["geom_bodyid"]).astype(np.int64)[np.asarray(A["cg_orig"]).astype(np.int64)]
    for part, carrier in carry:
        pb, cb = names.index(part), names.index(carrier)
        osim.data.qpos[:] = qpos
        osim.forward()
        rec = {dt: pose(cb, dt) + pose(pb, dt) for dt in (np.float64, f)}
        # the part's geoms in the part's frame (float64), from the record
        pp, qp = rec[np.float64][2], rec[np.float64][3]
        local = [qrot(conj(qp), np.array(osim.data.geom_xpos[int(A["cg_orig"][k])], dtype=np.float64) - pp) for k in np.nonzero(carried_geoms(m, part))[0]]
        for cand in cands:
            q, _ = candidate_qpos(m, qpos, dofs, cand)
            osim.data.qpos[:] = q
            osim.forward()
            out = {dt: compose(*rec[dt], *pose(cb, dt)) for dt in (np.float64, f)}
            for loc in local:
                a = out[np.float64][0] + qrot(out[np.float64][1], loc)
                b = out[f][0].astype(np.float64) + qrot(out[f][1].astype(np.float64), loc)
                worst = max(worst, float(np.linalg.norm(a - b)))
    return worst
