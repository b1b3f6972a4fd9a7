"""Can the stored states tell?  Ten deliberate defects of the contact rows (the issue's nine, and the gap of a pair left out of its includemargin), each put into a scratch copy of the checker's float32 build
(oracle/fsim_oracle.c with real = float: the arithmetic of the device), and what each does to the measures of tests/conerows_reference.py on the
states of tests/golden/cone_states.npz -- and, for the record of DESIGN.md 26, on the 19 older cases of solve_states.npz and row_states.npz.

CPU only.  tests/test_conerows.py::test_the_states_can_tell builds the variants in a temporary directory and asserts that every defect moves some
new case past DEFECT_FLOORS x its fp32 floor; run as a script, this prints both tables."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle_sim import OracleSim  # noqa: E402
from tests import conerows_reference as cr  # noqa: E402
from tests import rows_reference as rref  # noqa: E402
from tests import solve_reference as sref  # noqa: E402

DEFECT_FLOORS = 100.0
SOURCES = ("fsim_oracle.c", "fsim_oracle.h", "fsim_oracle_collide.inc", "fsim_oracle_solve.inc")
PTVEL = """      finish_row(s, r, k->solref, k->solimp, dA, a > 0);
      { /* DEFECT: geom 2's side of the relative velocity taken at its body's centre of mass, not at the contact point */
        int idx2[MAXNNZ]; real J2[MAXNNZ], kk, bb, jv = 0, jv2 = 0;
        int n2 = jac_point_sparse(s, b2, s->xipos + 3 * b2, k->frame + 3 * a, 1.0, idx2, J2, 0);
        n2 = jac_point_sparse(s, b1, k->pos, k->frame + 3 * a, -1.0, idx2, J2, n2);
        impedance_k_b(k->solref, k->solimp, r->pos - r->margin, m->timestep, &kk, &bb);
        for (int i = 0; i < r->nnz; i++) jv += r->J[i] * s->qvel[r->idx[i]];
        for (int i = 0; i < n2; i++) jv2 += J2[i] * s->qvel[idx2[i]];
        r->aref += bb * (jv - jv2);
      }
"""
# name -> (file, the text that is replaced, what replaces it); every text occurs exactly once
DEFECTS = {
    "upper branch of the impedance = the lower one, for contacts": (
        "fsim_oracle_solve.inc", "  if (is_friction) k = 0;\n",
        "  if (is_friction) k = 0;\n  if (r->type == C_CONTACT) { real x = fabs(r->pos - r->margin) / solimp[2];\n"
        "    if (x < 1 && x > solimp[3]) imp = solimp[0] + pow(x, solimp[4]) / pow(solimp[3], solimp[4] - 1) * (solimp[1] - solimp[0]); }\n"),
    "normal velocity term dropped from aref": (
        "fsim_oracle_solve.inc", "  r->aref = -b * jv - k * imp * (r->pos - r->margin);", "  if (r->type == C_CONTACT && !is_friction) jv = 0;\n  r->aref = -b * jv - k * imp * (r->pos - r->margin);"),
    "tangential velocity terms dropped from aref": (
        "fsim_oracle_solve.inc", "  r->aref = -b * jv - k * imp * (r->pos - r->margin);", "  if (is_friction) jv = 0;\n  r->aref = -b * jv - k * imp * (r->pos - r->margin);"),
    "lever arm of the point velocity dropped on geom 2's side": ("fsim_oracle_solve.inc", "      finish_row(s, r, k->solref, k->solimp, dA, a > 0);\n", PTVEL),
    "solref taken from geom 1 alone": (
        "fsim_oracle_collide.inc", "k->solref[i] = mix * m->geom_solref[2 * g1 + i] + (1 - mix) * m->geom_solref[2 * g2 + i];", "k->solref[i] = m->geom_solref[2 * g1 + i];"),
    "friction taken as the minimum of the pair": ("fsim_oracle_collide.inc", "k->mu = f1 > f2 ? f1 : f2;", "k->mu = f1 < f2 ? f1 : f2;"),
    "R_t = R_n (impratio ignored)": ("fsim_oracle_solve.inc", "r->R = rn->R / ir;", "r->R = rn->R; (void)ir;"),
    "dist used in place of dist - includemargin": ("fsim_oracle_solve.inc", "r->margin = a == 0 ? k->includemargin : 0.0;", "r->margin = 0.0;"),
    "gap left out of includemargin = margin - gap": ("fsim_oracle_collide.inc", "k->includemargin = margin - gap;", "k->includemargin = margin; (void)gap;"),
    "the 2 * timestep clamp dropped": ("fsim_oracle_solve.inc", "    if (tc < 2 * timestep) tc = 2 * timestep; /* refsafe */\n", ""),
}


def build(tmp):
    """{defect name: path of a float32 build of oracle/fsim_oracle.c with the defect} (and None: the source as it is), compiled side by side"""
    jobs = {}
    for k, name in enumerate([None] + list(DEFECTS)):
        d = os.path.join(str(tmp), "v%d" % k)
        os.makedirs(d)
        for f in SOURCES:
            shutil.copy(os.path.join(ROOT, "oracle", f), d)
        if name is not None:
            f, old, new = DEFECTS[name]
            with open(os.path.join(d, f)) as fh:
                text = fh.read()
            assert text.count(old) == 1, (name, text.count(old))
            with open(os.path.join(d, f), "w") as fh:
                fh.write(text.replace(old, new))
        jobs[name] = (d, [os.environ.get("CC", "gcc"), "-O1", "-fPIC", "-std=c11", "-w", "-DOSIM_REAL=float", "-fsingle-precision-constant", "-ffp-contract=off",
                          "-shared", "-o", os.path.join(d, "libosim32.so"), os.path.join(d, "fsim_oracle.c"), "-lm"])
    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1, 16)) as pool:
        list(pool.map(lambda j: subprocess.check_call(j[1]), jobs.values()))
    return {name: os.path.join(d, "libosim32.so") for name, (d, _) in jobs.items()}


def measures(path, stored, model, refs, grp):
    """the largest force / island / row (and, where the build lists the reference's contacts, fn / cforce) of the float32 build at `path` over the
    states of a case, cold start, against the float64 references"""
    worst = dict.fromkeys(("force", "island", "row") + cr.CONTACT_MEASURES, 0.0)
    o = OracleSim(model, np.float32, lib_path=path)
    for e, ref in enumerate(refs):
        sref.put(o, model, stored, e, False, 200, 1e-7)
        o.forward()
        qacc = np.array(o.data.qacc, dtype=np.float64)
        v = dict(force=sref.force(qacc, ref), island=sref.island(qacc, ref), row=rref.row(qacc, ref, grp))
        c = o.contact_rows()
        if "con" in ref and o.contacts() == [tuple(g) for g in ref["con"]["geoms"].tolist()]:
            v.update(cr.contact_measure(c["force"][:, 0], c["wforce"], ref))
        for k in v:
            worst[k] = max(worst[k], v[k] if np.isfinite(v[k]) else np.inf)
    o.close()
    return worst


def table(libs, cases, load, model, floors, reference):
    """{defect: {case: largest measure / its floor}} over the cases of one stored file"""
    out = {name: {} for name in libs}
    for case, c in load.items():
        m = model(case)
        o = OracleSim(m)
        refs = [reference(o, m, c["st"], e) for e in range(len(c["island"]))]
        o.close()
        for name, path in libs.items():
            v = measures(path, c["st"], m, refs, rref.groups(m))
            out[name][case] = max(v[k] / floors[case][k] for k in v if k in floors[case])
    return out


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        libs = build(tmp)
        new = table(libs, cr.CASES, cr.load(), cr.model, cr.FLOOR, lambda o, m, st, e: cr.reference(o, m, st, e, step=False))
        old = table(libs, sref.CASES, sref.load(), sref.model, sref.FLOOR, lambda o, m, st, e: sref.reference(o, m, st, e, step=False))
        old2 = table(libs, rref.CASES, rref.load(), rref.model, rref.FLOOR, lambda o, m, st, e: sref.reference(o, m, st, e, step=False))
    for name in libs:
        o = dict(old[name], **old2[name])
        print("%-58s new: %s | old 19: worst %.1f floors (%s)" % (name or "(no defect)", "  ".join("%s %.0f" % kv for kv in new[name].items()), max(o.values()), max(o, key=o.get)))
