/* fsim_oracle.h -- CPU restatement (double precision, one env) of the physics the
 * reference reaches through mujoco-py (sim.forward()/sim.step(), furniture/env/furniture.py:2857-2879).
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in furniture_amd/ may link or call this;
 * it is the checker for the HIP path (tests/, __graft_entry__.smoke(), and the
 * cpu_baseline leg of bench.py).
 *
 * PARITY UNPINNED: MuJoCo 2.0 (closed binary, un-vendored: README.md:44,
 * requirements.txt:12) is absent from /root/reference and from this image and the
 * reference ships no numeric tests for this path.  The pipeline
 * below restates MuJoCo's *published* computation (kinematics, CRB, RNE, soft
 * constraint model with solref/solimp impedance, elliptic cones, PGS dual solver,
 * semi-implicit Euler with implicit joint damping) and is pinned only by analytic
 * invariants (tests/test_oracle_physics.py), by the reference's MJCF geometry, and by ONE
 * trajectory recorded from MuJoCo itself: the first 62 frames of the reference's
 * demos/Cursor_7.pkl are replayed within 1.5 mm (tests/test_demo_replay.py).  That is
 * evidence, not a pin of the solver: the status stays PARITY UNPINNED.
 */
#ifndef FSIM_ORACLE_H
#define FSIM_ORACLE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* `real` is the arithmetic type of the whole checker: double in libfsim_oracle.so / libfsim_cpu.so (THE checker), float in the
 * control build libfsim_cpu32.so (-DOSIM_REAL=float -fsingle-precision-constant, <tgmath.h>: the same source in fp32 throughout --
 * what `fp32 alone` does to a trajectory, scripts/divergence_control.py).  The Python binding (oracle/oracle_sim.py) is fp64 unless asked:
 * OracleSim(model, np.float32) binds the control build's osim_* entry points, for the per-contact read-out below. */
#ifndef OSIM_REAL
#define OSIM_REAL double
#endif
typedef OSIM_REAL real;

typedef struct osim osim_t;

osim_t *osim_create(const void *model_blob, size_t nbytes);
void osim_destroy(osim_t *);
const char *osim_last_error(void);

/* named views into the simulator's own memory (mujoco_py-style in-place access) */
real *osim_dptr(osim_t *, const char *name, int *count);
int32_t *osim_iptr(osim_t *, const char *name, int *count);

void osim_reset_data(osim_t *);          /* sim.reset(): qpos=qpos0, everything else 0 */
void osim_forward(osim_t *);             /* sim.forward() */
int osim_step(osim_t *);                 /* sim.step(); !=0 -> unstable (MujocoException analogue) */
void osim_site_vel(osim_t *, int site, real *velp3, real *velr3); /* data.site_xvelp/xvelr */
void osim_body_jac(osim_t *, int body, const real *point3, real *jacp_3xnv, real *jacr_3xnv);
void osim_full_M(osim_t *, real *M_nvxnv);

/* solver knobs: iterations, tolerance (<=0: fixed iterations), order (0 canonical) */
void osim_set_solver(osim_t *, int iterations, real tolerance);
int osim_last_solver_iters(osim_t *);
real osim_contact_dist(osim_t *, int i);
/* diagnostics: efc row of contact i; (type, dim, aref, R, D, mu, pos - margin, force) of row i; J_i . a; the Newton objective at qacc */
int osim_contact_row(osim_t *, int i);
int osim_row_info(osim_t *, int i, real *out8);
real osim_row_dot(osim_t *, int i, const real *a);
real osim_cost_at(osim_t *, const real *qacc);
/* listed contact i of the last osim_forward / osim_step, in list order; reads only.  out26: pos[3], frame[9] (rows: the normal from geom 1 to
 * geom 2, two tangents), includemargin, mu, dim, whether the contact became a row (dist < includemargin), R of the normal row, aref[3], the
 * three row forces of the last solve (frame coordinates), the world force on geom 2's body (frame' f).  Everything after `became a row` is 0
 * for a contact that did not.  -1: no such contact */
int osim_contact_info(osim_t *, int i, real *out26);
void osim_set_solver_kind(osim_t *, int kind); /* 0 = PGS (dual), 1 = Newton (primal, MuJoCo default) */

/* The narrow phase of ONE pair of geoms, with no model behind it: types (MuJoCo's mjtGeom numbers), world positions, row-major rotation
 * matrices, sizes, and for a convex mesh its hull vertices (geom frame, n of them; NULL / 0 otherwise).  Dispatches exactly as the
 * collision pass of osim_forward does (the pair is evaluated with the lower type number first; both share one routine) and writes
 * dist, pos[3], n[3] per contact, the normal pointing from the geom passed first to the geom passed second.  Returns the number of
 * contacts, or -1 when no routine serves the two types.  Pairs served by the portal routine ignore the margin: they are contacts only
 * once the shapes interpenetrate. */
int osim_narrowphase(int t1, const real *p1, const real *R1, const real *s1, const real *verts1, int n1,
                     int t2, const real *p2, const real *R2, const real *s2, const real *verts2, int n2, real margin, real out[16][7]);

#ifdef __cplusplus
}
#endif
#endif
