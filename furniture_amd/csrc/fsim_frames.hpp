// fsim_frames.hpp -- body and site frame sensors with their Jacobians (include/fsim_frames.h).  Included at the end of fsim.hip, after
// fsim_pairs.hpp: the host part folds a frame's body into its reduced body with cam_mount_row, the function fsim_set_cameras places its
// mounts with, so a frame row has the layout of a camera row (CCW_*).
//
// One launch per fsim_frame_state, on the handle's stream:
//   k_frame_state  one wave per env, like k_cam_twist.  qpos of the env record (read only) -> world pose of every reduced body (stages (A)
//                  and (B) of k_cam_pose); when vel is asked for, qvel -> every body's summed twist about the WORLD ORIGIN (stages (T)
//                  and (U) of k_cam_twist; all four are the functions of fsim_kin.hpp); when jac is asked for, (J) the unit twist of
//                  every dof about the world origin into LDS, 6 * nv words (row-major [6][nv]: lanes of one round read consecutive words), a free joint contributing six columns and a model
//                  with nv > 64 taking a second round.  (S) lane s then takes sensor s: the poses of its two frames, pos and quat,
//                  and vel from the DIFFERENCE of the two bodies' twists taken at p -- (V_f - V_g) + (W_f - W_g) x p, which is
//                  v - v_g - w_g x r in real arithmetic and exactly 0 for two frames of one body; it leaves p, R_g and the two
//                  bodies' ancestor masks in LDS.  (K) the Jacobian, sensor by sensor (wave-uniform): column d is
//                  c * R_g^T (uv_d + uw_d x p | uw_d) with c = [d moves F] - [d moves G] from r_ancmask (which carries the self
//                  bit); lane d computes the column's six entries once, into a [6][nv] tile in LDS, and the tile is copied out with
//                  the lane index running along the contiguous [6][nv] tail of the sensor: every store of a round is 64 consecutive
//                  words.  (The first version computed element by element, the shared cross product six times over: 0.114 ms for
//                  64 sensors at 4096 envs and the same 0.086 ms at 1024 -- one wave's instruction stream, not traffic: DESIGN.md 19.)
//                  A dof that moves both frames or neither writes an exact 0.
// No atomics, no scratch: every output word is written once, and an env's output depends on nothing but its record and the frame set;
// every LDS word read was written in the same call.  The measurements: DESIGN.md 19.
#include "../../include/fsim_frames.h"

#define FRM_SW 16 // LDS words per sensor for stage (K): p 3, R_g 9, ancestor masks of F's and G's bodies, 2 unused

struct FrameArgs {
  KinArgs kin;
  const int *r_ancmask, *dof_rbody;
  const float *cursor_pos0;
  int nv, nsens, ecpos /* Cursor agent: EC_POS of the record, else -1 */;
};

// world pose of a frame row (CCW_*): reduced body pose (x) the host-composed offset; a cursor body's frame follows the env's cursor
DEV void frm_pose(const FrameArgs &a, const float *rec, const float *fw, const float *sp, const float *sq, V3 *p, Q4 *q, int *rb) {
  *rb = __float_as_int(fw[CCW_RBODY]);
  const int cur = __float_as_int(fw[CCW_CURSOR]);
  const Q4 qb = ldq(sq + 4 * *rb);
  V3 fp = ldv3(sp + 3 * *rb) + qrot(qb, ldv3(fw + CCW_POS));
  if (cur >= 0 && a.ecpos >= 0) fp = fp + ldv3(rec + a.ecpos + 3 * cur) - ldv3(a.cursor_pos0 + 3 * cur);
  *p = fp;
  *q = qnormalized(qmul(qb, ldq(fw + CCW_QUAT)));
}

__global__ __launch_bounds__(64) void k_frame_state(FrameArgs a, const float *__restrict__ state, const float *__restrict__ frames,
                                                    float *__restrict__ pos, float *__restrict__ quat, float *__restrict__ vel,
                                                    float *__restrict__ jac) {
  extern __shared__ float frm_ut[]; // (J) [6][nv]: rows 0-2 the dof's unit linear velocity at the world origin, rows 3-5 its unit angular velocity; then (K)'s two tiles
  __shared__ float sp[3 * 32], sq[4 * 32], sv[3 * 32], sw[3 * 32], ssen[FRM_SW * FSIM_FRAME_MAX_SENSORS];
  __shared__ int sanc[32], sdb[FSIM_FRAME_MAX_NV];
  const int e = blockIdx.x, b = threadIdx.x;
  const float *rec = state + (size_t)e * a.kin.stride;
  // (A) + (B) the world pose of every reduced body; when vel is asked for, (T) + (U) its summed twist about the world origin: fsim_kin.hpp
  V3 P;
  Q4 Q;
  const KinLane l = kin_joint_pose(a.kin, rec, b, &P, &Q);
  kin_world_poses(a.kin, l, b, sp, sq, sanc, &P, &Q);
  if (b < a.kin.nr) { stv3(sp + 3 * b, P); stq(sq + 4 * b, Q); }
  if (vel) {
    V3 v0, w;
    kin_joint_twist(a.kin, l, rec, P, Q, &v0, &w);
    kin_sum_twists(a.kin, l, b, sv, sw, sanc, v0, w);
  }
  __syncthreads();
  // (J) the unit twist of every dof about the world origin: hinge (anchor x a, a), slide (a, 0), free translation (e_i, 0), free
  //     rotation (x_b x R_b e_i, R_b e_i)
  if (jac) {
    for (int d = b; d < a.nv; d += 64) {
      const int db = a.dof_rbody[d], djt = a.kin.r_jtype[db], k = d - a.kin.r_dofadr[db];
      const V3 Pb = ldv3(sp + 3 * db);
      const Q4 Qb = ldq(sq + 4 * db);
      V3 uv = v3(0, 0, 0), uw = v3(0, 0, 0);
      if (djt == JT_FREE) {
        const V3 ax = v3(k % 3 == 0 ? 1.0f : 0.0f, k % 3 == 1 ? 1.0f : 0.0f, k % 3 == 2 ? 1.0f : 0.0f);
        if (k < 3) uv = ax;
        else { uw = qrot(Qb, ax); uv = cross(Pb, uw); }
      } else {
        const V3 ax = qrot(Qb, ldv3(a.kin.r_jaxis + 3 * db));
        if (djt == JT_SLIDE) uv = ax;
        else { uw = ax; uv = cross(Pb + qrot(Qb, ldv3(a.kin.r_jpos + 3 * db)), ax); }
      }
      frm_ut[d] = uv.x; frm_ut[a.nv + d] = uv.y; frm_ut[2 * a.nv + d] = uv.z;
      frm_ut[3 * a.nv + d] = uw.x; frm_ut[4 * a.nv + d] = uw.y; frm_ut[5 * a.nv + d] = uw.z;
      sdb[d] = db;
    }
  }
  // (S) lane s: sensor s
  for (int s = b; s < a.nsens; s += 64) {
    const float *fw = frames + 2 * CCW_WORDS * s;
    V3 pf, pg;
    Q4 qf, qg;
    int rf, rg;
    frm_pose(a, rec, fw, sp, sq, &pf, &qf, &rf);
    frm_pose(a, rec, fw + CCW_WORDS, sp, sq, &pg, &qg, &rg);
    const M3 Rg = q2m(qg);
    const size_t o = (size_t)e * a.nsens + s;
    if (pos) stv3(pos + 3 * o, multv(Rg, pf - pg));
    if (quat) stq(quat + 4 * o, qnormalized(qmul(qconj(qg), qf)));
    if (vel) {
      const V3 dw = ldv3(sw + 3 * rf) - ldv3(sw + 3 * rg);
      const V3 dv = ldv3(sv + 3 * rf) - ldv3(sv + 3 * rg);
      stv3(vel + 6 * o, multv(Rg, dv + cross(dw, pf)));
      stv3(vel + 6 * o + 3, multv(Rg, dw));
    }
    if (jac) {
      float *S = ssen + FRM_SW * s;
      stv3(S, pf);
      stm3(S + 3, Rg);
      S[12] = __int_as_float(a.r_ancmask[rf]);
      S[13] = __int_as_float(a.r_ancmask[rg]);
    }
  }
  if (!jac) return;
  __syncthreads();
  // (K) the Jacobian, sensor by sensor.  Lane d computes the six entries of column d once (the cross product and the two products
  //     with R_g^T are shared by the six rows) into the sensor's [6][nv] tile in LDS; then lane j of a round copies element j of the
  //     tile out: every store instruction covers 64 consecutive words.  Two tiles, used in turn, so that one barrier per sensor orders
  //     the writes of a tile after the reads of its previous use.
  const int len = 6 * a.nv;
  float *tiles = frm_ut + len; // [2][6][nv]
  for (int s = 0; s < a.nsens; s++) {
    const float *S = ssen + FRM_SW * s;
    float *T = tiles + (s & 1) * len;
    const V3 pf = ldv3(S);
    const M3 Rg = ldm3(S + 3);
    const unsigned mf = (unsigned)__float_as_int(S[12]), mg = (unsigned)__float_as_int(S[13]);
    for (int d = b; d < a.nv; d += 64) {
      const int db = sdb[d];
      const int c = (int)((mf >> db) & 1u) - (int)((mg >> db) & 1u);
      V3 lin = v3(0.0f, 0.0f, 0.0f), ang = v3(0.0f, 0.0f, 0.0f);
      if (c != 0) {
        const V3 uw = v3(frm_ut[3 * a.nv + d], frm_ut[4 * a.nv + d], frm_ut[5 * a.nv + d]);
        const V3 t = v3(frm_ut[d], frm_ut[a.nv + d], frm_ut[2 * a.nv + d]) + cross(uw, pf);
        const float cf = (float)c; // +-1: exact
        lin = multv(Rg, t) * cf;
        ang = multv(Rg, uw) * cf;
      }
      T[d] = lin.x; T[a.nv + d] = lin.y; T[2 * a.nv + d] = lin.z;
      T[3 * a.nv + d] = ang.x; T[4 * a.nv + d] = ang.y; T[5 * a.nv + d] = ang.z;
    }
    __syncthreads();
    float *out = jac + ((size_t)e * a.nsens + s) * len;
    for (int j = b; j < len; j += 64) out[j] = T[j];
  }
}

// ------------------------------------------------------------------------------------------ host
struct FrameState {
  int nsens = 0;
  float *d_frames = nullptr; // [nsens][2][CCW_WORDS]: the frame's row, then the reference's
  DevTables tabs; // owns it
};

extern "C" int fsim_set_frames(fsim_t *s, int n_sensors, const fsim_frame_sensor_t *sensors) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_frames: null handle");
  if (n_sensors == 0) return sensor_clear(s, s->frame);
  if (!sensors) FAIL(FSIM_EINVAL, "fsim_set_frames: null argument");
  if (n_sensors < 1 || n_sensors > FSIM_FRAME_MAX_SENSORS) FAIL(FSIM_EINVAL, "fsim_set_frames: %d sensors (1 .. %d)", n_sensors, FSIM_FRAME_MAX_SENSORS);
  const DModel &m = s->m;
  if (m.nr > 32) FAIL(FSIM_EINVAL, "fsim_set_frames: %d reduced bodies (the frame pass holds at most 32)", m.nr);
  if (m.nv > FSIM_FRAME_MAX_NV) FAIL(FSIM_EINVAL, "fsim_set_frames: nv = %d (the frame pass holds at most %d dofs)", m.nv, FSIM_FRAME_MAX_NV);
  CamMountTables mt;
  { int rc_ = cam_mount_tables(s, mt); if (rc_) return rc_; }
  std::vector<float> rows((size_t)2 * CCW_WORDS * n_sensors, 0.0f);
  for (int i = 0; i < n_sensors; i++) {
    const fsim_frame_t *two[2] = {&sensors[i].frame, &sensors[i].ref};
    for (int j = 0; j < 2; j++) {
      const fsim_frame_t &f = *two[j];
      const char *who = j ? "reference" : "frame";
      float *r = rows.data() + CCW_WORDS * (2 * i + j);
      if (f.body < -1 || f.body >= m.nbody) FAIL(FSIM_EINVAL, "frame sensor %d: %s: unknown body %d (the model has %d bodies)", i, who, f.body, m.nbody);
      if (cam_mount_row(mt, f.body, f.pos, f.quat, r)) FAIL(FSIM_EINVAL, "frame sensor %d: %s: bad pose (not finite, or a zero quaternion)", i, who);
      const int rb = __builtin_bit_cast(int, r[CCW_RBODY]);
      if (rb < 0 || rb >= m.nr) FAIL(FSIM_EINVAL, "frame sensor %d: %s: body %d folds into reduced body %d of %d", i, who, f.body, rb, m.nr);
    }
  }
  FrameState c;
  c.nsens = n_sensors;
  return sensor_install(s, "fsim_set_frames", s->frame, c, [&](DevTables &t) { t.put(&c.d_frames, rows.data(), rows.size()); });
}

extern "C" int fsim_frame_state(fsim_t *s, float *pos_dev, float *quat_dev, float *vel_dev, float *jac_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_frame_state: null handle");
  if (!s->frame) FAIL(FSIM_EINVAL, "fsim_frame_state: no frame set (fsim_set_frames)");
  if (!pos_dev && !quat_dev && !vel_dev && !jac_dev) FAIL(FSIM_EINVAL, "fsim_frame_state: no output (pos, quat, vel and jac all NULL)");
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const FrameState &k = *s->frame;
  const DModel &m = s->m;
  FrameArgs fa{kin_args(s), m.r_ancmask, m.dof_rbody, m.cursor_pos0, m.nv, k.nsens, m.agent == 2 ? s->ly.env + E_GROUP + m.nparts + EC_POS : -1};
  const size_t lds = jac_dev ? 4 * (size_t)18 * m.nv : 0; // the unit twists and the two tiles of stage (K): at most 9 KB
  hipLaunchKernelGGL(k_frame_state, dim3(s->n_envs), dim3(64), lds, s->stream, fa, s->d_state, k.d_frames, pos_dev, quat_dev, vel_dev, jac_dev);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
