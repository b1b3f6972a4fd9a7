// fsim_clearance.hpp -- what-if clearance queries (include/fsim_clearance.h).  Included at the end of fsim.hip, after fsim_pairs.hpp: the
// host part takes the pair sensors through pair_tables and launches k_pair_dist as it is through pair_launch, a pose row standing for an
// env; what is new is the kernel in front of it, which evaluates the kinematics at a configuration other than the record's.
//
// Two launches per chunk of envs (fsim_clearance splits a call so that its rows fit the scratch), both on the handle's stream:
//   k_clr_pose   one wave per row (env, candidate), lane b = reduced body b, as k_cam_pose.  The env's qpos is copied into LDS and the
//                listed addresses are overwritten with the candidate's finite values; stages (A) and (B) of fsim_kin.hpp then run on
//                that image (a KinArgs of its own with qpos = 0), so the record is never written and the arithmetic is the one every
//                other pose kernel runs.  Where the env's carry mask is not zero the two stages run a second time on the record itself
//                and one lane per rule composes X_carrier(candidate) o X_carrier(record)^-1 o X_part(record) into the part's pose: all
//                rules read first, a barrier, then they write, so a rule never sees another rule's result.  With a zero mask none of
//                that runs and the row is the one without rules.  Stage (C) is k_cam_pose's, operand for operand, Cursor branch included.
//   k_pair_dist  (fsim_pairs.hpp) over the chunk's rows, with the output pointers moved to the chunk.
// No atomics; every scratch and output word is written once per launch, and a row depends on nothing but its env's record, its candidate,
// its env's mask byte and the set.  The measurements: DESIGN.md 28.
#include "../../include/fsim_clearance.h"

#define CLR_DEFAULT_ROWS 32768

struct ClrArgs {
  CamPoseArgs cp;   // (ncam = 0; pstride: words of a scratch row)
  const int *adr;   // [ndofs] the qpos address of a candidate's column
  const int *carry; // [ncarry][2] the reduced body of the part, of the carrier
  int nq, ndofs, ncarry, K, e0 /* first env of the chunk */;
};

__global__ __launch_bounds__(64) void k_clr_pose(ClrArgs a, const float *__restrict__ state, const float *__restrict__ cand,
                                                 const uint8_t *__restrict__ cmask, float *__restrict__ pose, uint8_t *__restrict__ valid) {
  extern __shared__ float clr_q[]; // [nq] the env's qpos with the candidate written over it
  __shared__ float sp[3 * 32], sq[4 * 32], sp0[3 * 32], sq0[4 * 32];
  __shared__ int sanc[32];
  const int row = blockIdx.x, b = threadIdx.x;
  const int e = a.e0 + row / a.K, k = row % a.K;
  const float *rec = state + (size_t)e * a.cp.kin.stride;
  float *out = pose + (size_t)row * a.cp.pstride;
  for (int i = b; i < a.nq; i += 64) clr_q[i] = rec[a.cp.kin.qpos + i];
  __syncthreads();
  int bad = 0;
  if (b < a.ndofs) { // (at most 32 columns: one per lane)
    const float v = cand[((size_t)e * a.K + k) * a.ndofs + b];
    if ((__float_as_uint(v) & 0x7f800000u) != 0x7f800000u) clr_q[a.adr[b]] = v;
    else bad = 1; // not finite: the env's own value stays
  }
  bad = wave_or(bad);
  if (valid && b == 0) valid[(size_t)e * a.K + k] = bad ? 0 : 1;
  __syncthreads();
  // (A) + (B) at the candidate: fsim_kin.hpp on the image
  KinArgs ka = a.cp.kin;
  ka.qpos = 0;
  V3 P;
  Q4 Q;
  const KinLane l = kin_joint_pose(ka, clr_q, b, &P, &Q);
  kin_world_poses(ka, l, b, sp, sq, sanc, &P, &Q);
  if (b < ka.nr) { stv3(sp + 3 * b, P); stq(sq + 4 * b, Q); }
  __syncthreads();
  // carried parts: (A) + (B) once more, on the record, and the composition
  const int mask = cmask ? __builtin_amdgcn_readfirstlane((int)cmask[e] & ((1 << a.ncarry) - 1)) : 0;
  if (mask) {
    V3 P0;
    Q4 Q0;
    const KinLane l0 = kin_joint_pose(a.cp.kin, rec, b, &P0, &Q0);
    kin_world_poses(a.cp.kin, l0, b, sp0, sq0, sanc, &P0, &Q0);
    if (b < ka.nr) { stv3(sp0 + 3 * b, P0); stq(sq0 + 4 * b, Q0); }
    __syncthreads();
    int part = -1;
    V3 Pn = v3(0, 0, 0);
    Q4 Qn = q4(1, 0, 0, 0);
    if (b < a.ncarry && ((mask >> b) & 1)) {
      part = a.carry[2 * b];
      const int c = a.carry[2 * b + 1];
      const Q4 qi = qconj(ldq(sq0 + 4 * c)); // X_carrier(record)^-1 o X_part(record)
      const V3 prel = qrot(qi, ldv3(sp0 + 3 * part) - ldv3(sp0 + 3 * c));
      const Q4 qrel = qmul(qi, ldq(sq0 + 4 * part));
      const Q4 qc = ldq(sq + 4 * c);
      Pn = ldv3(sp + 3 * c) + qrot(qc, prel);
      Qn = qnormalized(qmul(qc, qrel));
    }
    __syncthreads();
    if (part >= 0) { stv3(sp + 3 * part, Pn); stq(sq + 4 * part, Qn); }
    __syncthreads();
  }
  // (C) colliding geoms: k_cam_pose's stage, operand for operand
  for (int g = b; g < a.cp.ncg; g += 64) {
    const int gb = a.cp.cg_body[g];
    const M3 Rb = q2m(ldq(sq + 4 * gb));
    V3 gp = ldv3(sp + 3 * gb) + mulv(Rb, ldv3(a.cp.cg_pos + 3 * g));
    if (a.cp.ecpos >= 0) {
      const int cm = a.cp.cg_cursor[g];
      if (cm) { const int kc = (cm & 1) ? 0 : 1; gp = gp + ldv3(rec + a.cp.ecpos + 3 * kc) - ldv3(a.cp.cursor_pos0 + 3 * kc); }
    }
    stv3(out + CAM_PW * g, gp);
    stm3(out + CAM_PW * g + 3, mulm(Rb, ldm3(a.cp.cg_mat + 9 * g)));
  }
}

// ------------------------------------------------------------------------------------------ host
struct ClrState {
  int nsens = 0, npairs = 0, pstride = 0, ndofs = 0, ncarry = 0, maxcand = 0, rows = 0;
  float *d_cg = nullptr, *d_sens = nullptr, *d_pose = nullptr;
  int *d_pairs = nullptr, *d_adr = nullptr, *d_carry = nullptr;
  DevTables tabs; // owns them
};

extern "C" int fsim_set_clearance(fsim_t *s, int n_dofs, const int32_t *dofs, int n_sensors, const fsim_pair_sensor_t *sensors, int n_carry,
                                  const fsim_clr_carry_t *carry, int max_candidates, int scratch_rows) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_clearance: null handle");
  if (n_sensors == 0) return sensor_clear(s, s->clr);
  const DModel &m = s->m;
  if (m.nr > 32) FAIL(FSIM_EINVAL, "fsim_set_clearance: %d reduced bodies (the pose pass holds at most 32: one body per lane)", m.nr);
  std::vector<int> dof_rbody, dof_qposadr, jtype, red;
  if (!blob_i(s->blob, "dof_rbody", dof_rbody) || !blob_i(s->blob, "dof_qposadr", dof_qposadr) || !blob_i(s->blob, "r_jtype", jtype) || !blob_i(s->blob, "body_red", red)) return FSIM_EINVAL;
  if ((int)dof_rbody.size() < m.nv || (int)dof_qposadr.size() < m.nv || (int)jtype.size() < m.nr || (int)red.size() < m.nbody) FAIL(FSIM_EINVAL, "fsim_set_clearance: the model's joint tables are short");
  if (n_dofs == 0 || (n_dofs > 0 && !dofs))
    FAIL(FSIM_EINVAL, "fsim_set_clearance: no dofs listed (a candidate needs at least one hinge or slide joint%s)", m.agent == 2 ? "; the Cursor agent has none: its cursors do not move by joints" : "");
  if (n_dofs < 0 || n_dofs > FSIM_CLR_MAX_DOFS) FAIL(FSIM_EINVAL, "fsim_set_clearance: %d dofs (1 .. %d)", n_dofs, FSIM_CLR_MAX_DOFS);
  std::vector<int> adr(n_dofs);
  for (int j = 0; j < n_dofs; j++) {
    const int d = dofs[j];
    if (d < 0 || d >= m.nv) FAIL(FSIM_EINVAL, "fsim_set_clearance: dof %d (column %d) is out of range (the model has %d dofs)", d, j, m.nv);
    const int rb = dof_rbody[d];
    if (rb <= 0 || rb >= m.nr || (jtype[rb] != JT_HINGE && jtype[rb] != JT_SLIDE))
      FAIL(FSIM_EINVAL, "fsim_set_clearance: dof %d (column %d) is not the dof of a hinge or slide joint (a free joint's dofs cannot be candidates)", d, j);
    for (int i = 0; i < j; i++)
      if (dofs[i] == d) FAIL(FSIM_EINVAL, "fsim_set_clearance: dof %d is listed twice (columns %d and %d)", d, i, j);
    adr[j] = dof_qposadr[d];
    if (adr[j] < 0 || adr[j] >= m.nq) FAIL(FSIM_EINVAL, "fsim_set_clearance: dof %d has qpos address %d (nq = %d)", d, adr[j], m.nq);
  }
  if (n_carry < 0 || n_carry > FSIM_CLR_MAX_CARRY) FAIL(FSIM_EINVAL, "fsim_set_clearance: %d carry rules (0 .. %d)", n_carry, FSIM_CLR_MAX_CARRY);
  if (n_carry > 0 && !carry) FAIL(FSIM_EINVAL, "fsim_set_clearance: null argument (carry)");
  std::vector<int> crow(2 * (size_t)n_carry);
  for (int r = 0; r < n_carry; r++) {
    const int pb = carry[r].part_body, cb = carry[r].carrier_body;
    if (pb < 0 || pb >= m.nbody || red[pb] <= 0 || red[pb] >= m.nr || jtype[red[pb]] != JT_FREE)
      FAIL(FSIM_EINVAL, "carry rule %d: body %d is not a furniture part (a body that moves by a free joint)", r, pb);
    if (cb < 0 || cb >= m.nbody || red[cb] < 0 || red[cb] >= m.nr) FAIL(FSIM_EINVAL, "carry rule %d: unknown carrier body %d (the model has %d bodies)", r, cb, m.nbody);
    if (red[cb] == red[pb]) FAIL(FSIM_EINVAL, "carry rule %d: the carrier body %d belongs to the part it carries", r, cb);
    for (int i = 0; i < r; i++)
      if (crow[2 * i] == red[pb]) FAIL(FSIM_EINVAL, "carry rule %d: the part of body %d is carried by rule %d already", r, pb, i);
    crow[2 * r] = red[pb]; crow[2 * r + 1] = red[cb];
  }
  if (max_candidates < 1 || max_candidates > FSIM_CLR_MAX_CANDIDATES) FAIL(FSIM_EINVAL, "fsim_set_clearance: max_candidates %d (1 .. %d)", max_candidates, FSIM_CLR_MAX_CANDIDATES);
  const size_t all = (size_t)s->n_envs * max_candidates;
  if (scratch_rows != 0 && scratch_rows < max_candidates) FAIL(FSIM_EINVAL, "fsim_set_clearance: scratch_rows %d (0, or at least max_candidates = %d)", scratch_rows, max_candidates);
  const size_t rows = std::min(all, scratch_rows ? (size_t)scratch_rows : (size_t)CLR_DEFAULT_ROWS);
  PairTables pt;
  { int rc_ = pair_tables(s, "fsim_set_clearance", n_sensors, sensors, pt); if (rc_) return rc_; }
  if (rows * n_sensors > 0x7fffffff) FAIL(FSIM_EINVAL, "fsim_set_clearance: %zu scratch rows of %d sensors (at most 2^31 - 1 units per launch)", rows, n_sensors);
  ClrState c;
  c.nsens = n_sensors; c.npairs = (int)pt.pairs.size(); c.pstride = std::max(pt.pstride, 4);
  c.ndofs = n_dofs; c.ncarry = n_carry; c.maxcand = max_candidates; c.rows = (int)rows;
  return sensor_install(s, "fsim_set_clearance", s->clr, c, [&](DevTables &t) {
    t.put(&c.d_sens, pt.srow.data(), pt.srow.size());
    t.put(&c.d_pairs, pt.pairs.data(), pt.pairs.size());
    t.put(&c.d_cg, pt.cg.data(), pt.cg.size());
    t.put(&c.d_adr, adr.data(), adr.size());
    t.put(&c.d_carry, crow.data(), crow.size());
    t.put(&c.d_pose, nullptr, rows * c.pstride);
  });
}

extern "C" int fsim_clearance(fsim_t *s, int K, const float *cand_dev, const uint8_t *carry_mask_dev, float *dist_dev, int32_t *geoms_dev, float *fromto_dev,
                              float *normal_dev, uint8_t *valid_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_clearance: null handle");
  if (!s->clr) FAIL(FSIM_EINVAL, "fsim_clearance: no clearance set (fsim_set_clearance)");
  const ClrState &k = *s->clr;
  if (K < 1 || K > k.maxcand) FAIL(FSIM_EINVAL, "fsim_clearance: K = %d candidates (1 .. max_candidates = %d)", K, k.maxcand);
  if (!cand_dev) FAIL(FSIM_EINVAL, "fsim_clearance: null argument (candidates)");
  if (!dist_dev && !geoms_dev && !fromto_dev && !normal_dev) FAIL(FSIM_EINVAL, "fsim_clearance: no output (distance, geoms, fromto and normal all NULL)");
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const DModel &m = s->m;
  ClrArgs ca{cam_pose_args(s, 0 /* no frames */, k.pstride), k.d_adr, k.d_carry, m.nq, k.ndofs, k.ncarry, K, 0};
  const int per = k.rows / K; // envs per chunk (rows >= max_candidates >= K: at least one)
  for (int e0 = 0; e0 < s->n_envs; e0 += per) {
    const size_t rows = (size_t)std::min(per, s->n_envs - e0) * K, o = (size_t)e0 * K * k.nsens;
    ca.e0 = e0;
    hipLaunchKernelGGL(k_clr_pose, dim3((unsigned)rows), dim3(64), 4 * (size_t)m.nq, s->stream, ca, s->d_state, cand_dev, carry_mask_dev, k.d_pose, valid_dev);
    HIPCHK(hipGetLastError());
    int rc_ = pair_launch(s, "fsim_clearance", rows, k.nsens, k.pstride, k.d_pose, k.d_cg, k.d_sens, k.d_pairs, dist_dev ? dist_dev + o : nullptr,
                          geoms_dev ? geoms_dev + 2 * o : nullptr, fromto_dev ? fromto_dev + 6 * o : nullptr, normal_dev ? normal_dev + 3 * o : nullptr);
    if (rc_) return rc_;
  }
  return FSIM_OK;
}
