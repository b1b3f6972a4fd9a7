// fsim_wrench.hpp -- force-torque, accelerometer and joint-load sensors (include/fsim_wrench.h).  Included at the end of fsim.hip, after
// fsim_contacts.hpp.
//
// One launch per fsim_wrenches, on the handle's stream:
//   k_wrench<GenCtx>  one wave per env, the generic one-wave context with the handle's one-wave layout, as k_contact_force.  (A) + (B) of
//               k_contact_force: the record into LDS, the scalars cleared, the model cache, fs_substeps(c, 1, 1), never stored back; then
//               fs_load_slots, fs_body_spatial(qacc), fs_jdot, fs_slot_k: W_b(qacc) of every body in Layout::W, J qacc - aref of every
//               weld in its record, the world force of every contact slot in a register.  (C) staged behind the layout's LDS image, before
//               anything below writes into the layout: per listed contact slot, compacted to the order of the contact list, the world
//               force, the point and the two compiled bodies; per weld its force F = -(D jar)[0..2] and torque T = C^T (-(D jar)[3..5]),
//               its two bodies and the two points.  (D) what the solve left standing and what it did not: xpos, xmat, xipos,
//               com, cvel, cdof, M, smooth and x survive; cinert, crb, cdofdot, cacc and cfrc lie under the Newton Hessian.  The body
//               inertias about the tree's centre of mass are therefore built again (wr_inertia: the loop of fs_com_inertia; that function
//               itself also needs the joint anchors, which lie under the Hessian too), and the (U, C) chain rule of fs_velocity_bias is
//               run again on its own (wr_velocity_product: that function keeps C in registers only).  (E) lane = body:
//               cacc_b = W_b(qacc) + C_b - g; cfrc_ext_b by a walk over the staged rows in list order, then the welds, then xfrc_applied
//               -- no atomics, a fixed order; cfrc_b = I cacc + v x* I v - cfrc_ext, all about the tree's centre of mass.  (F) lane =
//               sensor sums cfrc over its body's subtree in ascending body order, moves the wrench to the sensor origin and turns it into
//               the sensor frame -- except where the body hangs on a FREE joint: its six dofs span the wrench, so it is read off the
//               joint-space forces smooth + bias - xfrc_applied of those dofs, which is the same quantity without the cancellation of
//               m (a - g) against the constraint forces and without the solve's rounding of qacc; the accelerometer is the spatial
//               linear acceleration at the origin plus w x v_origin.  (G)
//               qfrc_constraint = fs_mulM(qacc) - smooth: both operands survive the solve, and the difference holds contacts, welds and
//               limits alike without walking them.  (H) the results go through a staging area so that the lanes stride over the outputs,
//               every store covering consecutive words.
// Every output word is written exactly once.  DESIGN.md 22.
#include "../../include/fsim_wrench.h"

#define WR_CW 9  // words per staged contact row (odd: lane = slot stores spread over the banks)
#define WR_WW 15 // words per staged weld row
#define WR_OW 19 // words per staged sensor result
enum { WC_F = 0, WC_POS = 3, WC_B1 = 6, WC_B2 = 7 };
enum { WW_ACT = 0, WW_F = 1, WW_T = 4, WW_B1 = 7, WW_B2 = 8, WW_P0 = 9, WW_X2 = 12 };
enum { WO_FORCE = 0, WO_TORQUE = 3, WO_ACCEL = 6, WO_ANGACC = 9, WO_EXT = 12 };

struct WrArgs {
  const float *rows; // [nsens][CCW_WORDS]: the sensor's reduced body, its origin and orientation in that body's frame
  int nsens;
  fsim_wrench_out_t out;
};

// body inertias about the tree's centre of mass into Layout::cinert (the second loop of fs_com_inertia; xmat, xipos and com survive the solve)
template <class Ctx> DEV void wr_inertia(const Ctx &c) {
  CModel &m = c.m;
  float *L = c.L;
  for (int b = c.lane; b < c.D.nr; b += 64) {
    float *I = L + c.ly.cinert + 10 * b;
    if (b == 0) { for (int k = 0; k < 10; k++) I[k] = 0; continue; }
    M3 R = ldm3(L + c.ly.xmat + 9 * b);
    auto ib = GP(m.r_inertia) + 6 * b; // xx yy zz xy xz yz in body frame
    M3 Ib;
    Ib.m[0] = ib[0]; Ib.m[4] = ib[1]; Ib.m[8] = ib[2]; Ib.m[1] = Ib.m[3] = ib[3]; Ib.m[2] = Ib.m[6] = ib[4]; Ib.m[5] = Ib.m[7] = ib[5];
    M3 T = mulm(R, Ib);
    float w[6];
    const int ij[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
    for (int e = 0; e < 6; e++) {
      int i = ij[e][0], j = ij[e][1];
      w[e] = T.m[3 * i] * R.m[3 * j] + T.m[3 * i + 1] * R.m[3 * j + 1] + T.m[3 * i + 2] * R.m[3 * j + 2];
    }
    float ms = KF(r_mass, b);
    V3 d = ldv3(L + c.ly.xipos + 3 * b) - ldv3(L + c.ly.com + 3 * KI(r_tree, b));
    float dd = dot(d, d);
    I[0] = w[0] + ms * (dd - d.x * d.x); I[1] = w[1] + ms * (dd - d.y * d.y); I[2] = w[2] + ms * (dd - d.z * d.z);
    I[3] = w[3] - ms * d.x * d.y; I[4] = w[4] - ms * d.x * d.z; I[5] = w[5] - ms * d.y * d.z;
    I[6] = ms * d.x; I[7] = ms * d.y; I[8] = ms * d.z; I[9] = ms;
  }
  SYNC();
}

// lane = body: its spatial velocity U and velocity-product acceleration C about the tree's centre of mass, by the associative rule
// (U, C) o (U', C') = (U + U', C + C' + U x U') of fs_velocity_bias, with that function's scratch (cacc, cfrc, the survivor list)
template <class Ctx> DEV void wr_velocity_product(const Ctx &c, S6 *U, S6 *C) {
  float *L = c.L;
  int *ancs = c.I(c.ly.surv);
  float *SU = L + c.ly.cacc, *SC = L + c.ly.cfrc;
  const int b = c.lane;
  const bool on = b < c.D.nr && b > 0;
  const int bb = on ? b : 0;
  const int jt = KI(r_jtype, bb), da = KI(r_dofadr, bb), parent = KI(r_parent, bb);
  S6 u = s6zero(), cc = s6zero();
  if (on) {
    if (jt == JT_FREE) {
      S6 vt = s6zero();
#pragma unroll
      for (int t = 0; t < 3; t++) vt = vt + lds6(L + c.ly.cdof + 6 * (da + t)) * L[c.ly.qvel + da + t];
      u = vt;
#pragma unroll
      for (int k = 3; k < 6; k++) {
        const S6 sk = lds6(L + c.ly.cdof + 6 * (da + k));
        const float qd = L[c.ly.qvel + da + k];
        u = u + sk * qd;
        cc = cc + cross_motion(vt, sk) * qd;
      }
    } else
      u = lds6(L + c.ly.cdof + 6 * da) * L[c.ly.qvel + da];
  }
  int anc = on ? parent : 0;
  for (int span = 1; span < c.D.maxdepth; span <<= 1) {
    if (b < c.D.nr) { sts6(SU + 6 * b, u); sts6(SC + 6 * b, cc); ancs[b] = anc; }
    SYNC();
    if (anc > 0) {
      const S6 ua = lds6(SU + 6 * anc), ca = lds6(SC + 6 * anc);
      const int na = ancs[anc];
      cc = ca + cc + cross_motion(ua, u);
      u = ua + u;
      anc = na;
    }
    SYNC();
  }
  *U = u;
  *C = cc;
}

template <class Ctx> __global__ __launch_bounds__(64, 2) void k_wrench(const DModel *mp, const Layout *lp, KParams kp, const float *state, WrArgs a) {
  extern __shared__ float L[];
  CModel &m = *(CModel *)mp;
  const int env = blockIdx.x;
  if (env >= kp.n_envs) return;
  const Ctx c(L, m, *(CLayout *)lp, (int)threadIdx.x, kp.newton_maxit, kp.newton_tol);
  const int lane = c.lane;
  const fsim_wrench_out_t &o = a.out;
  // (A)
  load_record(L, state + (size_t)env * c.ly.stride, c.ly.stride, lane);
  for (int i = lane; i < SC_WORDS; i += 64) reinterpret_cast<int *>(L + c.ly.scal)[i] = 0;
  SYNC();
  fs_load_cache(c);
  fs_substeps(c, 1, 1);
  // (B)
  const int *scal = c.I(c.ly.scal);
  const int nslot = min(scal[SC_NSLOT], c.ly.ncon_max), C = c.ly.ncon_max;
  const int status = (scal[SC_OVERFLOW] != 0 ? 1 : 0) | (scal[SC_BAD] != 0 ? 2 : 0);
  const float *r = L + c.ly.con + FSIM_CONW * min(lane, C - 1);
  const int *ri = reinterpret_cast<const int *>(r);
  const int act = lane < nslot ? ri[C_ACTIVE] : 0; // 1: a constraint, 2: listed, beyond margin - gap
  SolSlot S = fs_load_slots(c);
  fs_body_spatial(c, c.ly.x);
  fs_jdot(c, S, c.ly.x, true);
  V3 Fw;
  fs_slot_k(S, &Fw);
  // (C)
  const unsigned long long listed = __ballot(act != 0);
  const int n = __popcll(listed), row = __popcll(listed & ((1ull << lane) - 1ull));
  const int neq = c.D.neq, nr = c.D.nr, nv = c.D.nv;
  float *st = L + c.ly.lds_words, *sw = st + WR_CW * FSIM_WRENCH_MAX_SLOTS, *so = sw + WR_WW * neq;
  if (act != 0) {
    float *q = st + WR_CW * row;
    int *qi = reinterpret_cast<int *>(q);
    stv3(q + WC_F, Fw);
    stv3(q + WC_POS, ldv3(r + C_POS));
    qi[WC_B1] = S.bt1 & 255; qi[WC_B2] = S.bt2 & 255; // (a listed slot that is no constraint: body 0 twice, a zero force)
  }
  for (int e = lane; e < neq; e += 64) {
    const float *w = L + c.ly.weld + FSIM_WELDW * e;
    const int *wi = reinterpret_cast<const int *>(w);
    float *q = sw + WR_WW * e;
    int *qi = reinterpret_cast<int *>(q);
    const int on = wi[WD_ACTIVE] != 0;
    qi[WW_ACT] = on;
    if (!on) continue;
    float f[6];
    for (int k = 0; k < 6; k++) f[k] = -w[WD_D + k] * w[WD_JAR + k];
    stv3(q + WW_F, v3(f[0], f[1], f[2]));
    stv3(q + WW_T, v3(w[WD_C] * f[3] + w[WD_C + 3] * f[4] + w[WD_C + 6] * f[5], w[WD_C + 1] * f[3] + w[WD_C + 4] * f[4] + w[WD_C + 7] * f[5],
                      w[WD_C + 2] * f[3] + w[WD_C + 5] * f[4] + w[WD_C + 8] * f[5]));
    qi[WW_B1] = wi[WD_B1]; qi[WW_B2] = wi[WD_B2];
    stv3(q + WW_P0, ldv3(w + WD_P0));
    stv3(q + WW_X2, ldv3(w + WD_X2));
  }
  SYNC();
  // (G) first: fs_mulM reads M and x and writes Mx, none of which (D) touches
  if (o.qfrc_constraint) fs_mulM(c, c.ly.Mx, c.ly.x);
  // (D)
  wr_inertia(c);
  S6 u, cc;
  wr_velocity_product(c, &u, &cc);
  // (E)
  if (lane < nr) {
    const int b = lane;
    S6 acc = lds6(L + c.ly.W + 6 * b) + cc;
    acc.l = acc.l + v3(-c.D.gravity[0], -c.D.gravity[1], -c.D.gravity[2]);
    S6 ext = s6zero(), f = s6zero();
    if (b > 0) {
      const V3 com = ldv3(L + c.ly.com + 3 * KI(r_tree, b));
      for (int k = 0; k < n; k++) {
        const float *q = st + WR_CW * k;
        const int *qi = reinterpret_cast<const int *>(q);
        const int b1 = qi[WC_B1], b2 = qi[WC_B2];
        if (b1 != b && b2 != b) continue;
        const V3 F = ldv3(q + WC_F), mo = cross(ldv3(q + WC_POS) - com, F);
        if (b2 == b) { ext.a = ext.a + mo; ext.l = ext.l + F; }
        if (b1 == b) { ext.a = ext.a - mo; ext.l = ext.l - F; }
      }
      for (int e = 0; e < neq; e++) {
        const float *q = sw + WR_WW * e;
        const int *qi = reinterpret_cast<const int *>(q);
        if (!qi[WW_ACT] || (qi[WW_B1] != b && qi[WW_B2] != b)) continue;
        const V3 F = ldv3(q + WW_F), T = ldv3(q + WW_T);
        if (qi[WW_B1] == b) { ext.a = ext.a + (cross(ldv3(q + WW_P0) - com, F) + T); ext.l = ext.l + F; }
        if (qi[WW_B2] == b) { ext.a = ext.a - (cross(ldv3(q + WW_X2) - com, F) + T); ext.l = ext.l - F; }
      }
      for (int p = 0; p < c.D.nparts; p++) {
        if (GP(m.part_rbody)[p] != b) continue;
        const float *X = L + c.ly.xfrc + 6 * p; // force, then torque, at the body's centre of mass (fs_smooth)
        const V3 F = ldv3(X);
        ext.a = ext.a + (cross(ldv3(L + c.ly.xipos + 3 * b) - com, F) + ldv3(X + 3));
        ext.l = ext.l + F;
      }
      const float *I = L + c.ly.cinert + 10 * b;
      f = inert_mul(I, acc) + cross_force(u, inert_mul(I, u));
      f.a = f.a - ext.a; f.l = f.l - ext.l;
    }
    sts6(L + c.ly.cfrc + 6 * b, f);
    sts6(L + c.ly.cacc + 6 * b, ext);
    sts6(L + c.ly.crb + 6 * b, acc);
  }
  SYNC();
  // (F)
  if (lane < a.nsens) {
    const float *row_ = a.rows + CCW_WORDS * lane;
    const int rb = __float_as_int(row_[CCW_RBODY]);
    S6 fs = s6zero();
    for (unsigned mm = (unsigned)KI(r_submask, rb); mm; mm &= mm - 1u) fs = fs + lds6(L + c.ly.cfrc + 6 * (__ffs((int)mm) - 1)); // (unsigned: body 31 is the top bit)
    const M3 R = ldm3(L + c.ly.xmat + 9 * rb);
    const V3 org = ldv3(L + c.ly.xpos + 3 * rb) + mulv(R, ldv3(row_ + CCW_POS));
    const M3 Rs = mulm(R, q2m(ldq(row_ + CCW_QUAT)));
    const V3 d = org - ldv3(L + c.ly.com + 3 * KI(r_tree, rb));
    const S6 ab = lds6(L + c.ly.crb + 6 * rb), vb = lds6(L + c.ly.cvel + 6 * rb), ex = lds6(L + c.ly.cacc + 6 * rb);
    const V3 vo = vb.l + cross(vb.a, d);
    float *q = so + WR_OW * lane;
    V3 Fj = fs.l, Tj = fs.a - cross(d, fs.l); // the wrench through the joint: force, torque about the sensor origin, world frame
    if (KI(r_jtype, rb) == JT_FREE) {
      // A free joint's six dofs span the wrench, so the equation of motion gives it without the subtree sum: row d of
      // sum S_d . cfrc = qfrc_passive + qfrc_actuator + qfrc_applied = smooth + bias - (xfrc_applied on the dofs), the three translational
      // dofs the world-frame force, the three rotational ones the body-frame torque about the body origin (fs_com_inertia's cdof).  The sum
      // above is the same quantity as m (a - g) minus the constraint forces, a difference of terms of m g that carries the solve's rounding
      // of qacc (2.9e-7 N on a falling part of 30 g); this one carries neither, and is an exact zero where nothing acts along the joint.
      const int da = KI(r_dofadr, rb);
      const V3 xp = ldv3(L + c.ly.xpos + 3 * rb);
      V3 xl = v3(0, 0, 0), xr = v3(0, 0, 0);
      for (int p = 0; p < c.D.nparts; p++) {
        if (GP(m.part_rbody)[p] != rb) continue;
        const float *X = L + c.ly.xfrc + 6 * p;
        const V3 f = ldv3(X);
        xl = xl + f;
        xr = xr + multv(R, ldv3(X + 3) + cross(ldv3(L + c.ly.xipos + 3 * rb) - xp, f)); // (as fs_smooth projects it)
      }
      const float *sm = L + c.ly.smooth + da, *qb = L + c.ly.qfrcbias + da;
      Fj = v3((sm[0] + qb[0]) - xl.x, (sm[1] + qb[1]) - xl.y, (sm[2] + qb[2]) - xl.z);
      const V3 tb = v3((sm[3] + qb[3]) - xr.x, (sm[4] + qb[4]) - xr.y, (sm[5] + qb[5]) - xr.z);
      Tj = mulv(R, tb) - cross(org - xp, Fj);
    }
    stv3(q + WO_FORCE, multv(Rs, Fj));
    stv3(q + WO_TORQUE, multv(Rs, Tj));
    stv3(q + WO_ACCEL, multv(Rs, ab.l + cross(ab.a, d) + cross(vb.a, vo)));
    stv3(q + WO_ANGACC, multv(Rs, ab.a));
    stv3(q + WO_EXT, ex.l);
    stv3(q + WO_EXT + 3, ex.a - cross(d, ex.l));
  }
  SYNC();
  // (H)
  const int ns = a.nsens;
  for (int w = 0; w < 4; w++) {
    float *dst = w == 0 ? o.force : (w == 1 ? o.torque : (w == 2 ? o.accel : o.angacc));
    if (!dst) continue;
    for (int i = lane; i < 3 * ns; i += 64) {
      const int k = i / 3;
      dst[(size_t)env * 3 * ns + i] = so[WR_OW * k + 3 * w + (i - 3 * k)];
    }
  }
  if (o.external)
    for (int i = lane; i < 6 * ns; i += 64) {
      const int k = i / 6;
      o.external[(size_t)env * 6 * ns + i] = so[WR_OW * k + WO_EXT + (i - 6 * k)];
    }
  if (o.qacc)
    for (int i = lane; i < nv; i += 64) o.qacc[(size_t)env * nv + i] = L[c.ly.x + i];
  if (o.qfrc_constraint)
    for (int i = lane; i < nv; i += 64) o.qfrc_constraint[(size_t)env * nv + i] = L[c.ly.Mx + i] - L[c.ly.smooth + i];
  if (o.status && lane == 0) o.status[env] = status;
}

// ------------------------------------------------------------------------------------------ host
struct WrState {
  int nsens = 0;
  float *d_rows = nullptr; // WrArgs::rows
  DevTables tabs; // owns it
};

extern "C" int fsim_set_wrenches(fsim_t *s, int n_sensors, const fsim_wrench_sensor_t *sensors) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_wrenches: null handle");
  if (n_sensors == 0) return sensor_clear(s, s->wr);
  if (!sensors) FAIL(FSIM_EINVAL, "fsim_set_wrenches: null argument");
  if (n_sensors < 1 || n_sensors > FSIM_WRENCH_MAX_SENSORS) FAIL(FSIM_EINVAL, "fsim_set_wrenches: %d sensors (1 .. %d)", n_sensors, FSIM_WRENCH_MAX_SENSORS);
  if (s->ly.ncon_max > FSIM_WRENCH_MAX_SLOTS) FAIL(FSIM_EINVAL, "fsim_set_wrenches: the handle has %d contact slots (the wrench pass serves at most %d: one slot per lane)", s->ly.ncon_max, FSIM_WRENCH_MAX_SLOTS);
  const DModel &m = s->m;
  if (m.nr > 32) FAIL(FSIM_EINVAL, "fsim_set_wrenches: %d reduced bodies (the wrench pass holds at most 32: one body per lane, subtrees as 32-bit masks)", m.nr);
  CamMountTables mt;
  { int rc_ = cam_mount_tables(s, mt); if (rc_) return rc_; }
  std::vector<float> rows((size_t)CCW_WORDS * n_sensors, 0.0f);
  for (int i = 0; i < n_sensors; i++) {
    const fsim_wrench_sensor_t &k = sensors[i];
    float *r = rows.data() + CCW_WORDS * i;
    if (k.body < 0 || k.body >= m.nbody) FAIL(FSIM_EINVAL, "wrench sensor %d: unknown body %d (the model has %d bodies; a frame fixed in the world has no joint to cut)", i, k.body, m.nbody);
    if (cam_mount_row(mt, k.body, k.pos, k.quat, r)) FAIL(FSIM_EINVAL, "wrench sensor %d: bad pose (not finite, or a zero quaternion)", i);
    const int rb = __builtin_bit_cast(int, r[CCW_RBODY]);
    if (rb <= 0 || rb >= m.nr || __builtin_bit_cast(int, r[CCW_CURSOR]) >= 0) FAIL(FSIM_EINVAL, "wrench sensor %d: body %d does not move (it is fixed in the world)", i, k.body);
  }
  WrState c;
  c.nsens = n_sensors;
  return sensor_install(s, "fsim_set_wrenches", s->wr, c, [&](DevTables &t) { t.put(&c.d_rows, rows.data(), rows.size()); });
}

extern "C" int fsim_wrenches(fsim_t *s, const fsim_wrench_out_t *out) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_wrenches: null handle");
  if (!out) FAIL(FSIM_EINVAL, "fsim_wrenches: null argument");
  if (!s->wr) FAIL(FSIM_EINVAL, "fsim_wrenches: no sensor set (fsim_set_wrenches)");
  if (!out->force && !out->torque && !out->accel && !out->angacc && !out->external && !out->qacc && !out->qfrc_constraint && !out->status)
    FAIL(FSIM_EINVAL, "fsim_wrenches: no output (every pointer NULL)");
#if defined(FSIM_MFMA_HESSIAN) && FSIM_MFMA_HESSIAN != 2
  FAIL(FSIM_EINVAL, "fsim_wrenches: this build assembles big islands on the matrix cores (-DFSIM_MFMA_HESSIAN), which stages over the contact records the pass reads");
#endif
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const WrState &k = *s->wr;
  // the one-wave image and behind it the staged contact rows, weld rows and sensor results
  const size_t lds = (size_t)s->lds_bytes + 4 * ((size_t)WR_CW * FSIM_WRENCH_MAX_SLOTS + (size_t)WR_WW * s->m.neq + (size_t)WR_OW * FSIM_WRENCH_MAX_SENSORS);
  if (lds > 160 * 1024) FAIL(FSIM_ENOMEM, "fsim_wrenches: the per-env LDS image and the staged rows take %zu bytes (160 KiB at most)", lds);
  {
    // the attribute is per function and process-wide: it is only ever raised, here to the ceiling, once per device
    static std::mutex mu;
    static std::vector<char> raised;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)raised.size() <= s->device) raised.resize(s->device + 1, 0);
    if (!raised[s->device]) {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_wrench<GenCtx>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      raised[s->device] = 1;
    }
  }
  WrArgs wa{k.d_rows, k.nsens, *out};
  hipLaunchKernelGGL(k_wrench<GenCtx>, dim3(s->n_envs), dim3(64), lds, s->stream, s->d_m, s->d_ly, kparams(s, 0, 1), (const float *)s->d_state, wa);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
