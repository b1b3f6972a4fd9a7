// fsim_contacts.hpp -- contact-force and touch sensors (include/fsim_contacts.h).  Included at the end of fsim.hip, after fsim_dynamics.hpp.
//
// One launch per fsim_contact_forces, on the handle's stream:
//   k_contact_force<GenCtx>  one wave per env, the generic one-wave context with the handle's one-wave layout (what FSIM_GENERIC=1 picks
//               for k_physics): the launch's speed matters less than the library's size and build time, so there is no specialised or
//               multi-wave instantiation.  (A) k_physics in mode 1 up to its stores: the record into LDS, the scalars cleared, the model
//               cache, then the shared out-of-line fs_substeps(c, 1, 1) -- collision, constraint assembly, the Newton solve; the final
//               qacc is in Layout::x.  The record is NEVER stored back.  (B) the slot registers of the solve die with it, so they are
//               read again from the contact records: the assembly left aref, D_n and D_t there, and nothing the solve does in the
//               default build writes those words (fs_stage_k runs only for islands assembled on the matrix cores, -DFSIM_MFMA_HESSIAN: in
//               that build the host refuses the call).  fs_make_constraints is NOT run again: it consumed C_DIST / C_INCM and wrote
//               aref[1], aref[2] over them, so a second run would read those as distances.  fs_load_slots, fs_body_spatial(qacc),
//               fs_jdot give J qacc - aref of every slot, fs_slot_k the cone state and the world force on geom 2's body.  (C) lane =
//               slot writes its row -- force, normal force, geom ids, point, normal, distance -- to a staging area behind the layout's
//               LDS image, compacted to the order of the contact list (the listed slots in slot order, as k_physics lists
//               contact_geoms).  (D) lane = sensor walks the rows in that order and sums: no atomics, a fixed order, every output word
//               written exactly once, zeros explicitly.  (E) the lanes stride over the raw list, every store covering 64 consecutive words.
// The distance of a slot that became a constraint is no longer in its record; it is recovered from aref[0] = -b v_n - k imp (dist -
// margin) with imp taken from D_n (header: con_dist).  DESIGN.md 21.
#include "../../include/fsim_contacts.h"

#define CON_SW 17 // words per staged row (odd: lane = slot stores spread over the banks)
enum { CS_F = 0, CS_FN = 3, CS_G1 = 4, CS_G2 = 5, CS_POS = 6, CS_NRM = 9, CS_DIST = 12, CS_CG = 13 /* colliding-geom indices g1 | g2 << 8 */ };

struct ConArgs {
  const unsigned *masks; // [nsens][2][mw]: bit g of side A, then of side B, over the colliding geoms
  int nsens, mw;
  fsim_contact_out_t out;
};

DEV bool con_bit(const unsigned *m, int g) { return (m[g >> 5] >> (g & 31)) & 1u; }

// dist of a slot that is an active constraint, from what fs_make_constraints left of it (S: the slot's registers, r: its record)
template <class Ctx> DEV float con_slot_dist(const Ctx &c, const float *r, const SolSlot &S) {
  CModel &m = c.m;
  const int *ri = reinterpret_cast<const int *>(r);
  const int g1 = ri[C_G1], g2 = ri[C_G2];
  const float mix = GP(m.cg_solmix)[g1] / (GP(m.cg_solmix)[g1] + GP(m.cg_solmix)[g2]);
  float sr[2], si[5];
  for (int i = 0; i < 2; i++) sr[i] = mix * GP(m.cg_solref)[2 * g1 + i] + (1 - mix) * GP(m.cg_solref)[2 * g2 + i];
  for (int i = 0; i < 5; i++) si[i] = mix * GP(m.cg_solimp)[5 * g1 + i] + (1 - mix) * GP(m.cg_solimp)[5 * g2 + i];
  float k, b;
  fs_impedance(sr, si, 0.0f, c.D.timestep, &k, &b); // (k and b do not depend on the distance)
  const float iw = GP(m.cg_invweight)[g1] + GP(m.cg_invweight)[g2];
  const float imp = iw / (1.0f / S.dn + iw); // D_n = 1 / R, R = (1 - imp) / imp * iw
  const V3 pos = ldv3(r + C_POS);
  const V3 vrel = fs_ptvel(c, c.ly.cvel, S.bt2, pos) - fs_ptvel(c, c.ly.cvel, S.bt1, pos);
  const float incm = fmaxf(GP(m.cg_margin)[g1], GP(m.cg_margin)[g2]) - fmaxf(GP(m.cg_gap)[g1], GP(m.cg_gap)[g2]); // (the pair record's margin - gap)
  return k * imp > 0.0f ? incm - (S.aref[0] + b * dot(S.fx, vrel)) / (k * imp) : 0.0f;
}

template <class Ctx> __global__ __launch_bounds__(64, 2) void k_contact_force(const DModel *mp, const Layout *lp, KParams kp, const float *state, ConArgs a) {
  extern __shared__ float L[];
  CModel &m = *(CModel *)mp;
  const int env = blockIdx.x;
  if (env >= kp.n_envs) return;
  const Ctx c(L, m, *(CLayout *)lp, (int)threadIdx.x, kp.newton_maxit, kp.newton_tol);
  const int lane = c.lane;
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
  float *st = L + c.ly.lds_words;
  if (act != 0) {
    float *q = st + CON_SW * row;
    int *qi = reinterpret_cast<int *>(q);
    const int g1 = ri[C_G1], g2 = ri[C_G2];
    stv3(q + CS_F, Fw);
    q[CS_FN] = fmaxf(dot(Fw, S.fx), 0.0f);
    qi[CS_G1] = m.cg_orig[g1]; qi[CS_G2] = m.cg_orig[g2];
    stv3(q + CS_POS, ldv3(r + C_POS));
    stv3(q + CS_NRM, ldv3(r + C_FRAME));
    q[CS_DIST] = act == 1 ? con_slot_dist(c, r, S) : r[C_DIST];
    qi[CS_CG] = g1 | (g2 << 8);
  }
  SYNC();
  // (D)
  const fsim_contact_out_t &o = a.out;
  if (lane < a.nsens && (o.force || o.touch || o.count)) {
    const unsigned *A = a.masks + (size_t)lane * 2 * a.mw, *B = A + a.mw;
    V3 acc = v3(0, 0, 0);
    float touch = 0.0f;
    int cnt = 0;
    for (int k = 0; k < n; k++) {
      const float *q = st + CON_SW * k;
      const int cg = reinterpret_cast<const int *>(q)[CS_CG], g1 = cg & 255, g2 = cg >> 8;
      const bool on2 = con_bit(A, g2) && con_bit(B, g1), on1 = con_bit(A, g1) && con_bit(B, g2); // A holds geom 2: + the force; geom 1: - the force
      if (on1 || on2) {
        const V3 F = ldv3(q + CS_F);
        acc = acc + (on2 ? F : -F);
        touch += q[CS_FN];
        cnt++;
      }
    }
    const size_t u = (size_t)env * a.nsens + lane;
    if (o.force) stv3(o.force + 3 * u, acc);
    if (o.touch) o.touch[u] = touch;
    if (o.count) o.count[u] = cnt;
  }
  if (o.status && lane == 0) o.status[env] = status;
  // (E)
  const size_t e1 = (size_t)env * C;
  if (o.con_geoms)
    for (int i = lane; i < 2 * C; i += 64) o.con_geoms[2 * e1 + i] = (i >> 1) < n ? reinterpret_cast<const int *>(st)[CON_SW * (i >> 1) + CS_G1 + (i & 1)] : -1;
  for (int w = 0; w < 3; w++) {
    float *dst = w == 0 ? o.con_pos : (w == 1 ? o.con_normal : o.con_force);
    const int off = w == 0 ? CS_POS : (w == 1 ? CS_NRM : CS_F);
    if (!dst) continue;
    for (int i = lane; i < 3 * C; i += 64) {
      const int k = i / 3;
      dst[3 * e1 + i] = k < n ? st[CON_SW * k + off + (i - 3 * k)] : 0.0f;
    }
  }
  if (o.con_dist)
    for (int i = lane; i < C; i += 64) o.con_dist[e1 + i] = i < n ? st[CON_SW * i + CS_DIST] : 0.0f;
  if (o.con_fn)
    for (int i = lane; i < C; i += 64) o.con_fn[e1 + i] = i < n ? st[CON_SW * i + CS_FN] : 0.0f;
}

// ------------------------------------------------------------------------------------------ host
struct ConState {
  int nsens = 0, mw = 0;
  unsigned *d_masks = nullptr; // ConArgs::masks
  DevTables tabs; // owns it
};

extern "C" int fsim_set_contacts(fsim_t *s, int n_sensors, const fsim_contact_sensor_t *sensors) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_contacts: null handle");
  if (n_sensors == 0) return sensor_clear(s, s->con);
  if (!sensors) FAIL(FSIM_EINVAL, "fsim_set_contacts: null argument");
  if (n_sensors < 1 || n_sensors > FSIM_CON_MAX_SENSORS) FAIL(FSIM_EINVAL, "fsim_set_contacts: %d sensors (1 .. %d)", n_sensors, FSIM_CON_MAX_SENSORS);
  if (s->ly.ncon_max > FSIM_CON_MAX_SLOTS) FAIL(FSIM_EINVAL, "fsim_set_contacts: the handle has %d contact slots (the contact-force pass serves at most %d: one slot per lane)", s->ly.ncon_max, FSIM_CON_MAX_SLOTS);
  const DModel &m = s->m;
  std::vector<int> orig;
  if (!blob_i(s->blob, "cg_orig", orig) || (int)orig.size() < m.ncg) FAIL(FSIM_EINVAL, "fsim_set_contacts: the model's cg_orig table is short");
  std::vector<int> cg_of(std::max(s->ngeom, 1), -1); // model geom id -> colliding-geom index
  for (int g = 0; g < m.ncg; g++)
    if (orig[g] >= 0 && orig[g] < s->ngeom) cg_of[orig[g]] = g;
  ConState c;
  c.nsens = n_sensors;
  c.mw = (m.ncg + 31) / 32;
  std::vector<unsigned> tab((size_t)n_sensors * 2 * c.mw, 0u);
  for (int i = 0; i < n_sensors; i++) {
    const fsim_contact_sensor_t &k = sensors[i];
    unsigned *A = tab.data() + (size_t)i * 2 * c.mw, *B = A + c.mw;
    if (k.na < 1 || !k.a) FAIL(FSIM_EINVAL, "contact sensor %d: side A is empty", i);
    if (k.nb < 0 || (k.nb > 0 && !k.b)) FAIL(FSIM_EINVAL, "contact sensor %d: side B has %d geoms and a null list", i, k.nb);
    for (int side = 0; side < 2; side++) {
      const int32_t *ids = side ? k.b : k.a;
      const int cnt = side ? k.nb : k.na;
      unsigned *M = side ? B : A;
      for (int j = 0; j < cnt; j++) {
        const int g = ids[j];
        if (g < 0 || g >= s->ngeom) FAIL(FSIM_EINVAL, "contact sensor %d: side %c names geom %d (the model has %d geoms)", i, side ? 'B' : 'A', g, s->ngeom);
        const int cg = cg_of[g];
        if (cg < 0) FAIL(FSIM_EINVAL, "contact sensor %d: side %c names geom %d, which does not collide", i, side ? 'B' : 'A', g);
        if ((M[cg >> 5] >> (cg & 31)) & 1u) FAIL(FSIM_EINVAL, "contact sensor %d: side %c lists geom %d twice", i, side ? 'B' : 'A', g);
        if (side && ((A[cg >> 5] >> (cg & 31)) & 1u)) FAIL(FSIM_EINVAL, "contact sensor %d: geom %d is on side A and on side B", i, g);
        M[cg >> 5] |= 1u << (cg & 31);
      }
    }
    if (k.nb == 0) // every colliding geom not in A
      for (int cg = 0; cg < m.ncg; cg++)
        if (!((A[cg >> 5] >> (cg & 31)) & 1u)) B[cg >> 5] |= 1u << (cg & 31);
  }
  return sensor_install(s, "fsim_set_contacts", s->con, c, [&](DevTables &t) { t.put(&c.d_masks, tab.data(), tab.size()); });
}

extern "C" int fsim_contact_forces(fsim_t *s, const fsim_contact_out_t *out) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_contact_forces: null handle");
  if (!out) FAIL(FSIM_EINVAL, "fsim_contact_forces: null argument");
  if (!s->con) FAIL(FSIM_EINVAL, "fsim_contact_forces: no sensor set (fsim_set_contacts)");
  if (!out->force && !out->touch && !out->count && !out->status && !out->con_geoms && !out->con_pos && !out->con_normal && !out->con_dist && !out->con_force && !out->con_fn)
    FAIL(FSIM_EINVAL, "fsim_contact_forces: no output (every pointer NULL)");
#if defined(FSIM_MFMA_HESSIAN) && FSIM_MFMA_HESSIAN != 2
  FAIL(FSIM_EINVAL, "fsim_contact_forces: this build assembles big islands on the matrix cores (-DFSIM_MFMA_HESSIAN), which stages over the contact records the pass reads");
#endif
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const ConState &k = *s->con;
  const size_t lds = (size_t)s->lds_bytes + 4 * (size_t)CON_SW * FSIM_CON_MAX_SLOTS; // the one-wave image and the staged rows behind it
  if (lds > 160 * 1024) FAIL(FSIM_ENOMEM, "fsim_contact_forces: the per-env LDS image and the staged rows take %zu bytes (160 KiB at most)", lds);
  {
    // the attribute is per function and process-wide: it is only ever raised, here to the ceiling, once per device
    static std::mutex mu;
    static std::vector<char> raised;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)raised.size() <= s->device) raised.resize(s->device + 1, 0);
    if (!raised[s->device]) {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_contact_force<GenCtx>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      raised[s->device] = 1;
    }
  }
  ConArgs ca{k.d_masks, k.nsens, k.mw, *out};
  hipLaunchKernelGGL(k_contact_force<GenCtx>, dim3(s->n_envs), dim3(64), lds, s->stream, s->d_m, s->d_ly, kparams(s, 0, 1), (const float *)s->d_state, ca);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
