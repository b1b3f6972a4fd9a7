// fsim_momentum.hpp -- centre of mass, momentum and energy of sets of bodies (include/fsim_momentum.h).  Included at the end of fsim.hip, after
// fsim_wrench.hpp.
//
// One launch per fsim_momenta, on the handle's stream:
//   k_momenta  one wave per env, like k_dynamics.  qpos / qvel of the env record (read only) and nothing else of it.  The stages are those of
//              k_dynamics and of the step's fs_velocity_bias; the latter, which runs on the step's own context, and the chain sum, whose
//              reference point and scratch are this kernel's own, are written out here:
//              (1) world pose of every reduced body by pointer doubling (fsim_kin.hpp), then the inertial-frame origins x_b and the
//              subtree masks (stages A to C of k_dynamics); (2) the motion axes of every dof about the origin of the first body of the dof's tree (the reference
//              point of the tree's spatial vectors; a free part's own origin, so that its velocity is formed from R ipos and never from a
//              difference of positions: the same bits 8 m out as at the origin), every body's own joint twist,
//              the associative chain U o U' = U + U' up the ancestors by pointer doubling (stage H of k_dynamics without its acceleration
//              half), then per body the velocity v_b of x_b, the body's own angular momentum R (I_b (R^T w_b)) -- the product in the BODY
//              frame, then turned: turned into the world frame first, a leg's inertia (6.9e-6, 6.9e-6, 1.8e-7 kg m^2) loses its small
//              axis (stage G of k_dynamics) -- and its shares of the two energies; (3) lane = sensor: the set's 32-bit body
//              mask (unsigned: body 31 is the top bit) walked in ascending body order, mass-weighted sums of x_b - x_0 and v_b with x_0
//              the inertial origin of the set's lowest-numbered body, then the angular momentum from (x_b - c) and (v_b - v_c); (4) lane o
//              takes element o of the env's flat [S][3][nv] Jacobian, so that every store covers 64 consecutive words: the sum over the
//              bodies the dof moves AND the set holds, an exact 0 where there are none; (5) the energies: the per-body shares summed over
//              the wave in the fixed order of wave_sum, then the armature term over the dofs.
// No atomics, no scratch buffer, static LDS only: every output word is written once; every LDS word read was written in the same call.
// DESIGN.md 25.
#include "../../include/fsim_momentum.h"

#define MOM_MAX_NV 128 // dofs whose motion axes the pass holds (FSIM_DYN_MAX_NV; fsim_create refuses a model beyond it)

struct MomArgs {
  KinArgs kin;
  const int *r_ancmask, *r_tree, *dof_rbody, *tree_bodyadr;
  const float *r_mass, *r_ipos, *r_inertia, *dof_armature;
  const unsigned *masks; // [S]: the reduced bodies of every sensor
  int nv, S;
  float g[3];
  fsim_momentum_out_t out;
};

__global__ __launch_bounds__(64) void k_momenta(MomArgs a, const float *__restrict__ state) {
  __shared__ float sp[3 * 32], sq[4 * 32], sxi[3 * 32], sU[6 * 32], soff[3 * 32], sv[3 * 32], sh[3 * 32], sm[32], sinv[FSIM_MOM_MAX_SENSORS], scdof[6 * MOM_MAX_NV];
  __shared__ int sanc[32], sdb[MOM_MAX_NV], sref[32];
  __shared__ unsigned ssub[32], smask[FSIM_MOM_MAX_SENSORS];
  const int e = blockIdx.x, b = threadIdx.x;
  const float *rec = state + (size_t)e * a.kin.stride;
  for (int d = b; d < a.nv; d += 64) sdb[d] = a.dof_rbody[d];
  if (b < a.S) smask[b] = a.masks[b];
  // (1) stages A + B of k_dynamics: the pose of every body in its parent, then in the world by pointer doubling, left in sp / sq (fsim_kin.hpp)
  V3 P;
  Q4 Q;
  const KinLane l = kin_joint_pose(a.kin, rec, b, &P, &Q);
  kin_world_poses(a.kin, l, b, sp, sq, sanc, &P, &Q);
  const bool on = l.on;
  const int bb = l.bb;
  // stage C: inertial-frame origins, masses, the subtree masks from the ancestor masks (which carry the self bit), the tree's reference body
  const M3 R = q2m(Q);
  const float ms = on ? a.r_mass[bb] : 0.0f;
  const V3 ri = mulv(R, ldv3(a.r_ipos + 3 * bb));
  if (b < a.kin.nr) {
    stv3(sp + 3 * b, P);
    stq(sq + 4 * b, Q);
    stv3(sxi + 3 * b, P + ri);
    unsigned sub = 0;
    for (int d = b; d < a.kin.nr; d++)
      if (b > 0 && (((unsigned)a.r_ancmask[d] >> b) & 1u)) sub |= 1u << d;
    ssub[b] = sub;
    sm[b] = ms;
    sref[b] = on ? a.tree_bodyadr[a.r_tree[bb]] : 0;
  }
  __syncthreads();
  // (2) the motion axes of every dof about the origin of its tree's first body (for a free part its own origin: no difference of positions)
  for (int d = b; d < a.nv; d += 64) {
    const int db = sdb[d], djt = a.kin.r_jtype[db], k = d - a.kin.r_dofadr[db];
    const V3 Pb = ldv3(sp + 3 * db), ref = ldv3(sp + 3 * sref[db]);
    const Q4 Qb = ldq(sq + 4 * db);
    S6 s;
    s.a = v3(0, 0, 0);
    if (djt == JT_FREE) {
      const V3 ax = v3(k % 3 == 0 ? 1.0f : 0.0f, k % 3 == 1 ? 1.0f : 0.0f, k % 3 == 2 ? 1.0f : 0.0f);
      if (k < 3) s.l = ax;
      else { s.a = qrot(Qb, ax); s.l = cross(s.a, ref - Pb); }
    } else {
      const V3 ax = qrot(Qb, ldv3(a.kin.r_jaxis + 3 * db));
      if (djt == JT_SLIDE) s.l = ax;
      else { s.a = ax; s.l = cross(ax, ref - (Pb + qrot(Qb, ldv3(a.kin.r_jpos + 3 * db)))); }
    }
    sts6(scdof + 6 * d, s);
  }
  __syncthreads();
  // every body's own joint twist, then the sum up its ancestors
  S6 u = s6zero();
  if (on) {
    const int da = l.da;
    const float *qv = rec + a.kin.qvel + da;
    if (l.jt == JT_FREE) {
#pragma unroll
      for (int k = 0; k < 6; k++) u = u + lds6(scdof + 6 * (da + k)) * qv[k];
    } else
      u = lds6(scdof + 6 * da) * qv[0];
  }
  int anc = l.anc;
  for (int span = 1; span < a.kin.maxdepth; span <<= 1) {
    if (b < a.kin.nr) { sts6(sU + 6 * b, u); sanc[b] = anc; }
    __syncthreads();
    if (anc > 0) {
      const S6 ua = lds6(sU + 6 * anc);
      const int na = sanc[anc];
      u = ua + u;
      anc = na;
    }
    __syncthreads();
  }
  // per body: the velocity of its inertial origin, its own angular momentum (the product in the body frame, then turned), its energies
  float pe = 0.0f, ke = 0.0f;
  if (b < a.kin.nr) {
    const V3 xi = ldv3(sxi + 3 * b);
    const V3 off = (P - ldv3(sp + 3 * sref[b])) + ri; // x_b from the tree's reference point: for a free part 0 + ri, whatever its distance from the origin
    const V3 v = u.l + cross(u.a, off);
    stv3(soff + 3 * b, off);
    const float *ib = a.r_inertia + 6 * bb; // xx yy zz xy xz yz in the body frame
    const V3 wl = multv(R, u.a);
    const V3 Iw = v3(ib[0] * wl.x + ib[3] * wl.y + ib[4] * wl.z, ib[3] * wl.x + ib[1] * wl.y + ib[5] * wl.z, ib[4] * wl.x + ib[5] * wl.y + ib[2] * wl.z);
    stv3(sv + 3 * b, v);
    stv3(sh + 3 * b, on ? mulv(R, Iw) : v3(0, 0, 0));
    if (on) {
      pe = -ms * (a.g[0] * xi.x + a.g[1] * xi.y + a.g[2] * xi.z);
      ke = 0.5f * (ms * dot(v, v) + dot(wl, Iw));
    }
  }
  __syncthreads();
  // (3) lane = sensor: sums over the set's bodies in ascending order, positions relative to the inertial origin of the lowest-numbered one
  if (b < a.S) {
    const unsigned mask = smask[b];
    const V3 x0 = ldv3(sxi + 3 * (__ffs(mask) - 1));
    V3 sx = v3(0, 0, 0), sw = v3(0, 0, 0);
    float tot = 0.0f;
    for (unsigned mm = mask; mm; mm &= mm - 1) {
      const int k = __ffs(mm) - 1;
      const float mk = sm[k];
      sx = sx + mk * (ldv3(sxi + 3 * k) - x0);
      sw = sw + mk * ldv3(sv + 3 * k);
      tot += mk;
    }
    const float inv = 1.0f / tot; // (the host refuses a set without mass)
    const V3 c = sx * inv, vc = sw * inv;
    V3 L = v3(0, 0, 0);
    for (unsigned mm = mask; mm; mm &= mm - 1) {
      const int k = __ffs(mm) - 1;
      L = L + (ldv3(sh + 3 * k) + sm[k] * cross((ldv3(sxi + 3 * k) - x0) - c, ldv3(sv + 3 * k) - vc));
    }
    sinv[b] = inv;
    const size_t o = ((size_t)e * a.S + b) * 3;
    if (a.out.com) stv3(a.out.com + o, x0 + c);
    if (a.out.linvel) stv3(a.out.linvel + o, vc);
    if (a.out.angmom) stv3(a.out.angmom + o, L);
  }
  __syncthreads();
  // (4) lane o takes element o of the flat [S][3][nv] Jacobian: the bodies that dof d moves and sensor s holds
  if (a.out.jac) {
    const int row = 3 * a.nv, n = a.S * row;
    float *oj = a.out.jac + (size_t)e * n;
    for (int o = b; o < n; o += 64) {
      const int s = o / row, rem = o - s * row, k = rem / a.nv, d = rem - k * a.nv, db = sdb[d];
      const unsigned both = smask[s] & ssub[db];
      float val = 0.0f;
      if (both) {
        const S6 sd = lds6(scdof + 6 * d);
        V3 acc = v3(0, 0, 0);
        for (unsigned mm = both; mm; mm &= mm - 1) {
          const int kb = __ffs(mm) - 1;
          acc = acc + sm[kb] * (sd.l + cross(sd.a, ldv3(soff + 3 * kb)));
        }
        val = comp(acc, k) * sinv[s];
      }
      oj[o] = val;
    }
  }
  // (5) the energies: the bodies' shares over the wave in wave_sum's order, then the armature term over the dofs
  if (a.out.energy) {
    const float pot = wave_sum(pe), kin = wave_sum(ke);
    float arm = 0.0f;
    for (int d = b; d < a.nv; d += 64) {
      const float qd = rec[a.kin.qvel + d];
      arm += 0.5f * a.dof_armature[d] * qd * qd;
    }
    arm = wave_sum(arm);
    if (b == 0) {
      a.out.energy[2 * (size_t)e] = pot;
      a.out.energy[2 * (size_t)e + 1] = kin + arm;
    }
  }
}

// ------------------------------------------------------------------------------------------ host
struct MomState {
  int nsens = 0;
  unsigned *d_masks = nullptr; // MomArgs::masks
  DevTables tabs; // owns it
};

extern "C" int fsim_set_momenta(fsim_t *s, int n_sensors, const int32_t *adr, const int32_t *bodies, const int32_t *subtree) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_momenta: null handle");
  if (n_sensors == 0) return sensor_clear(s, s->mom);
  if (!adr || !bodies || !subtree) FAIL(FSIM_EINVAL, "fsim_set_momenta: null argument");
  if (n_sensors < 1 || n_sensors > FSIM_MOM_MAX_SENSORS) FAIL(FSIM_EINVAL, "fsim_set_momenta: %d sensors (1 .. %d)", n_sensors, FSIM_MOM_MAX_SENSORS);
  const DModel &m = s->m;
  if (m.nr > 32) FAIL(FSIM_EINVAL, "fsim_set_momenta: %d reduced bodies (the momentum pass holds at most 32: one body per lane, sets as 32-bit masks)", m.nr);
  if (m.nv > MOM_MAX_NV) FAIL(FSIM_EINVAL, "fsim_set_momenta: nv = %d (the momentum pass holds at most %d dofs)", m.nv, MOM_MAX_NV);
  std::vector<int> red, par;
  std::vector<float> rmass;
  if (!blob_i(s->blob, "body_red", red) || !blob_i(s->blob, "body_parentid", par) || !blob_f(s->blob, "r_mass", rmass)) return FSIM_EINVAL;
  if ((int)red.size() < m.nbody || (int)par.size() < m.nbody || (int)rmass.size() < m.nr) FAIL(FSIM_EINVAL, "fsim_set_momenta: the model's body tables are short");
  if (adr[0] != 0) FAIL(FSIM_EINVAL, "fsim_set_momenta: adr[0] is %d (0)", adr[0]);
  std::vector<unsigned> masks(n_sensors, 0u);
  for (int i = 0; i < n_sensors; i++) {
    if (adr[i + 1] <= adr[i]) FAIL(FSIM_EINVAL, "momentum sensor %d: adr gives it %d bodies (at least one)", i, adr[i + 1] - adr[i]);
    for (int k = adr[i]; k < adr[i + 1]; k++) {
      const int body = bodies[k];
      if (body < 0 || body >= m.nbody) FAIL(FSIM_EINVAL, "momentum sensor %d: unknown body %d (the model has %d bodies)", i, body, m.nbody);
      if (red[body] <= 0 || red[body] >= m.nr) FAIL(FSIM_EINVAL, "momentum sensor %d: body %d does not move (it is fixed in the world)", i, body);
      masks[i] |= 1u << red[body];
      if (!subtree[k]) continue;
      for (int d = body + 1; d < m.nbody; d++) { // the model bodies below it: a child's id is above its parent's
        int up = d;
        while (up > body && par[up] >= 0 && par[up] < up) up = par[up];
        if (up == body && red[d] > 0 && red[d] < m.nr) masks[i] |= 1u << red[d];
      }
    }
    float tot = 0.0f;
    for (int r = 1; r < m.nr; r++)
      if ((masks[i] >> r) & 1u) tot += rmass[r];
    if (!(tot > 0.0f)) FAIL(FSIM_EINVAL, "momentum sensor %d: the bodies of the set have zero total mass", i);
  }
  MomState c;
  c.nsens = n_sensors;
  return sensor_install(s, "fsim_set_momenta", s->mom, c, [&](DevTables &t) { t.put(&c.d_masks, masks.data(), masks.size()); });
}

extern "C" int fsim_momenta(fsim_t *s, const fsim_momentum_out_t *out) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_momenta: null handle");
  if (!out) FAIL(FSIM_EINVAL, "fsim_momenta: null argument");
  if (!s->mom) FAIL(FSIM_EINVAL, "fsim_momenta: no sensor set (fsim_set_momenta)");
  if (!out->com && !out->linvel && !out->angmom && !out->jac && !out->energy) FAIL(FSIM_EINVAL, "fsim_momenta: no output (every pointer NULL)");
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const MomState &k = *s->mom;
  const DModel &m = s->m;
  MomArgs ma{kin_args(s), m.r_ancmask, m.r_tree, m.dof_rbody, m.tree_bodyadr, m.r_mass, m.r_ipos, m.r_inertia, m.dof_armature, k.d_masks,
             m.nv, k.nsens, {m.gravity[0], m.gravity[1], m.gravity[2]}, *out};
  hipLaunchKernelGGL(k_momenta, dim3(s->n_envs), dim3(64), 0, s->stream, ma, s->d_state);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
