// fsim_dynamics.hpp -- joint-space inertia, its inverse and the bias forces (include/fsim_dynamics.h).  Included at the end of fsim.hip, after
// fsim_frames.hpp.
//
// One launch per fsim_dynamics, on the handle's stream:
//   k_dynamics  one wave per env, like k_frame_state.  qpos / qvel of the env record (read only).  The stages are those of k_frame_state and
//               of the step's fs_com_inertia / fs_crb_factor / fs_velocity_bias; the latter, which run on the step's own context, are
//               written out here (DESIGN.md 11, 15 and 19 record what sharing a loop did to existing kernels):
//               (A) + (B) world pose of every reduced body by pointer doubling (fsim_kin.hpp); (C) inertial-frame origins; (D) per-tree
//               centre of mass, the reference point of every spatial vector of the tree (what keeps fp32 honest far from the origin); (E) body inertias
//               about it and the motion axes of every dof, a model with nv > 64 taking a second round; (F) composite inertias of every
//               body's strict descendants through the subtree masks (unsigned: body 31 is the top bit); (G) lane = dof i: row i of the
//               packed per-tree lower triangle of M, M_ij = cdof_j . (crb_body(i) cdof_i) + the share of body(i) itself, where body(j) is
//               an ancestor-or-self of body(i), an exact 0 elsewhere, armature on the diagonal.  Body(i)'s own share is evaluated in ITS
//               frame, m v_j . v_i + w_j . (I_b w_i) with v the velocity of its centre of mass and w the angular axis in the body frame
//               (for the body's own dofs the model's constants: e_k of a free joint, the hinge axis): a part's rotational block is then
//               its body-frame inertia itself.  Turned into the world frame in fp32, a leg's inertia (6.9e-6, 6.9e-6, 1.8e-7 kg m^2)
//               loses its small axis, and M^-1 was off by 9e-6 of its largest entry, 30 x what fp32 does to M itself; (H) bias and gravity: the associative (U, C) chain rule of fs_velocity_bias gives every body's velocity and
//               velocity-product acceleration, the body force is f_g = I (0, -g) for gravity and f_g + (I C + U x* I U) for bias, and ONE
//               loop (not unrolled: the same instructions) projects first the one and then the other on the dofs -- at qvel = 0 the
//               added term is a zero in every component, so bias and gravity agree bit for bit; (I) for minv, the Cholesky factor
//               L of every tree at once, left-looking, lane = row, one barrier per column; (J) X = L^-1, lane = column, no barrier;
//               (K) the gather: lane o takes element o of the flat [K][K] tile, so that every store covers 64 consecutive words;
//               mass(i, j) is the packed entry (max, min), minv(i, j) = sum_k X[k][lo] X[k][hi] with the factors in that order, so
//               that (i, j) and (j, i) are the same bits and an entry depends on its two dofs alone.
// No atomics, no scratch: every output word is written once; every LDS word read was written in the same call.  DESIGN.md 20.
#include "../../include/fsim_dynamics.h"

struct DynArgs {
  KinArgs kin;
  const int *r_ancmask, *r_tree, *dof_rbody, *tree_bodyadr, *tree_bodynum;
  const float *r_mass, *r_ipos, *r_inertia, *dof_armature;
  const int *tab; // [2 * nv]: per dof (first dof of its tree | dofs of the tree << 8), first word of the tree's packed triangle; then [K]: the selection
  int nv, ntree, K, W /* words of all packed triangles */, maxn /* dofs of the largest tree */;
  float g[3];
};

#define DYN_TRI(l) (((l) * ((l) + 1)) >> 1)

__global__ __launch_bounds__(64) void k_dynamics(DynArgs a, const float *__restrict__ state, float *__restrict__ mass, float *__restrict__ minv,
                                                 float *__restrict__ bias, float *__restrict__ gravity) {
  extern __shared__ float dyn_tri[]; // [3][W]: M, its Cholesky factor L, X = L^-1; each the packed lower triangles of the trees, one after the other
  __shared__ float sp[3 * 32], sq[4 * 32], sxi[3 * 32], scom[3 * 32], sI[10 * 32], sC[10 * 32], sU[6 * 32], sCC[6 * 32], sF[2 * 6 * 32];
  __shared__ float scdof[6 * FSIM_DYN_MAX_NV], sax[3 * FSIM_DYN_MAX_NV], sbg[2 * FSIM_DYN_MAX_NV];
  __shared__ int sanc[32], sdb[FSIM_DYN_MAX_NV], st0[FSIM_DYN_MAX_NV], st1[FSIM_DYN_MAX_NV], ssel[FSIM_DYN_MAX_NV];
  __shared__ unsigned ssub[32], sam[32];
  const int e = blockIdx.x, b = threadIdx.x;
  const float *rec = state + (size_t)e * a.kin.stride;
  float *Mt = dyn_tri, *Lt = dyn_tri + a.W, *Xt = dyn_tri + 2 * a.W;
  const bool want_m = mass || minv, want_b = bias != nullptr, want_f = bias || gravity;
  for (int d = b; d < a.nv; d += 64) { sdb[d] = a.dof_rbody[d]; st0[d] = a.tab[2 * d]; st1[d] = a.tab[2 * d + 1]; }
  for (int k = b; k < a.K; k += 64) ssel[k] = a.tab[2 * a.nv + k];
  // (A) + (B) the world pose of every reduced body, left in sp / sq: fsim_kin.hpp
  V3 P;
  Q4 Q;
  const KinLane l = kin_joint_pose(a.kin, rec, b, &P, &Q);
  kin_world_poses(a.kin, l, b, sp, sq, sanc, &P, &Q);
  // (C) inertial-frame origins; the subtree masks from the ancestor masks (which carry the self bit; a descendant's index is above its ancestor's)
  const M3 R = q2m(Q);
  if (b < a.kin.nr) {
    stv3(sp + 3 * b, P);
    stq(sq + 4 * b, Q);
    stv3(sxi + 3 * b, P + mulv(R, ldv3(a.r_ipos + 3 * l.bb)));
    unsigned sub = 0;
    for (int d = b; d < a.kin.nr; d++)
      if (b > 0 && (((unsigned)a.r_ancmask[d] >> b) & 1u)) sub |= 1u << d;
    ssub[b] = sub;
    sam[b] = (unsigned)a.r_ancmask[b];
  }
  __syncthreads();
  // (D) per-tree centre of mass
  for (int t = b; t < a.ntree; t += 64) {
    V3 s = v3(0, 0, 0);
    float tot = 0;
    const int b0 = a.tree_bodyadr[t], b1 = b0 + a.tree_bodynum[t];
    for (int k = b0; k < b1; k++) {
      const float ms = a.r_mass[k];
      s = s + ms * ldv3(sxi + 3 * k);
      tot += ms;
    }
    stv3(scom + 3 * t, tot > 0 ? s * (1.0f / tot) : ldv3(sp + 3 * b0));
  }
  __syncthreads();
  // (E) body inertias about the tree's centre of mass: Ixx Iyy Izz Ixy Ixz Iyz hx hy hz m (inert_mul's record); motion axes of every dof
  if (b < a.kin.nr) {
    float *I = sI + 10 * b;
    if (b == 0) {
      for (int k = 0; k < 10; k++) I[k] = 0.0f;
    } else {
      const float *ib = a.r_inertia + 6 * b; // xx yy zz xy xz yz in the body frame
      M3 Ib;
      Ib.m[0] = ib[0]; Ib.m[4] = ib[1]; Ib.m[8] = ib[2]; Ib.m[1] = Ib.m[3] = ib[3]; Ib.m[2] = Ib.m[6] = ib[4]; Ib.m[5] = Ib.m[7] = ib[5];
      const M3 T = mulm(R, Ib);
      float w[6];
      const int ij[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {0, 2}, {1, 2}};
      for (int k = 0; k < 6; k++) {
        const int i = ij[k][0], j = ij[k][1];
        w[k] = T.m[3 * i] * R.m[3 * j] + T.m[3 * i + 1] * R.m[3 * j + 1] + T.m[3 * i + 2] * R.m[3 * j + 2];
      }
      const float ms = a.r_mass[b];
      const V3 d = ldv3(sxi + 3 * b) - ldv3(scom + 3 * a.r_tree[b]);
      const float dd = dot(d, d);
      I[0] = w[0] + ms * (dd - d.x * d.x); I[1] = w[1] + ms * (dd - d.y * d.y); I[2] = w[2] + ms * (dd - d.z * d.z);
      I[3] = w[3] - ms * d.x * d.y; I[4] = w[4] - ms * d.x * d.z; I[5] = w[5] - ms * d.y * d.z;
      I[6] = ms * d.x; I[7] = ms * d.y; I[8] = ms * d.z; I[9] = ms;
    }
  }
  for (int d = b; d < a.nv; d += 64) {
    const int db = sdb[d], djt = a.kin.r_jtype[db], k = d - a.kin.r_dofadr[db];
    const V3 Pb = ldv3(sp + 3 * db), com = ldv3(scom + 3 * a.r_tree[db]);
    const Q4 Qb = ldq(sq + 4 * db);
    S6 s;
    s.a = v3(0, 0, 0);
    V3 axb = v3(0, 0, 0); // the dof's angular axis in its own body's frame
    if (djt == JT_FREE) {
      const V3 ax = v3(k % 3 == 0 ? 1.0f : 0.0f, k % 3 == 1 ? 1.0f : 0.0f, k % 3 == 2 ? 1.0f : 0.0f);
      if (k < 3) s.l = ax;
      else { axb = ax; s.a = qrot(Qb, ax); s.l = cross(s.a, com - Pb); }
    } else {
      const V3 axl = ldv3(a.kin.r_jaxis + 3 * db), ax = qrot(Qb, axl);
      if (djt == JT_SLIDE) s.l = ax;
      else { axb = axl; s.a = ax; s.l = cross(ax, com - (Pb + qrot(Qb, ldv3(a.kin.r_jpos + 3 * db)))); }
    }
    sts6(scdof + 6 * d, s);
    stv3(sax + 3 * d, axb);
  }
  __syncthreads();
  if (want_m) {
    // (F) composite inertias of the strict descendants
    if (b < a.kin.nr) {
      float acc[10];
      for (int k = 0; k < 10; k++) acc[k] = 0.0f;
      for (unsigned mm = ssub[b] & ~(1u << b); mm; mm &= mm - 1) {
        const float *I = sI + 10 * (__ffs(mm) - 1);
#pragma unroll
        for (int k = 0; k < 10; k++) acc[k] += I[k];
      }
      for (int k = 0; k < 10; k++) sC[10 * b + k] = acc[k];
    }
    __syncthreads();
    // (G) row i of the packed triangle of i's tree
    for (int i = b; i < a.nv; i += 64) {
      const int bi = sdb[i], a0 = st0[i] & 0xff, li = i - a0;
      const unsigned am = sam[bi];
      const S6 si = lds6(scdof + 6 * i);
      const S6 f = inert_mul(sC + 10 * bi, si);
      // body(i)'s own share, in its frame: its mass times the velocity of its centre of mass, its body-frame inertia times the dof's body-frame axis
      const V3 r = ldv3(sxi + 3 * bi) - ldv3(scom + 3 * a.r_tree[bi]), wi = ldv3(sax + 3 * i);
      const V3 mvi = (si.l + cross(si.a, r)) * a.r_mass[bi];
      const float *ib = a.r_inertia + 6 * bi; // xx yy zz xy xz yz
      const V3 Iwi = v3(ib[0] * wi.x + ib[3] * wi.y + ib[4] * wi.z, ib[3] * wi.x + ib[1] * wi.y + ib[5] * wi.z, ib[4] * wi.x + ib[5] * wi.y + ib[2] * wi.z);
      const Q4 qc = qconj(ldq(sq + 4 * bi));
      float *row = Mt + st1[i] + DYN_TRI(li);
      for (int lj = 0; lj <= li; lj++) {
        const int j = a0 + lj;
        float v = 0.0f;
        if ((am >> sdb[j]) & 1u) {
          const S6 sj = lds6(scdof + 6 * j);
          const V3 wj = sdb[j] == bi ? ldv3(sax + 3 * j) : qrot(qc, sj.a);
          v = dot6(sj, f) + dot(sj.l + cross(sj.a, r), mvi) + dot(wj, Iwi);
        }
        if (lj == li) v += a.dof_armature[i];
        row[lj] = v;
      }
    }
  }
  if (want_f) {
    // (H) body velocities U and velocity-product accelerations C by the chain rule (U, C) o (U', C') = (U + U', C + C' + U x U')
    S6 u = s6zero(), cc = s6zero();
    if (want_b) {
      if (l.on) {
        const int da = l.da;
        const float *qv = rec + a.kin.qvel + da;
        if (l.jt == JT_FREE) {
          S6 vt = s6zero();
#pragma unroll
          for (int t = 0; t < 3; t++) vt = vt + lds6(scdof + 6 * (da + t)) * qv[t];
          u = vt;
#pragma unroll
          for (int k = 3; k < 6; k++) {
            const S6 sk = lds6(scdof + 6 * (da + k));
            u = u + sk * qv[k];
            cc = cc + cross_motion(vt, sk) * qv[k];
          }
        } else
          u = lds6(scdof + 6 * da) * qv[0];
      }
      int anc = l.anc;
      for (int span = 1; span < a.kin.maxdepth; span <<= 1) {
        if (b < a.kin.nr) { sts6(sU + 6 * b, u); sts6(sCC + 6 * b, cc); sanc[b] = anc; }
        __syncthreads();
        if (anc > 0) {
          const S6 ua = lds6(sU + 6 * anc), ca = lds6(sCC + 6 * anc);
          const int na = sanc[anc];
          cc = ca + cc + cross_motion(ua, u);
          u = ua + u;
          anc = na;
        }
        __syncthreads();
      }
    }
    if (b < a.kin.nr) {
      S6 ag = s6zero();
      ag.l = v3(-a.g[0], -a.g[1], -a.g[2]);
      const float *I = sI + 10 * b;
      const S6 fg = inert_mul(I, ag); // (body 0: a zero record)
      sts6(sF + 6 * b, fg);
      if (want_b) sts6(sF + 6 * 32 + 6 * b, fg + (inert_mul(I, cc) + cross_force(u, inert_mul(I, u))));
    }
    __syncthreads();
    // one loop for both: w = 0 gravity, w = 1 bias
#pragma nounroll
    for (int w = 0; w < 2; w++) {
      if (w == 0 ? gravity == nullptr : bias == nullptr) continue;
      const float *F = sF + 6 * 32 * w;
      for (int d = b; d < a.nv; d += 64) {
        const S6 s_ = lds6(scdof + 6 * d);
        float acc = 0.0f;
        for (unsigned mm = ssub[sdb[d]]; mm; mm &= mm - 1) acc += dot6(s_, lds6(F + 6 * (__ffs(mm) - 1)));
        sbg[FSIM_DYN_MAX_NV * w + d] = acc + 0.0f; // (a zero is +0 on both sides)
      }
    }
  }
  __syncthreads();
  if (minv) {
    // (I) L of every tree at once, left-looking: in round k the lane of row i >= k of a tree computes L[i][k] from the columns before k;
    //     it recomputes the pivot itself (the same instructions on the same words in every lane), which saves a barrier per column
    for (int k = 0; k < a.maxn; k++) {
      for (int i = b; i < a.nv; i += 64) {
        const int w0 = st0[i], li = i - (w0 & 0xff), n = w0 >> 8;
        if (k >= n || li < k) continue;
        const int rowi = st1[i] + DYN_TRI(li), rowk = st1[i] + DYN_TRI(k);
        float s = Mt[rowi + k], p = Mt[rowk + k];
        for (int j = 0; j < k; j++) {
          const float lk = Lt[rowk + j];
          s -= Lt[rowi + j] * lk;
          p -= lk * lk;
        }
        const float piv = sqrtf(fmaxf(p, FS_MINVAL));
        Lt[rowi + k] = li == k ? piv : s / piv;
      }
      __syncthreads();
    }
    // (J) X = L^-1: lane = column c, down the rows; a lane reads back only what it wrote itself
    for (int c = b; c < a.nv; c += 64) {
      const int w0 = st0[c], lc = c - (w0 & 0xff), n = w0 >> 8, base = st1[c];
      for (int li = lc; li < n; li++) {
        const int rowi = base + DYN_TRI(li);
        const float inv = 1.0f / Lt[rowi + li];
        float s = 0.0f;
        for (int lj = lc; lj < li; lj++) s += Lt[rowi + lj] * Xt[base + DYN_TRI(lj) + lc];
        Xt[rowi + lc] = li == lc ? inv : -s * inv;
      }
    }
    __syncthreads();
  }
  // (K) the gather of the selected rows and columns
  const int K = a.K, KK = K * K;
  if (want_m) {
    float *om = mass ? mass + (size_t)e * KK : nullptr, *oi = minv ? minv + (size_t)e * KK : nullptr;
    for (int o = b; o < KK; o += 64) {
      const int r = o / K, c = o - r * K, i = ssel[r], j = ssel[c];
      const int hi = max(i, j), lo = min(i, j), a0 = st0[hi] & 0xff, n = st0[hi] >> 8, base = st1[hi];
      const bool same = a0 == (st0[lo] & 0xff);
      const int lh = hi - a0, ll = same ? lo - a0 : 0;
      if (om) om[o] = same ? Mt[base + DYN_TRI(lh) + ll] : 0.0f;
      if (oi) {
        float s = 0.0f;
        if (same)
          for (int k = lh; k < n; k++) s += Xt[base + DYN_TRI(k) + ll] * Xt[base + DYN_TRI(k) + lh];
        oi[o] = s;
      }
    }
  }
  if (gravity)
    for (int k = b; k < K; k += 64) gravity[(size_t)e * K + k] = sbg[ssel[k]];
  if (bias)
    for (int k = b; k < K; k += 64) bias[(size_t)e * K + k] = sbg[FSIM_DYN_MAX_NV + ssel[k]];
}

// ------------------------------------------------------------------------------------------ host
struct DynState {
  int K = 0, W = 0, maxn = 0;
  int *d_tab = nullptr; // DynArgs::tab
  DevTables tabs; // owns it
};

extern "C" int fsim_set_dynamics(fsim_t *s, int n_dofs, const int32_t *dofs) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_dynamics: null handle");
  if (n_dofs == 0) return sensor_clear(s, s->dyn);
  if (!dofs) FAIL(FSIM_EINVAL, "fsim_set_dynamics: null argument");
  const DModel &m = s->m;
  if (n_dofs < 1 || n_dofs > m.nv) FAIL(FSIM_EINVAL, "fsim_set_dynamics: %d dofs (1 .. nv = %d)", n_dofs, m.nv);
  if (m.nr > 32) FAIL(FSIM_EINVAL, "fsim_set_dynamics: %d reduced bodies (the dynamics pass holds at most 32)", m.nr);
  if (m.nv > FSIM_DYN_MAX_NV) FAIL(FSIM_EINVAL, "fsim_set_dynamics: nv = %d (the dynamics pass holds at most %d dofs)", m.nv, FSIM_DYN_MAX_NV);
  std::vector<char> seen(m.nv, 0);
  for (int i = 0; i < n_dofs; i++) {
    if (dofs[i] < 0 || dofs[i] >= m.nv) FAIL(FSIM_EINVAL, "fsim_set_dynamics: dof %d of the list is %d (the model has nv = %d)", i, dofs[i], m.nv);
    if (seen[dofs[i]]) FAIL(FSIM_EINVAL, "fsim_set_dynamics: dof %d is listed twice", dofs[i]);
    seen[dofs[i]] = 1;
  }
  std::vector<int> tadr, tnum, dtree;
  if (!blob_i(s->blob, "tree_dofadr", tadr) || !blob_i(s->blob, "tree_dofnum", tnum) || !blob_i(s->blob, "dof_tree", dtree)) return FSIM_EINVAL;
  if ((int)tadr.size() < m.ntree || (int)tnum.size() < m.ntree || (int)dtree.size() < m.nv) FAIL(FSIM_EINVAL, "fsim_set_dynamics: the model's tree tables are short");
  DynState c;
  c.K = n_dofs;
  std::vector<int> tbase(m.ntree, 0), tab((size_t)2 * m.nv + n_dofs, 0);
  for (int t = 0; t < m.ntree; t++) {
    if (tnum[t] < 0 || tnum[t] > 255 || tadr[t] < 0 || tadr[t] + tnum[t] > m.nv) FAIL(FSIM_EINVAL, "fsim_set_dynamics: tree %d holds dofs %d .. %d of %d", t, tadr[t], tadr[t] + tnum[t], m.nv);
    tbase[t] = c.W;
    c.W += tnum[t] * (tnum[t] + 1) / 2;
    c.maxn = std::max(c.maxn, tnum[t]);
  }
  for (int d = 0; d < m.nv; d++) {
    const int t = dtree[d];
    if (t < 0 || t >= m.ntree || d < tadr[t] || d >= tadr[t] + tnum[t]) FAIL(FSIM_EINVAL, "fsim_set_dynamics: dof %d is not among the dofs of its tree %d", d, t);
    tab[2 * d] = tadr[t] | (tnum[t] << 8);
    tab[2 * d + 1] = tbase[t];
  }
  for (int i = 0; i < n_dofs; i++) tab[2 * m.nv + i] = dofs[i];
  if ((size_t)12 * c.W > 40 * 1024) FAIL(FSIM_EINVAL, "fsim_set_dynamics: the trees' triangles take %d words (the dynamics pass holds 3 x 3413)", c.W);
  return sensor_install(s, "fsim_set_dynamics", s->dyn, c, [&](DevTables &t) { t.put(&c.d_tab, tab.data(), tab.size()); });
}

extern "C" int fsim_dynamics(fsim_t *s, float *mass_dev, float *minv_dev, float *bias_dev, float *gravity_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_dynamics: null handle");
  if (!s->dyn) FAIL(FSIM_EINVAL, "fsim_dynamics: no dof selection (fsim_set_dynamics)");
  if (!mass_dev && !minv_dev && !bias_dev && !gravity_dev) FAIL(FSIM_EINVAL, "fsim_dynamics: no output (mass, minv, bias and gravity all NULL)");
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const DynState &k = *s->dyn;
  const DModel &m = s->m;
  DynArgs da{kin_args(s), m.r_ancmask, m.r_tree, m.dof_rbody, m.tree_bodyadr, m.tree_bodynum, m.r_mass, m.r_ipos, m.r_inertia, m.dof_armature, k.d_tab,
             m.nv, m.ntree, k.K, k.W, k.maxn, {m.gravity[0], m.gravity[1], m.gravity[2]}};
  const size_t lds = 4 * (size_t)3 * k.W; // M, L and X: 1.8 KB for Sawyer + table_lack_0825, 4.1 KB for Baxter + table_liden_0921, at most 20 KB for 128 dofs in trees of 25
  hipLaunchKernelGGL(k_dynamics, dim3(s->n_envs), dim3(64), lds, s->stream, da, s->d_state, mass_dev, minv_dev, bias_dev, gravity_dev);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
