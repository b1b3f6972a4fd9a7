// fsim_kin.hpp -- the body-pose and twist stages the read-only one-wave-per-env kernels share: k_cam_pose (fsim_camera.hpp), k_cam_twist
// (fsim_flow.hpp), k_frame_state (fsim_frames.hpp), k_dynamics (fsim_dynamics.hpp) and k_momenta (fsim_momentum.hpp).  Included by fsim.hip
// ahead of fsim_camera.hpp.  Plain functions, called directly and inlined into each kernel (DEV); lane b of the wave is reduced body b, and a
// model has at most 32 of them.  The arithmetic is that of the step's fs_kinematics (pointer doubling up the reduced tree, qnormalized on
// free joints and on every composition); the record is never written: the free-joint quaternion is normalised in registers, as
// fs_kinematics does in LDS.  What was measured when the five copies became this file, and why it has this shape: DESIGN.md 16b.
//   (A) kin_joint_pose   the pose of every reduced body in its parent, and the lane's joint constants for the stages after it;
//   (B) kin_world_poses  the world poses, by pointer doubling up the tree;
//   (T) kin_joint_twist  the body's own joint twist about the WORLD ORIGIN, so that the twists of a chain add;
//   (U) kin_sum_twists   their sum up the tree, by pointer doubling as (B), left in LDS.
// k_dynamics' stage (H) and k_momenta's chain sum spatial vectors about a per-tree reference point in scratch of their own: they stay there.

struct KinArgs {
  const int *r_parent, *r_jtype, *r_qposadr, *r_dofadr;
  const float *r_pos, *r_quat, *r_jaxis, *r_jpos;
  int nr, maxdepth, stride, qpos /* offsets of qpos and qvel in the record */, qvel;
};

// what (A) leaves in lane b for the later stages: the body is a moving one (on; bb = b then, else 0), its joint type, first dof, where
// a pointer doubling starts (anc: the parent of a moving body, else 0), and the joint's anchor and axis in the body's frame
struct KinLane {
  bool on;
  int bb, jt, da, anc;
  V3 jpos, jax;
};

DEV KinLane kin_joint_pose(const KinArgs &a, const float *rec, int b, V3 *Pout, Q4 *Qout) {
  KinLane l;
  l.on = b < a.nr && b > 0;
  l.bb = l.on ? b : 0;
  const int bb = l.bb, qa = a.r_qposadr[bb], parent = a.r_parent[bb];
  l.jt = a.r_jtype[bb]; l.da = a.r_dofadr[bb];
  l.jpos = ldv3(a.r_jpos + 3 * bb); l.jax = ldv3(a.r_jaxis + 3 * bb);
  V3 P = v3(0, 0, 0);
  Q4 Q = q4(1, 0, 0, 0);
  if (l.on) {
    if (l.jt == JT_FREE) {
      P = ldv3(rec + a.qpos + qa);
      Q = qnormalized(ldq(rec + a.qpos + qa + 3));
    } else {
      const Q4 q0 = ldq(a.r_quat + 4 * bb);
      const V3 p0 = ldv3(a.r_pos + 3 * bb);
      const V3 al = p0 + qrot(q0, l.jpos), axl = qrot(q0, l.jax);
      const float q = rec[a.qpos + qa];
      if (l.jt == JT_SLIDE) { Q = q0; P = p0 + axl * q; }
      else { Q = qmul(q0, axisangle(l.jax, q)); P = al - qrot(Q, l.jpos); }
    }
  }
  // Keep this line HERE, right behind the branch on l.on.  Computed at the head of (B) and (U) instead, the same value reaches their
  // loops as a select and not as a phi out of that branch: k_cam_twist then takes 48 VGPRs for 46 and orders its floating-point
  // instructions differently (gfx950, ROCm's clang of this tree).  The outputs are pinned bit for bit only by
  // profiles/kin_a_bit_identity.txt, so after moving it, or after a compiler upgrade, compare the assembly and the bits again.
  l.anc = l.on ? parent : 0;
  *Pout = P; *Qout = Q;
  return l;
}

// (P, Q): in, the lane's pose in its parent; out, in the world.  sp [32][3], sq [32][4] and sanc [32] are the loop's scratch: on
// return they do NOT hold the final poses.  A caller that reads poses from LDS afterwards stores its (P, Q) itself,
//   if (b < a.nr) { stv3(sp + 3 * b, P); stq(sq + 4 * b, Q); }
// BEHIND this call and not depending on the loop having run, and puts its barrier behind the store.  Forgetting it shows only where
// every moving body is a root (maxdepth 1: the Cursor): the loop never runs there and that store is the only write.  (The store is
// not in here, unlike kin_sum_twists' own: k_cam_twist reads no pose from LDS, and k_dynamics and k_momenta fold it into their next
// block, where moving it changed k_momenta's floating-point instructions.  DESIGN.md 16b.)
DEV void kin_world_poses(const KinArgs &a, const KinLane &l, int b, float *sp, float *sq, int *sanc, V3 *Pio, Q4 *Qio) {
  V3 P = *Pio;
  Q4 Q = *Qio;
  int anc = l.anc;
  for (int span = 1; span < a.maxdepth; span <<= 1) {
    if (b < a.nr) { stv3(sp + 3 * b, P); stq(sq + 4 * b, Q); sanc[b] = anc; }
    __syncthreads();
    if (anc > 0) {
      const V3 pa = ldv3(sp + 3 * anc);
      const Q4 qa_ = ldq(sq + 4 * anc);
      const int na = sanc[anc];
      P = pa + qrot(qa_, P);
      Q = qnormalized(qmul(qa_, Q));
      anc = na;
    }
    __syncthreads();
  }
  *Pio = P; *Qio = Q;
}

// w, and v0 = the velocity of the body-fixed point that is at the world origin now.  A twist about one common point is a plain
// 6-vector: those of a chain add.  (P, Q) is the body's world pose; a hinge or slide axis is the same in the body's frame before and
// after its own joint moved, so R_b axis needs no parent.
DEV void kin_joint_twist(const KinArgs &a, const KinLane &l, const float *rec, V3 P, Q4 Q, V3 *v0out, V3 *wout) {
  V3 w = v3(0, 0, 0), v0 = v3(0, 0, 0);
  if (l.on) {
    const float *qv = rec + a.qvel + l.da;
    if (l.jt == JT_FREE) { // qvel[0:3]: world velocity of the body origin; qvel[3:6]: angular velocity in the body's own frame
      w = qrot(Q, ldv3(qv + 3));
      v0 = ldv3(qv) - cross(w, P);
    } else if (l.jt == JT_SLIDE) {
      v0 = qrot(Q, l.jax) * qv[0];
    } else { // hinge, about the anchor x_b + R_b jpos
      w = qrot(Q, l.jax) * qv[0];
      v0 = cross(P + qrot(Q, l.jpos), w);
    }
  }
  *v0out = v0; *wout = w;
}

// (v0, w): the lane's own twist, summed with its ancestors' (plain sums, as fs_velocity_bias sums its spatial velocities) and stored in
// sv / sw [32][3], the store standing behind the loop as above.  The caller's barrier follows.
DEV void kin_sum_twists(const KinArgs &a, const KinLane &l, int b, float *sv, float *sw, int *sanc, V3 v0, V3 w) {
  int anc = l.anc;
  for (int span = 1; span < a.maxdepth; span <<= 1) {
    if (b < a.nr) { stv3(sv + 3 * b, v0); stv3(sw + 3 * b, w); sanc[b] = anc; }
    __syncthreads();
    if (anc > 0) {
      const V3 va = ldv3(sv + 3 * anc), wa = ldv3(sw + 3 * anc);
      const int na = sanc[anc];
      v0 = va + v0;
      w = wa + w;
      anc = na;
    }
    __syncthreads();
  }
  if (b < a.nr) { stv3(sv + 3 * b, v0); stv3(sw + 3 * b, w); }
}

// ------------------------------------------------------------------------------------------ host
static KinArgs kin_args(const fsim *s) {
  const DModel &m = s->m;
  return KinArgs{m.r_parent, m.r_jtype, m.r_qposadr, m.r_dofadr, m.r_pos, m.r_quat, m.r_jaxis, m.r_jpos, m.nr, m.maxdepth, s->ly.stride, s->ly.qpos, s->ly.qvel};
}
