/* fsim_dynamics.h -- joint-space inertia, its inverse and the bias forces of libfsim.so, computed on the device (a C-ABI of its own beside
 * fsim.h, fsim_camera.h, fsim_points.h, fsim_voxels.h, fsim_normals.h, fsim_flow.h, fsim_rays.h, fsim_probes.h, fsim_pairs.h and
 * fsim_frames.h).
 *
 * The dynamics half of a user-side operational-space controller, tau = J^T Lambda a* + bias with Lambda = (J M^-1 J^T)^-1: MuJoCo's
 * mj_fullM, mj_solveM and data.qfrc_bias for every env, next to the Jacobians of fsim_frames.h.  The quantities are a pure function of
 * qpos / qvel of the env record; they need no cameras, rays, probes, pairs, frames or solver state and disturb none of them.
 *
 * Selection.  The outputs are restricted to a list d of K distinct dofs, in the caller's order (the seven dofs of an arm, say).
 *
 * Outputs, per env (K selected dofs), all float32:
 *   mass     [n_envs][K][K]  M[d][:, d].  M is the joint-space inertia of the reduced model at the record's qpos with dof_armature on
 *                            the diagonal (mj_fullM).  Symmetric bit for bit.  An entry whose two dofs are in different kinematic trees,
 *                            or in one tree with neither dof's body an ancestor-or-self of the other's, is exactly 0.0f.
 *   minv     [n_envs][K][K]  (M^-1)[d][:, d]: the inverse of the WHOLE M restricted to the selection, not the inverse of the selected
 *                            block, so that J M^-1 J^T of a Jacobian supported on d is exact.  Symmetric bit for bit; exactly 0.0f
 *                            across kinematic trees.
 *   bias     [n_envs][K]     qfrc_bias[d] at the record's qpos, qvel: Coriolis, centrifugal and gravity forces (RNE with zero
 *                            acceleration).
 *   gravity  [n_envs][K]     the same at qvel = 0: the generalised gravity force; -gravity is what a gravity-compensating torque must
 *                            cancel.  At qvel = 0, bias equals gravity bit for bit.
 *
 * Free joints follow fsim_flow.h's rule: qvel[0:3] is the world velocity of the body origin and qvel[3:6] the angular velocity in the
 * body's own frame.  The record's part quaternions are normalised by the kernel.  Welds and contacts are constraints and do not enter M;
 * Cursor bodies have no dofs and contribute nothing.
 *
 * No side effects: fsim_dynamics writes no state, RNG draw, look-ahead shadow or counter.  An env's output depends only on its own record
 * and the selection, never on the batch around it; an entry's bits depend only on its own one or two dofs, not on the rest of the
 * selection or on its order; an output's bits do not depend on which other outputs are asked for.  Without a selection, nothing is
 * allocated or launched.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_DYNAMICS_H
#define FSIM_DYNAMICS_H
#include "fsim.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FSIM_DYN_MAX_NV 128 /* dofs of the model */

/* Replace the handle's dof selection: n_dofs = 1 .. nv distinct dof indices in [0, nv), in any order.  n_dofs == 0 clears the selection
 * and frees its table (the other argument is ignored).  Host pointer, copied before return; the call settles the handle and waits for its
 * stream before it replaces the table.  FSIM_EINVAL, each with a message: a null handle or null list, n_dofs outside 1 .. nv, an index out
 * of range, a duplicate, a model with more than 32 reduced bodies, nv above 128.  A refused call leaves the previous selection in place. */
int fsim_set_dynamics(fsim_t *, int n_dofs, const int32_t *dofs);

/* The dynamics tensors of every env: mass_dev float32 [n_envs][K][K], minv_dev float32 [n_envs][K][K], bias_dev float32 [n_envs][K],
 * gravity_dev float32 [n_envs][K] (any may be NULL, not all; what is not asked for is not computed).  Works in the state fsim_sync leaves,
 * settled exactly as fsim_frame_state settles it (a step in flight is waited for and the overflow re-step ladder runs first); then one
 * launch is enqueued on the handle's stream and the call returns without waiting for it.  Reads the env records and writes nothing but the
 * outputs.  FSIM_EINVAL: null handle, no selection, all four pointers NULL. */
int fsim_dynamics(fsim_t *, float *mass_dev, float *minv_dev, float *bias_dev, float *gravity_dev);

#ifdef __cplusplus
}
#endif
#endif
