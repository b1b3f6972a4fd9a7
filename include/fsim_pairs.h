/* fsim_pairs.h -- geom-pair distance sensors of libfsim.so, computed on the device (a C-ABI of its own beside fsim.h, fsim_camera.h,
 * fsim_points.h, fsim_voxels.h, fsim_normals.h, fsim_flow.h, fsim_rays.h and fsim_probes.h).
 *
 * A pair sensor has two sets of colliding geoms, side A and side B, and a largest distance dmax in metres.  It answers: how far is the
 * nearest geom of A from the nearest geom of B, which two geoms are they, where are the two nearest points and along which direction is
 * the distance measured -- MuJoCo's distance / normal / fromto sensors (mj_geomDistance with geom1 / geom2 or body1 / body2): gripper to a
 * table leg, a leg to the table top, the arm links to every part, the gripper to the floor.  The query is geometric: collision masks
 * (contype / conaffinity) are ignored, geoms of one body or of welded bodies are NOT skipped, and a geom may be on both sides.  The sensors
 * see the collision geometry the cameras, rays and probes see; they need none of them and disturb none of them.
 *
 * Pair.  A pair of a sensor is (g1 in A, g2 in B) with g1 != g2 and not both planes.  The pairs are ordered A-major: by g1, then by g2,
 * both in colliding-geom order (the order of the model's cg_orig table).
 *
 * Contract per pair: the signed distance d, the unit normal n (from A to B: the direction along which d is measured) and the witness
 * points `from` (on g1) and `to` (on g2), to - from = d * n.
 *   Planes.  For a pair with a plane (normal n_p, point p_plane, X the other geom, h_X its support value):
 *       d = -h_X(-n_p) - n_p . p_plane,
 *     the height of X's lowest point over the plane, exact for either sign.  n = n_p when the plane is g1, -n_p when it is g2; the
 *     witness on X is its lowest point, the witness on the plane the foot of that point.
 *   Radii.  A sphere is its centre plus a radius, a capsule its axis segment plus a radius: their CORE is the point / the segment.  A
 *     box, a cylinder and a convex hull (the hull vertices of the model) are their own core, with radius 0.
 *   Cores apart.  While the two cores are disjoint, d is the Euclidean distance of the cores minus the two radii -- exact also when that
 *     is negative (two spheres or capsules that overlap by less than their radii).  It is computed by an fp32 GJK distance iteration on
 *     the cores, which stops when the distance along the current direction is within 1e-6 m + 1e-5 d_core of the distance found (or
 *     after 40 iterations).  n is the iteration's final unit direction -- never a normalised to - from, which has no direction left when
 *     the two points nearly coincide.  from / to are the nearest points of the cores moved by the radii along n.
 *   Cores intersecting.  The answer is the portal routine's (np_mpr, the routine the step's narrow phase runs for its portal pairs,
 *     here on the two whole solids): d is MINUS THE PORTAL DEPTH, and so
 *       d <= the true signed gap (minus the smallest translation that separates the two solids):
 *     the routine reports the distance to the face of the Minkowski difference that the line through the two centres leaves through,
 *     not to the nearest face, so it never reports a shallower overlap than the true one and may report a deeper one.  By how much has
 *     been measured against exact geometry, per pair type: the table PORTAL_OVER_FP64 of tests/test_narrowphase.py (nothing for a
 *     cylinder standing on a box, 1.9 cm for two parallel cylinders side by side).  For two boxes this is NOT the depth the step's
 *     closed-form box-box routine (np_box_box) uses for its contacts.  n is the portal's normal; from / to are the portal's contact
 *     position moved by -d / 2 and +d / 2 along n.
 *
 * Contract per sensor.  Over its pairs the smallest d wins; a strict < in pair order (A-major) settles ties: of equal distances the
 * first pair wins.  The winner is accepted when d <= dmax; the outputs are then the winner's.  Otherwise dist = dmax, geoms = (-1, -1)
 * and the vectors are (0, 0, 0) (MuJoCo's distmax convention).
 *
 * Outputs, per env and sensor (S sensors):
 *   dist    float32 [n_envs][S]      the signed distance in metres, negative when the two geoms overlap; dmax when nothing is within dmax.
 *   geoms   int32   [n_envs][S][2]   the MODEL geom ids (g1 of side A, g2 of side B) in the numbering of the segmentation image of
 *                                    fsim_camera.h; (-1, -1) when nothing is within dmax.
 *   fromto  float32 [n_envs][S][6]   world points: from (on g1), then to (on g2).
 *   normal  float32 [n_envs][S][3]   world-frame unit vector from A to B.
 *
 * No side effects: fsim_pair_distance writes no state, RNG draw, look-ahead shadow or counter.  An env's output depends only on its own
 * record and the pair set, never on the batch around it; a sensor's output does not depend on the other sensors of the set.  Without a
 * pair set, nothing is allocated or launched.
 *
 * Same conventions as fsim.h: 0 or a negative FSIM_* code with a message in fsim_last_error(); device pointers are raw HIP addresses;
 * work is enqueued on the handle's stream.
 */
#ifndef FSIM_PAIRS_H
#define FSIM_PAIRS_H
#include "fsim.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FSIM_PAIR_MAX_SENSORS 64
#define FSIM_PAIR_MAX_PAIRS 4096   /* per sensor */
#define FSIM_PAIR_MAX_TOTAL 16384  /* over the set */

typedef struct fsim_pair_sensor {
  uint32_t a[3], b[3]; /* bit k: colliding geom k (cg_orig order) belongs to side A / side B */
  float dmax;          /* metres: 0 < dmax < inf */
} fsim_pair_sensor_t;

/* Replace the handle's pair set: n_sensors = 1 .. FSIM_PAIR_MAX_SENSORS sensors.  n_sensors == 0 clears the set and frees its tables (the
 * other argument is ignored).  The hull vertices of convex-mesh colliders come from the model, so no plane tables are passed.  Host
 * pointer, copied before return; the call waits for the handle's stream before it replaces the tables.  FSIM_EINVAL, each with a message:
 * more than 64 sensors, more than 4096 pairs in a sensor or 16384 over the set, a side without a geom, a sensor with no valid pair (every
 * (g1, g2) has g1 == g2 or two planes), a mask bit at or beyond the number of colliding geoms, a dmax that is not 0 < dmax < inf, a model
 * with more than 96 colliding geoms.  A refused call leaves the previous set in place. */
int fsim_set_pairs(fsim_t *, int n_sensors, const fsim_pair_sensor_t *sensors);

/* The distance of every sensor of every env: dist_dev float32 [n_envs][S], geoms_dev int32 [n_envs][S][2], fromto_dev float32
 * [n_envs][S][6], normal_dev float32 [n_envs][S][3] (any may be NULL, not all).  Works in the state fsim_sync leaves, settled exactly as
 * fsim_probe_distance settles it (a step in flight is waited for and the overflow re-step ladder runs first); then two launches are
 * enqueued on the handle's stream (poses, distances) and the call returns without waiting for them.  Reads the env records and writes
 * nothing but the outputs and a pose scratch the pair set owns.  FSIM_EINVAL: null handle, no pair set, all four pointers NULL. */
int fsim_pair_distance(fsim_t *, float *dist_dev, int32_t *geoms_dev, float *fromto_dev, float *normal_dev);

#ifdef __cplusplus
}
#endif
#endif
