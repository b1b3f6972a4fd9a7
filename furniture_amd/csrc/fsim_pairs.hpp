// fsim_pairs.hpp -- geom-pair distance sensors (include/fsim_pairs.h).  Included at the end of fsim.hip, after fsim_probes.hpp: the host part
// launches k_cam_pose as it is, with an EMPTY mount table (no frames: the pose scratch holds the colliding geoms' world poses only); the
// distance kernel stages an env's geom table in k_cam_ray's staged layout, as k_probe_dist does, with the two hull-plane words of a row
// holding the geom's slice of the model's hull-vertex table instead (DModel::mesh_vert: the pair routine walks vertices, not planes).
//
// Two launches per fsim_pair_distance, both on the handle's stream:
//   k_cam_pose   (fsim_camera.hpp) one wave per env: world pose of every colliding geom;
//   k_pair_dist  256-thread workgroups of four INDEPENDENT waves, the shape of k_probe_dist.  A wave owns one (env, sensor): it stages the
//                env's geom rows in its own slice of LDS (one barrier per workgroup, nothing shared between the waves) and walks the
//                sensor's pair list -- built by the host in A-major order -- in chunks of 64, one pair per lane.
//                Prune, per chunk, with bounding spheres (c, rb: both centres lie inside their solids): lower bound lb = |c1 - c2| - rb1 -
//                rb2 (a plane: n . (c - p) - rb), upper bound ub = |c1 - c2| (a plane: n . (c - p)); a lane runs the pair routine
//                (fsim_gjk.hpp: gjk_pair) when lb <= min(best so far of the wave, smallest ub of the chunk, dmax) -- or when lb <= 0: two
//                bounding spheres that overlap may hold intersecting cores, whose portal answer may lie BELOW the true gap (the header's
//                contract) and so below lb; such pairs are never pruned, which keeps the winner the one an unpruned walk finds.  A pruned
//                pair has lb > 0, its cores are apart, its d is the exact one and d >= lb > the threshold: it would lose the strict <, or
//                win only to be refused by dmax.  The bounds carry the camera's slack (rb * 1.0001 + 1e-5), above the rounding of d.
//                A lane keeps the best of its own pairs (strict <: the earlier pair on a tie); the wave's winner is the smallest d, then
//                the smallest pair index, found with two DPP reductions.  No atomics, no scratch: every output word is written once, by
//                the winning lane (lane 0 when nothing is within dmax), and an env's output depends on nothing but its record and the
//                pair set.  The measurements: DESIGN.md 18.
#include "../../include/fsim_pairs.h"
#include "fsim_gjk.hpp"

#define PAIR_WAVES 4 // waves (units) per workgroup
enum { PRW_DMAX = 0, PRW_FIRST = 1, PRW_COUNT = 2, PRW_WORDS = 4 }; // d_sens rows (ints as float bits)

struct PairArgs { int ncg, nsens, pstride, nunits /* n_envs * nsens */; };

DEV Shape pair_shape(const float *Gg, MeshVerts mv) { // a staged geom row as the narrow phase's Shape
  Shape s;
  s.type = __float_as_int(Gg[CGW_TYPE]);
  s.pos = ldv3(Gg + CGW_POS);
  s.R = ldm3(Gg + CGW_MAT);
  s.size = ldv3(Gg + CGW_SIZE);
  s.verts = mv + 3 * __float_as_int(Gg[CGW_PADR]);
  s.nvert = __float_as_int(Gg[CGW_PNUM]);
  return s;
}

DEV float pair_wave_min(float v) { return -wave_max(-v); }

__global__ __launch_bounds__(64 * PAIR_WAVES) void k_pair_dist(PairArgs a, const float *__restrict__ pose, const float *__restrict__ cgtab,
                                                                const float *__restrict__ mesh_vert, const float *__restrict__ senstab,
                                                                const int *__restrict__ pairs /* g1 | g2 << 8 */, float *__restrict__ dist,
                                                                int *__restrict__ geoms, float *__restrict__ fromto, float *__restrict__ normal) {
  extern __shared__ __attribute__((aligned(16))) float pair_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  float *G = pair_lds + CAM_GW * a.ncg * w; // [ncg][CAM_GW], this wave's
  const int u = blockIdx.x * PAIR_WAVES + w;
  const bool live = u < a.nunits; // (the last workgroup may hold waves without a unit)
  const int e = live ? u / a.nsens : 0, sn = live ? u % a.nsens : 0;
  const float *P = pose + (size_t)e * a.pstride;
  if (live) {
    for (int i = lane; i < CAM_PW * a.ncg; i += 64) G[CAM_GW * (i / CAM_PW) + i % CAM_PW] = P[i];
    for (int i = lane; i < CAM_SW * a.ncg; i += 64) G[CAM_GW * (i / CAM_SW) + CAM_PW + i % CAM_SW] = cgtab[i];
  }
  __syncthreads();
  if (!live) return;
  const float *S = senstab + PRW_WORDS * sn;
  const float dmax = S[PRW_DMAX];
  const int first = __float_as_int(S[PRW_FIRST]), cnt = __float_as_int(S[PRW_COUNT]);
  const MeshVerts mv = GP(mesh_vert);
  float bd = CAM_INF, wbest = CAM_INF; // this lane's best, the wave's best so far
  int bi = -1, bg = 0;
  V3 bn = v3(0.0f, 0.0f, 0.0f), bf = bn, bt = bn;
  for (int c0 = 0; c0 < cnt; c0 += 64) {
    const int i = c0 + lane;
    const bool has = i < cnt;
    const int pk = pairs[first + min(i, cnt - 1)];
    const float *G1 = G + CAM_GW * (pk & 0xff), *G2 = G + CAM_GW * (pk >> 8);
    const int t1 = __float_as_int(G1[CGW_TYPE]), t2 = __float_as_int(G2[CGW_TYPE]);
    const V3 c = ldv3(G2 + CGW_POS) - ldv3(G1 + CGW_POS);
    float lb, ub; // (at most one of the two is a plane)
    if (t1 == GT_PLANE) { ub = dot(colv(ldm3(G1 + CGW_MAT), 2), c); lb = ub - (G2[CGW_RB] * 1.0001f + 1e-5f); }
    else if (t2 == GT_PLANE) { ub = -dot(colv(ldm3(G2 + CGW_MAT), 2), c); lb = ub - (G1[CGW_RB] * 1.0001f + 1e-5f); }
    else { ub = norm(c); lb = ub - (G1[CGW_RB] * 1.0001f + 1e-5f) - (G2[CGW_RB] * 1.0001f + 1e-5f); }
    ub = has ? ub + fabsf(ub) * 1e-4f + 1e-5f : CAM_INF;
    const float thr = fminf(fminf(wbest, pair_wave_min(ub)), dmax);
    float d = CAM_INF;
    if (has && (lb <= 0.0f || lb <= thr)) {
      const PairOut o = gjk_pair<true>(pair_shape(G1, mv), pair_shape(G2, mv));
      d = o.d;
      if (d < bd) { bd = d; bi = i; bg = pk; bn = o.n; bf = o.from; bt = o.to; }
    }
    wbest = fminf(wbest, pair_wave_min(d));
  }
  // the wave's winner: the smallest d, then the smallest pair index (pair indices are below 4096: exact as floats)
  const float dmin = pair_wave_min(bd);
  const bool tie = bi >= 0 && bd == dmin;
  const int imin = (int)pair_wave_min(tie ? (float)bi : 1.0e9f);
  const bool hit = dmin <= dmax;
  const size_t out = (size_t)e * a.nsens + sn;
  if (hit ? (tie && bi == imin) : lane == 0) {
    if (dist) dist[out] = hit ? bd : dmax;
    if (geoms) {
      geoms[2 * out] = hit ? __float_as_int(G[CAM_GW * (bg & 0xff) + CGW_ID]) : -1;
      geoms[2 * out + 1] = hit ? __float_as_int(G[CAM_GW * (bg >> 8) + CGW_ID]) : -1;
    }
    const V3 z = v3(0.0f, 0.0f, 0.0f);
    if (fromto) { stv3(fromto + 6 * out, hit ? bf : z); stv3(fromto + 6 * out + 3, hit ? bt : z); }
    if (normal) stv3(normal + 3 * out, hit ? bn : z);
  }
}

// ------------------------------------------------------------------------------------------ host
struct PairState {
  int nsens = 0, npairs = 0, pstride = 0;
  float *d_cg = nullptr, *d_sens = nullptr, *d_pose = nullptr;
  int *d_pairs = nullptr;
  DevTables tabs; // owns them
};

// What a set of pair sensors becomes on the host: the d_sens rows, the pair lists (A-major) and the static geom rows k_pair_dist stages,
// with the words of one pose-scratch row.  Validated here for fsim_set_pairs and fsim_set_clearance (fsim_clearance.hpp) alike; who:
// the caller's name for the messages.
struct PairTables {
  std::vector<float> srow, cg;
  std::vector<int> pairs;
  int pstride = 0;
};

static int pair_tables(const fsim *s, const char *who, int n_sensors, const fsim_pair_sensor_t *sensors, PairTables &pt) {
  if (!sensors) FAIL(FSIM_EINVAL, "%s: null argument", who);
  if (n_sensors < 1 || n_sensors > FSIM_PAIR_MAX_SENSORS) FAIL(FSIM_EINVAL, "%s: %d sensors (1 .. %d)", who, n_sensors, FSIM_PAIR_MAX_SENSORS);
  const DModel &m = s->m;
  if (m.ncg > FSIM_CAM_MAX_GEOMS) FAIL(FSIM_EINVAL, "%s: %d colliding geoms (the distance pass stages at most %d)", who, m.ncg, FSIM_CAM_MAX_GEOMS);
  CamMountTables mt;
  { int rc_ = cam_mount_tables(s, mt); if (rc_) return rc_; }
  std::vector<int> madr, mnum; // convex-mesh colliders' slices of the hull-vertex table (absent = none)
  blob_i(s->blob, "cg_meshadr", madr); blob_i(s->blob, "cg_meshnum", mnum);
  std::vector<float> &srow = pt.srow, &cg = pt.cg;
  std::vector<int> &pairs = pt.pairs;
  srow.assign((size_t)PRW_WORDS * n_sensors, 0.0f);
  pairs.clear();
  for (int i = 0; i < n_sensors; i++) {
    const fsim_pair_sensor_t &k = sensors[i];
    if (!(k.dmax > 0.0f) || !std::isfinite(k.dmax)) FAIL(FSIM_EINVAL, "pair sensor %d: needs 0 < dmax < inf (got %g)", i, k.dmax);
    for (int g = m.ncg; g < 96; g++)
      if (((k.a[g >> 5] | k.b[g >> 5]) >> (g & 31)) & 1u) FAIL(FSIM_EINVAL, "pair sensor %d: mask bit %d set (the model has %d colliding geoms)", i, g, m.ncg);
    if (!(k.a[0] | k.a[1] | k.a[2])) FAIL(FSIM_EINVAL, "pair sensor %d: side A is empty", i);
    if (!(k.b[0] | k.b[1] | k.b[2])) FAIL(FSIM_EINVAL, "pair sensor %d: side B is empty", i);
    const size_t first = pairs.size();
    for (int g1 = 0; g1 < m.ncg; g1++) {
      if (!((k.a[g1 >> 5] >> (g1 & 31)) & 1u)) continue;
      for (int g2 = 0; g2 < m.ncg; g2++)
        if (((k.b[g2 >> 5] >> (g2 & 31)) & 1u) && g1 != g2 && !(mt.cg_type[g1] == GT_PLANE && mt.cg_type[g2] == GT_PLANE)) pairs.push_back(g1 | (g2 << 8));
    }
    const size_t cnt = pairs.size() - first;
    if (cnt == 0) FAIL(FSIM_EINVAL, "pair sensor %d: no valid pair (every pair of its sides is a geom with itself or two planes)", i);
    if (cnt > FSIM_PAIR_MAX_PAIRS) FAIL(FSIM_EINVAL, "pair sensor %d: %zu pairs (at most %d per sensor)", i, cnt, FSIM_PAIR_MAX_PAIRS);
    if (pairs.size() > FSIM_PAIR_MAX_TOTAL) FAIL(FSIM_EINVAL, "%s: more than %d pairs over the set (sensor %d brings it to %zu)", who, FSIM_PAIR_MAX_TOTAL, i, pairs.size());
    float *r = srow.data() + PRW_WORDS * i;
    r[PRW_DMAX] = k.dmax; r[PRW_FIRST] = cam_bits((int)first); r[PRW_COUNT] = cam_bits((int)cnt);
  }
  // the static rows of cam_geom_rows, with a hull's vertex slice where that has its plane slice
  cg.assign((size_t)CAM_SW * m.ncg, 0.0f);
  std::vector<float> mvert;
  blob_f(s->blob, "mesh_vert", mvert);
  const size_t nvert = mvert.size() / 3;
  for (int g = 0; g < m.ncg; g++) {
    float *r = cg.data() + CAM_SW * g;
    for (int j = 0; j < 3; j++) r[j] = mt.cg_size[3 * g + j];
    r[3] = mt.cg_rbound[g];
    int adr = 0, num = 0;
    if (mt.cg_type[g] == GT_MESH) {
      if ((size_t)g >= madr.size() || (size_t)g >= mnum.size()) FAIL(FSIM_EINVAL, "%s: colliding geom %d is a convex mesh and the model has no hull vertices for it", who, g);
      adr = madr[g]; num = mnum[g];
      if (num < 4 || adr < 0 || (size_t)adr + num > nvert) FAIL(FSIM_EINVAL, "%s: hull vertices of colliding geom %d out of range (%d + %d of %zu)", who, g, adr, num, nvert);
    }
    r[4] = cam_bits(mt.cg_type[g]); r[5] = cam_bits(adr); r[6] = cam_bits(num); r[7] = cam_bits(mt.cg_orig[g]);
  }
  pt.pstride = (CAM_PW * m.ncg + 3) / 4 * 4;
  return FSIM_OK;
}

extern "C" int fsim_set_pairs(fsim_t *s, int n_sensors, const fsim_pair_sensor_t *sensors) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_pairs: null handle");
  if (n_sensors == 0) return sensor_clear(s, s->pair);
  PairTables pt;
  { int rc_ = pair_tables(s, "fsim_set_pairs", n_sensors, sensors, pt); if (rc_) return rc_; }
  PairState c;
  c.nsens = n_sensors;
  c.npairs = (int)pt.pairs.size();
  c.pstride = pt.pstride;
  return sensor_install(s, "fsim_set_pairs", s->pair, c, [&](DevTables &t) {
    t.put(&c.d_sens, pt.srow.data(), pt.srow.size());
    t.put(&c.d_pairs, pt.pairs.data(), pt.pairs.size());
    t.put(&c.d_cg, pt.cg.data(), pt.cg.size());
    t.put(&c.d_pose, nullptr, (size_t)s->n_envs * std::max(c.pstride, 4));
  });
}

// One k_pair_dist launch over `rows` pose rows of `pose` (an env each for fsim_pair_distance, an (env, candidate) each for fsim_clearance);
// the outputs are [rows][nsens]...
static int pair_launch(fsim *s, const char *who, size_t rows, int nsens, int pstride, const float *pose, const float *d_cg, const float *d_sens, const int *d_pairs,
                       float *dist_dev, int32_t *geoms_dev, float *fromto_dev, float *normal_dev) {
  const DModel &m = s->m;
  PairArgs ra{};
  ra.ncg = m.ncg; ra.nsens = nsens; ra.pstride = pstride;
  const size_t nunits = rows * nsens, nblk = (nunits + PAIR_WAVES - 1) / PAIR_WAVES;
  if (nunits > 0x7fffffff) FAIL(FSIM_EINVAL, "%s: %zu units", who, nunits);
  ra.nunits = (int)nunits;
  const size_t lds = 4 * (size_t)PAIR_WAVES * CAM_GW * m.ncg; // at most 30 KB (96 geoms)
  hipLaunchKernelGGL(k_pair_dist, dim3((unsigned)nblk), dim3(64 * PAIR_WAVES), lds, s->stream, ra, pose, d_cg, m.mesh_vert, d_sens, d_pairs, dist_dev, geoms_dev,
                     fromto_dev, normal_dev);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}

extern "C" int fsim_pair_distance(fsim_t *s, float *dist_dev, int32_t *geoms_dev, float *fromto_dev, float *normal_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_pair_distance: null handle");
  if (!s->pair) FAIL(FSIM_EINVAL, "fsim_pair_distance: no pair set (fsim_set_pairs)");
  if (!dist_dev && !geoms_dev && !fromto_dev && !normal_dev) FAIL(FSIM_EINVAL, "fsim_pair_distance: no output (distance, geoms, fromto and normal all NULL)");
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const PairState &k = *s->pair;
  hipLaunchKernelGGL(k_cam_pose, dim3(s->n_envs), dim3(64), 0, s->stream, cam_pose_args(s, 0 /* no frames */, k.pstride), s->d_state, (const float *)nullptr, k.d_pose);
  HIPCHK(hipGetLastError());
  return pair_launch(s, "fsim_pair_distance", (size_t)s->n_envs, k.nsens, k.pstride, k.d_pose, k.d_cg, k.d_sens, k.d_pairs, dist_dev, geoms_dev, fromto_dev, normal_dev);
}
