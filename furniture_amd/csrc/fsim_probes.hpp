// fsim_probes.hpp -- signed-distance proximity probes (include/fsim_probes.h).  Included at the end of fsim.hip, after fsim_rays.hpp: the
// host part launches k_cam_pose as it is, with the probe sensors' own mount table (rows of the CCW_* layout) and a pose scratch the probe
// set owns; the distance kernel stages an env's geom table and the hull planes in k_cam_ray's staged layout, as k_ray_cast does.
//
// Two launches per fsim_probe_distance, both on the handle's stream:
//   k_cam_pose    (fsim_camera.hpp) one wave per env: world pose of every colliding geom and of every sensor frame;
//   k_probe_dist  256-thread workgroups of four INDEPENDENT waves, the shape of k_ray_cast and for its reasons ("Workgroup
//                 shape").  A wave takes one unit: up to PRB_JPW consecutive jobs of one env, a job being up to 64 consecutive probes of
//                 one sensor (the host builds the job table, so a wave never straddles two sensors and frame, dmax and exclude mask are
//                 wave-uniform).  The wave stages its env's geom table in its own slice of LDS; the hull planes and the per-geom bound
//                 factors, which do not depend on the env, are staged once per workgroup by all four waves: one barrier per workgroup.
//                 Cull: the probes of a job share no origin, so the host stores with each job the bounding sphere (centre, radius rho) of
//                 its points in the sensor frame, and the wave keeps a geom that is not excluded and whose lower bound over that sphere,
//                 kap |c_geom - (o + R_s c_job)| - rb - rho, is <= dmax (planes always kept), with two ballots: the list is the two 64-bit
//                 masks, walked in geom order, wave-uniform, so it costs no LDS and no barrier.  Per lane and listed geom the lower bound
//                 kap |p - c_geom| - rb is tested against the lane's best so far before the exact formula; only lanes that pass walk a
//                 hull's planes.  The gradient is computed once, after the loop, for the winning geom only.
// The bound factor kap: a primitive lies inside the sphere (c_geom, rb), so its distance is at least |p - c_geom| - rb: kap = 1.  A hull's
// distance is by contract the PLANE BOUND max_i (n_i . q - c_i), which near an outside edge or vertex is smaller than the distance to the
// solid, so that bound does not hold for it.  What holds: every face plane touches the hull, which lies inside the sphere, so c_i <= rb and
// the plane bound is >= max_i n_i . q - rb >= kap |q| - rb with kap = min over unit u of max_i n_i . u (> 0 for a bounded hull; 1/sqrt(3)
// for a box-shaped one).  prb_hull_kappa evaluates that minimum on the host, on a grid of directions, minus the grid's covering radius.
// No atomics, no scratch: every output word is written once, by one lane, and an env's output depends on nothing but its record and the
// probe set.  The measurements: DESIGN.md 17.
#include "../../include/fsim_probes.h"

#define PRB_WAVES 4 // waves (units) per workgroup
#define PRB_JPW 4   // jobs per unit: up to 256 probes share one staging of the env's geom table
#define PRB_TINY 1e-12f // a vector shorter than this has no direction: the geom's local +x stands in (the header's degenerate points)
enum { PSW_DMAX = 0, PSW_EX = 1 /* three words */, PSW_WORDS = 4 }; // d_sens rows (masks as float bits)

struct ProbeArgs {
  int ncg, nprobes, nplanes, pstride, njobs;
  int upe /* units per env */, nunits /* n_envs * upe */;
};

DEV V3 prb_unit(V3 a) { // a / |a|, the local +x for a degenerate length
  const float l = norm(a);
  return l < PRB_TINY ? v3(1.0f, 0.0f, 0.0f) : a * (1.0f / l);
}

// the header's signed distance of the point q (geom frame) to the geom row G (k_cam_ray's staged layout); PL: the staged hull planes
DEV float prb_dist(int type, V3 q, const float *G, const float *PL) {
  const float s0 = G[CGW_SIZE], s1 = G[CGW_SIZE + 1], s2 = G[CGW_SIZE + 2];
  if (type == GT_PLANE) return q.z;
  if (type == GT_SPHERE) return norm(q) - s0;
  if (type == GT_CAPSULE) return norm(v3(q.x, q.y, q.z - fminf(fmaxf(q.z, -s1), s1))) - s0;
  if (type == GT_CYLINDER) {
    const float dr = sqrtf(q.x * q.x + q.y * q.y) - s0, dz = fabsf(q.z) - s1;
    if (dr <= 0.0f && dz <= 0.0f) return fmaxf(dr, dz);
    const float a = fmaxf(dr, 0.0f), b = fmaxf(dz, 0.0f);
    return sqrtf(a * a + b * b);
  }
  if (type == GT_BOX) {
    const float ax = fabsf(q.x) - s0, ay = fabsf(q.y) - s1, az = fabsf(q.z) - s2;
    if (ax <= 0.0f && ay <= 0.0f && az <= 0.0f) return fmaxf(ax, fmaxf(ay, az));
    return norm(v3(fmaxf(ax, 0.0f), fmaxf(ay, 0.0f), fmaxf(az, 0.0f)));
  }
  if (type == GT_MESH) { // the plane bound
    const int p0 = __float_as_int(G[CGW_PADR]), np = __float_as_int(G[CGW_PNUM]);
    float best = -CAM_INF;
    for (int k = 0; k < np; k++) {
      const float *pl = PL + 4 * (p0 + k);
      best = fmaxf(best, dot(ldv3(pl), q) - pl[3]);
    }
    return best;
  }
  return CAM_INF;
}

// the header's local unit gradient of that distance at q.  Ties as nrm_local settles them: the cylinder's side before its caps, the box's
// smallest axis, the hull's smallest plane index (strict > in the walks).
DEV V3 prb_grad(int type, V3 q, const float *G, const float *PL) {
  const float s0 = G[CGW_SIZE], s1 = G[CGW_SIZE + 1], s2 = G[CGW_SIZE + 2];
  if (type == GT_PLANE) return v3(0.0f, 0.0f, 1.0f);
  if (type == GT_SPHERE) return prb_unit(q);
  if (type == GT_CAPSULE) return prb_unit(v3(q.x, q.y, q.z - fminf(fmaxf(q.z, -s1), s1)));
  if (type == GT_CYLINDER) {
    const float dr = sqrtf(q.x * q.x + q.y * q.y) - s0, dz = fabsf(q.z) - s1, sz = q.z < 0.0f ? -1.0f : 1.0f;
    const V3 rad = prb_unit(v3(q.x, q.y, 0.0f));
    if (dr <= 0.0f && dz <= 0.0f) return dr >= dz ? rad : v3(0.0f, 0.0f, sz);
    const float a = fmaxf(dr, 0.0f), b = fmaxf(dz, 0.0f), il = 1.0f / sqrtf(a * a + b * b);
    return v3(rad.x * a * il, rad.y * a * il, sz * b * il);
  }
  if (type == GT_BOX) {
    const float ax = fabsf(q.x) - s0, ay = fabsf(q.y) - s1, az = fabsf(q.z) - s2;
    const float sx = q.x < 0.0f ? -1.0f : 1.0f, sy = q.y < 0.0f ? -1.0f : 1.0f, sz = q.z < 0.0f ? -1.0f : 1.0f;
    if (ax <= 0.0f && ay <= 0.0f && az <= 0.0f) { // strict >: the smallest axis wins a tie
      int k = 0;
      float best = ax;
      if (ay > best) { best = ay; k = 1; }
      if (az > best) k = 2;
      return v3(k == 0 ? sx : 0.0f, k == 1 ? sy : 0.0f, k == 2 ? sz : 0.0f);
    }
    const V3 m = v3(fmaxf(ax, 0.0f), fmaxf(ay, 0.0f), fmaxf(az, 0.0f));
    const float il = 1.0f / norm(m); // (outside: some component is > 0)
    return v3(sx * m.x * il, sy * m.y * il, sz * m.z * il);
  }
  if (type == GT_MESH) { // strict >: the smallest k wins a tie
    const int p0 = __float_as_int(G[CGW_PADR]), np = __float_as_int(G[CGW_PNUM]);
    V3 n = v3(0.0f, 0.0f, 0.0f);
    float best = -CAM_INF;
    for (int k = 0; k < np; k++) {
      const float *pl = PL + 4 * (p0 + k);
      const V3 nk = ldv3(pl);
      const float v = dot(nk, q) - pl[3];
      if (v > best) { best = v; n = nk; }
    }
    return n;
  }
  return v3(0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(64 * PRB_WAVES) void k_probe_dist(ProbeArgs a, const float *__restrict__ pose, const float *__restrict__ cgtab,
                                                               const float *__restrict__ planes_g, const float *__restrict__ kap_g,
                                                               const float *__restrict__ senstab,
                                                               const int *__restrict__ jobs /* [njobs][3]: sensor, first probe, probes */,
                                                               const float *__restrict__ jsph /* [njobs][4]: centre, rho (sensor frame) */,
                                                               const float *__restrict__ pts, float *__restrict__ dist, int *__restrict__ geom,
                                                               float *__restrict__ grad) {
  extern __shared__ __attribute__((aligned(16))) float prb_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nk = (a.ncg + 3) & ~3;
  float *PL = prb_lds;                                // [nplanes][4], shared by the workgroup
  float *KP = PL + 4 * a.nplanes;                     // [ncg] (padded to a multiple of 4), shared by the workgroup
  float *G = KP + nk + CAM_GW * a.ncg * w;            // [ncg][CAM_GW], this wave's
  const int u = blockIdx.x * PRB_WAVES + w;
  const bool live = u < a.nunits; // (the last workgroup may hold waves without a unit: they help with the shared tables and leave)
  const int e = live ? u / a.upe : 0, chunk = live ? u % a.upe : 0;
  const float *P = pose + (size_t)e * a.pstride;
  for (int i = tid; i < 4 * a.nplanes; i += 64 * PRB_WAVES) PL[i] = planes_g[i];
  for (int i = tid; i < a.ncg; i += 64 * PRB_WAVES) KP[i] = kap_g[i];
  if (live) {
    for (int i = lane; i < CAM_PW * a.ncg; i += 64) G[CAM_GW * (i / CAM_PW) + i % CAM_PW] = P[i];
    for (int i = lane; i < CAM_SW * a.ncg; i += 64) G[CAM_GW * (i / CAM_SW) + CAM_PW + i % CAM_SW] = cgtab[i];
  }
  __syncthreads();
  if (!live) return;
  const int j1 = min(a.njobs, (chunk + 1) * PRB_JPW);
  for (int j = chunk * PRB_JPW; j < j1; j++) {
    const int sn = jobs[3 * j], first = jobs[3 * j + 1], cnt = jobs[3 * j + 2];
    const float *S = senstab + PSW_WORDS * sn;
    const float dmax = S[PSW_DMAX];
    const V3 o = ldv3(P + CAM_PW * (a.ncg + sn));
    const M3 Rs = ldm3(P + CAM_PW * (a.ncg + sn) + 3);
    // cull, wave-uniform: not excluded, and the lower bound over the job's bounding sphere within dmax (planes always); ballot order is
    // geom order
    const V3 cj = o + mulv(Rs, ldv3(jsph + 4 * j));
    const float rho = jsph[4 * j + 3];
    unsigned long long keep[2];
    for (int h = 0; h < 2; h++) {
      const int g = 64 * h + lane;
      bool k = false;
      if (g < a.ncg && !((__float_as_uint(S[PSW_EX + (g >> 5)]) >> (g & 31)) & 1u)) {
        const float *Gg = G + CAM_GW * g;
        k = __float_as_int(Gg[CGW_TYPE]) == GT_PLANE || KP[g] * norm(ldv3(Gg + CGW_POS) - cj) - (Gg[CGW_RB] * 1.0001f + 1e-5f) - rho <= dmax;
      }
      keep[h] = __ballot(k);
    }
    const int r = first + min(lane, cnt - 1); // (lanes past the job's end repeat its last probe and write nothing)
    const V3 p = o + mulv(Rs, ldv3(pts + 3 * r));
    float best = CAM_INF;
    int bi = -1;
    for (int h = 0; h < 2; h++) {
      for (unsigned long long m = keep[h]; m; m &= m - 1) {
        const int g = 64 * h + __ffsll(m) - 1;
        const float *Gg = G + CAM_GW * g;
        const int type = __float_as_int(Gg[CGW_TYPE]);
        const V3 c = p - ldv3(Gg + CGW_POS);
        // Per-lane prune.  lb is below the geom's distance d (the file comment; the camera's slack only lowers it further, by more than
        // the rounding of the two norms), so a skipped geom has d >= lb > min(best, dmax): it would lose the strict < below, or win only
        // to be refused by dmax, which gives the same outputs as no winner.  Ties are unaffected: a geom with d == best has lb <= best, is
        // not skipped, and loses the strict < exactly as it would without the prune.
        if (type != GT_PLANE && KP[g] * norm(c) - (Gg[CGW_RB] * 1.0001f + 1e-5f) > fminf(best, dmax)) continue;
        const float d = prb_dist(type, multv(ldm3(Gg + CGW_MAT), c), Gg, PL);
        if (d < best) { best = d; bi = g; }
      }
    }
    if (lane < cnt) {
      const size_t out = (size_t)e * a.nprobes + r;
      const bool hit = bi >= 0 && best <= dmax;
      if (dist) dist[out] = hit ? best : dmax;
      if (geom) geom[out] = hit ? __float_as_int(G[CAM_GW * bi + CGW_ID]) : -1;
      if (grad) {
        V3 n = v3(0.0f, 0.0f, 0.0f);
        if (hit) {
          const float *Gb = G + CAM_GW * bi;
          const M3 Rg = ldm3(Gb + CGW_MAT);
          n = mulv(Rg, prb_grad(__float_as_int(Gb[CGW_TYPE]), multv(Rg, p - ldv3(Gb + CGW_POS)), Gb, PL));
        }
        stv3(grad + 3 * out, n);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ host
struct ProbeState {
  int nsens = 0, nprobes = 0, nplanes = 0, pstride = 0, njobs = 0;
  float *d_mounts = nullptr, *d_cg = nullptr, *d_planes = nullptr, *d_kap = nullptr, *d_pose = nullptr, *d_sens = nullptr, *d_pts = nullptr, *d_jsph = nullptr;
  int *d_jobs = nullptr;
  DevTables tabs; // owns them
};

// The bound factor of a hull (file comment): min over unit u of max_i n_i . u over the planes that touch the sphere's inside (c_i <= rb),
// evaluated on a latitude / longitude grid of step D and lowered by the grid's covering radius (any u is within D / 2 in each angle of a
// grid direction, a chord of at most D / sqrt(2), and n . u changes by at most that chord), never below 0.  A table the derivation does
// not cover gives a factor that switches cull and prune off for the geom.
static float prb_hull_kappa(const float *planes, int num, float rb) {
  const int NT = 90;
  const double D = M_PI / NT, slack = D * 0.7072;
  std::vector<double> n;
  for (int i = 0; i < num; i++) {
    const float *pl = planes + 4 * i;
    const double l = sqrt((double)pl[0] * pl[0] + (double)pl[1] * pl[1] + (double)pl[2] * pl[2]);
    if (!(l > 0.999 && l < 1.001) || pl[3] > rb * 1.0001f + 1e-5f) return -1e30f; // (not a unit normal, or no face of a solid inside the sphere: no bound, nothing culled or pruned)
    n.push_back(pl[0] / l); n.push_back(pl[1] / l); n.push_back(pl[2] / l);
  }
  double kap = 1.0;
  for (int it = 0; it <= NT; it++) {
    const double st = sin(it * D), ct = cos(it * D);
    for (int ip = 0; ip < 2 * NT; ip++) {
      const double ux = st * cos(ip * D), uy = st * sin(ip * D);
      double mx = -1.0;
      for (size_t i = 0; i < n.size(); i += 3) mx = std::max(mx, n[i] * ux + n[i + 1] * uy + n[i + 2] * ct);
      kap = std::min(kap, mx);
    }
  }
  return (float)std::max(0.0, kap - slack);
}

extern "C" int fsim_set_probes(fsim_t *s, int n_sensors, const fsim_probe_sensor_t *sensors, int n_probes, const float *pts, int n_planes,
                               const float *hull_planes, const int32_t *hull_adr, const int32_t *hull_num) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_probes: null handle");
  if (n_sensors == 0) return sensor_clear(s, s->probe);
  if (!sensors || !pts) FAIL(FSIM_EINVAL, "fsim_set_probes: null argument");
  if (n_sensors < 1 || n_sensors > FSIM_PROBE_MAX_SENSORS) FAIL(FSIM_EINVAL, "fsim_set_probes: %d sensors (1 .. %d)", n_sensors, FSIM_PROBE_MAX_SENSORS);
  if (n_probes < 1 || n_probes > FSIM_PROBE_MAX_PROBES) FAIL(FSIM_EINVAL, "fsim_set_probes: %d probes (1 .. %d over all sensors)", n_probes, FSIM_PROBE_MAX_PROBES);
  const DModel &m = s->m;
  if (m.ncg > FSIM_CAM_MAX_GEOMS) FAIL(FSIM_EINVAL, "fsim_set_probes: %d colliding geoms (the distance pass stages at most %d)", m.ncg, FSIM_CAM_MAX_GEOMS);
  if (n_planes < 0 || n_planes > FSIM_CAM_MAX_PLANES) FAIL(FSIM_EINVAL, "fsim_set_probes: %d hull planes (at most %d)", n_planes, FSIM_CAM_MAX_PLANES);
  for (int i = 0; i < 3 * n_probes; i++)
    if (!std::isfinite(pts[i])) FAIL(FSIM_EINVAL, "fsim_set_probes: point %d is not finite (%g, %g, %g)", i / 3, pts[i / 3 * 3], pts[i / 3 * 3 + 1], pts[i / 3 * 3 + 2]);
  CamMountTables mt;
  { int rc_ = cam_mount_tables(s, mt); if (rc_) return rc_; }
  ProbeState c;
  c.nsens = n_sensors; c.nprobes = n_probes; c.nplanes = n_planes;
  std::vector<float> mrow((size_t)CCW_WORDS * n_sensors, 0.0f), srow((size_t)PSW_WORDS * n_sensors, 0.0f), jsph;
  std::vector<int> jobs;
  int next = 0;
  for (int i = 0; i < n_sensors; i++) {
    const fsim_probe_sensor_t &k = sensors[i];
    if (k.body < -1 || k.body >= m.nbody) FAIL(FSIM_EINVAL, "probe sensor %d: unknown body %d (the model has %d bodies)", i, k.body, m.nbody);
    if (!(k.dmax > 0.0f) || !std::isfinite(k.dmax)) FAIL(FSIM_EINVAL, "probe sensor %d: needs 0 < dmax < inf (got %g)", i, k.dmax);
    if (k.n_probes < 1) FAIL(FSIM_EINVAL, "probe sensor %d: %d probes (at least 1)", i, k.n_probes);
    if (k.first_probe != next || k.n_probes > n_probes - next)
      FAIL(FSIM_EINVAL, "probe sensor %d: slice %d + %d is not contiguous with the slices before it (next probe %d of %d)", i, k.first_probe, k.n_probes, next, n_probes);
    for (int g = m.ncg; g < 96; g++)
      if ((k.exclude[g >> 5] >> (g & 31)) & 1u) FAIL(FSIM_EINVAL, "probe sensor %d: exclude bit %d set (the model has %d colliding geoms)", i, g, m.ncg);
    if (cam_mount_row(mt, k.body, k.pos, k.quat, mrow.data() + CCW_WORDS * i)) FAIL(FSIM_EINVAL, "probe sensor %d: bad pose", i);
    float *r = srow.data() + PSW_WORDS * i;
    r[PSW_DMAX] = k.dmax;
    for (int j = 0; j < 3; j++) memcpy(r + PSW_EX + j, &k.exclude[j], 4);
    for (int f = 0; f < k.n_probes; f += 64) { // a job and the bounding sphere of its points: the box's centre, the largest distance from it
      const int cnt = std::min(64, k.n_probes - f);
      const float *q = pts + 3 * (size_t)(next + f);
      double lo[3] = {q[0], q[1], q[2]}, hi[3] = {q[0], q[1], q[2]}, r2 = 0.0;
      for (int t = 0; t < cnt; t++)
        for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], (double)q[3 * t + a]); hi[a] = std::max(hi[a], (double)q[3 * t + a]); }
      const float cx = (float)(0.5 * (lo[0] + hi[0])), cy = (float)(0.5 * (lo[1] + hi[1])), cz = (float)(0.5 * (lo[2] + hi[2]));
      for (int t = 0; t < cnt; t++) {
        const double dx = q[3 * t] - (double)cx, dy = q[3 * t + 1] - (double)cy, dz = q[3 * t + 2] - (double)cz;
        r2 = std::max(r2, dx * dx + dy * dy + dz * dz);
      }
      jobs.push_back(i); jobs.push_back(next + f); jobs.push_back(cnt);
      jsph.push_back(cx); jsph.push_back(cy); jsph.push_back(cz); jsph.push_back((float)(sqrt(r2) * 1.0001 + 1e-6)); // (rounded up: the cull only keeps more)
    }
    next += k.n_probes;
  }
  if (next != n_probes) FAIL(FSIM_EINVAL, "fsim_set_probes: the sensors' slices cover %d of the %d probes", next, n_probes);
  std::vector<float> cg;
  { int rc_ = cam_geom_rows(m, mt, "fsim_set_probes", n_planes, hull_planes, hull_adr, hull_num, cg); if (rc_) return rc_; }
  std::vector<float> kap((size_t)std::max(m.ncg, 1), 1.0f);
  for (int g = 0; g < m.ncg; g++)
    if (mt.cg_type[g] == GT_MESH) kap[g] = prb_hull_kappa(hull_planes + 4 * (size_t)hull_adr[g], hull_num[g], mt.cg_rbound[g]);
  c.njobs = (int)jobs.size() / 3;
  c.pstride = (CAM_PW * (m.ncg + n_sensors) + 3) / 4 * 4;
  return sensor_install(s, "fsim_set_probes", s->probe, c, [&](DevTables &t) {
    t.put(&c.d_mounts, mrow.data(), mrow.size());
    t.put(&c.d_sens, srow.data(), srow.size());
    t.put(&c.d_pts, pts, (size_t)3 * n_probes);
    t.put(&c.d_jobs, jobs.data(), jobs.size());
    t.put(&c.d_jsph, jsph.data(), jsph.size());
    t.put(&c.d_cg, cg.data(), cg.size());
    t.put(&c.d_kap, kap.data(), kap.size());
    t.put(&c.d_planes, hull_planes, (size_t)4 * n_planes);
    t.put(&c.d_pose, nullptr, (size_t)s->n_envs * c.pstride);
  });
}

extern "C" int fsim_probe_distance(fsim_t *s, float *dist_dev, int32_t *geom_dev, float *grad_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_probe_distance: null handle");
  if (!s->probe) FAIL(FSIM_EINVAL, "fsim_probe_distance: no probes set (fsim_set_probes)");
  if (!dist_dev && !geom_dev && !grad_dev) FAIL(FSIM_EINVAL, "fsim_probe_distance: no output (distance, geom and gradient all NULL)");
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const ProbeState &k = *s->probe;
  const DModel &m = s->m;
  hipLaunchKernelGGL(k_cam_pose, dim3(s->n_envs), dim3(64), 0, s->stream, cam_pose_args(s, k.nsens, k.pstride), s->d_state, k.d_mounts, k.d_pose);
  HIPCHK(hipGetLastError());
  ProbeArgs ra{};
  ra.ncg = m.ncg; ra.nprobes = k.nprobes; ra.nplanes = k.nplanes; ra.pstride = k.pstride; ra.njobs = k.njobs;
  ra.upe = (k.njobs + PRB_JPW - 1) / PRB_JPW;
  const size_t nunits = (size_t)s->n_envs * ra.upe, nblk = (nunits + PRB_WAVES - 1) / PRB_WAVES;
  if (nunits > 0x7fffffff) FAIL(FSIM_EINVAL, "fsim_probe_distance: %zu units", nunits);
  ra.nunits = (int)nunits;
  const size_t lds = 4 * ((size_t)4 * k.nplanes + (size_t)((m.ncg + 3) & ~3) + (size_t)PRB_WAVES * CAM_GW * m.ncg); // at most 47 KB (1024 planes, 96 geoms)
  hipLaunchKernelGGL(k_probe_dist, dim3((unsigned)nblk), dim3(64 * PRB_WAVES), lds, s->stream, ra, k.d_pose, k.d_cg, k.d_planes, k.d_kap, k.d_sens, k.d_jobs,
                     k.d_jsph, k.d_pts, dist_dev, geom_dev, grad_dev);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
