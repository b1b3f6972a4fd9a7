// fsim_rays.hpp -- ray-cast range sensors and lidar (include/fsim_rays.h).  Included at the end of fsim.hip, after fsim_flow.hpp: the host
// part launches k_cam_pose as it is, with the sensors' own mount table (rows of the CCW_* layout) and a pose scratch the ray set owns;
// the cast kernel stages an env's geom table and the hull planes in k_cam_ray's staged layout and calls cam_interval and nrm_local as
// they are.
//
// Two launches per fsim_cast_rays, both on the handle's stream:
//   k_cam_pose  (fsim_camera.hpp) one wave per env: world pose of every colliding geom and of every sensor frame;
//   k_ray_cast  256-thread workgroups of four INDEPENDENT waves.  A wave takes one unit: up to RAY_JPW consecutive jobs of one env, a job
//               being up to 64 consecutive rays of one sensor (the host builds the job table, so a wave never straddles two sensors and
//               origin, range and exclude mask are wave-uniform).  The wave stages its env's geom table in its own slice of LDS; the hull
//               planes, which do not depend on the env, are staged once per workgroup by all four waves: one barrier per workgroup.
//               Per job the wave culls the geom table to the geoms that are not excluded and whose bounding sphere comes within tmax of
//               the origin (planes always kept) with two ballots: the list is the two 64-bit masks, walked in geom order, wave-uniform,
//               so it costs no LDS and no barrier.  Per lane and listed geom the closest approach of the ray to the bounding sphere is
//               tested before the exact interval (the camera's slack, 1.0001 r + 1e-5): that keeps a 459-plane hull affordable.  The
//               normal is computed once, after the loop, for the winning geom only.
// No atomics, no scratch: every output word is written once, by one lane, and an env's output depends on nothing but its record and the
// ray set.  The workgroup shape and the measurements: DESIGN.md 16.
#include "../../include/fsim_rays.h"

#define RAY_WAVES 4 // waves (units) per workgroup
#define RAY_JPW 4   // jobs per unit: up to 256 rays share one staging of the env's geom table
enum { RSW_TMIN = 0, RSW_TMAX = 1, RSW_EX = 2 /* three words */, RSW_WORDS = 8 }; // d_sens rows (masks as float bits)

struct RayArgs {
  int ncg, nrays, nplanes, pstride, njobs;
  int upe /* units per env */, nunits /* n_envs * upe */;
};

__global__ __launch_bounds__(64 * RAY_WAVES) void k_ray_cast(RayArgs a, const float *__restrict__ pose, const float *__restrict__ cgtab,
                                                             const float *__restrict__ planes_g, const float *__restrict__ senstab,
                                                             const int *__restrict__ jobs /* [njobs][3]: sensor, first ray, rays */,
                                                             const float *__restrict__ dirs, float *__restrict__ dist, int *__restrict__ geom,
                                                             float *__restrict__ normal) {
  extern __shared__ float ray_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  float *PL = ray_lds;                                          // [nplanes][4], shared by the workgroup
  float *G = PL + 4 * a.nplanes + CAM_GW * a.ncg * w;           // [ncg][CAM_GW], this wave's
  const int u = blockIdx.x * RAY_WAVES + w;
  const bool live = u < a.nunits; // (the last workgroup may hold waves without a unit: they help with the planes and leave)
  const int e = live ? u / a.upe : 0, chunk = live ? u % a.upe : 0;
  const float *P = pose + (size_t)e * a.pstride;
  for (int i = tid; i < 4 * a.nplanes; i += 64 * RAY_WAVES) PL[i] = planes_g[i];
  if (live) {
    for (int i = lane; i < CAM_PW * a.ncg; i += 64) G[CAM_GW * (i / CAM_PW) + i % CAM_PW] = P[i];
    for (int i = lane; i < CAM_SW * a.ncg; i += 64) G[CAM_GW * (i / CAM_SW) + CAM_PW + i % CAM_SW] = cgtab[i];
  }
  __syncthreads();
  if (!live) return;
  const int j1 = min(a.njobs, (chunk + 1) * RAY_JPW);
  for (int j = chunk * RAY_JPW; j < j1; j++) {
    const int sn = jobs[3 * j], first = jobs[3 * j + 1], cnt = jobs[3 * j + 2];
    const float *S = senstab + RSW_WORDS * sn;
    const float tmin = S[RSW_TMIN], tmax = S[RSW_TMAX];
    const V3 o = ldv3(P + CAM_PW * (a.ncg + sn));
    const M3 Rs = ldm3(P + CAM_PW * (a.ncg + sn) + 3);
    // cull, wave-uniform: not excluded, and the bounding sphere within tmax of the origin (planes always); ballot order is geom order
    unsigned long long keep[2];
    for (int h = 0; h < 2; h++) {
      const int g = 64 * h + lane;
      bool k = false;
      if (g < a.ncg && !((__float_as_uint(S[RSW_EX + (g >> 5)]) >> (g & 31)) & 1u)) {
        const float *Gg = G + CAM_GW * g;
        k = __float_as_int(Gg[CGW_TYPE]) == GT_PLANE || norm(ldv3(Gg + CGW_POS) - o) - (Gg[CGW_RB] * 1.0001f + 1e-5f) <= tmax;
      }
      keep[h] = __ballot(k);
    }
    const int r = first + min(lane, cnt - 1); // (lanes past the job's end cast its last ray again and write nothing)
    const V3 d = mulv(Rs, ldv3(dirs + 3 * r));
    float best = CAM_INF;
    int bi = -1;
    for (int h = 0; h < 2; h++) {
      for (unsigned long long m = keep[h]; m; m &= m - 1) {
        const int g = 64 * h + __ffsll(m) - 1;
        const float *Gg = G + CAM_GW * g;
        const int type = __float_as_int(Gg[CGW_TYPE]);
        const V3 gp = ldv3(Gg + CGW_POS);
        if (type != GT_PLANE) { // closest approach of the ray to the bounding sphere; every point of the solid has |t - tca| <= rb
          const V3 c = gp - o;
          const float tca = dot(c, d), rb = Gg[CGW_RB] * 1.0001f + 1e-5f;
          const V3 p = c - d * tca;
          if (dot(p, p) > rb * rb || tca + rb < tmin || tca - rb > tmax) continue;
        }
        const M3 Rg = ldm3(Gg + CGW_MAT);
        float t0, t1;
        if (!cam_interval(type, multv(Rg, o - gp), multv(Rg, d), Gg, PL, t0, t1)) continue;
        const float t = t0 >= tmin ? t0 : t1; // the nearest surface point at or beyond tmin
        if (t >= tmin && t <= tmax && t < best) { best = t; bi = g; }
      }
    }
    if (lane < cnt) {
      const size_t out = (size_t)e * a.nrays + r;
      if (dist) dist[out] = bi >= 0 ? best : -1.0f;
      if (geom) geom[out] = bi >= 0 ? __float_as_int(G[CAM_GW * bi + CGW_ID]) : -1;
      if (normal) {
        V3 n = v3(0.0f, 0.0f, 0.0f);
        if (bi >= 0) {
          const float *Gb = G + CAM_GW * bi;
          const M3 Rg = ldm3(Gb + CGW_MAT);
          n = mulv(Rg, nrm_local(Gb, PL, multv(Rg, o + d * best - ldv3(Gb + CGW_POS))));
        }
        stv3(normal + 3 * out, n);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ host
struct RayState {
  int nsens = 0, nrays = 0, nplanes = 0, pstride = 0, njobs = 0;
  float *d_mounts = nullptr, *d_cg = nullptr, *d_planes = nullptr, *d_pose = nullptr, *d_sens = nullptr, *d_dirs = nullptr;
  int *d_jobs = nullptr;
  DevTables tabs; // owns them
};

extern "C" int fsim_set_rays(fsim_t *s, int n_sensors, const fsim_ray_sensor_t *sensors, int n_rays, const float *dirs, int n_planes,
                             const float *hull_planes, const int32_t *hull_adr, const int32_t *hull_num) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_rays: null handle");
  if (n_sensors == 0) return sensor_clear(s, s->ray);
  if (!sensors || !dirs) FAIL(FSIM_EINVAL, "fsim_set_rays: null argument");
  if (n_sensors < 1 || n_sensors > FSIM_RAY_MAX_SENSORS) FAIL(FSIM_EINVAL, "fsim_set_rays: %d sensors (1 .. %d)", n_sensors, FSIM_RAY_MAX_SENSORS);
  if (n_rays < 1 || n_rays > FSIM_RAY_MAX_RAYS) FAIL(FSIM_EINVAL, "fsim_set_rays: %d rays (1 .. %d over all sensors)", n_rays, FSIM_RAY_MAX_RAYS);
  const DModel &m = s->m;
  if (m.ncg > FSIM_CAM_MAX_GEOMS) FAIL(FSIM_EINVAL, "fsim_set_rays: %d colliding geoms (the cast pass stages at most %d)", m.ncg, FSIM_CAM_MAX_GEOMS);
  if (n_planes < 0 || n_planes > FSIM_CAM_MAX_PLANES) FAIL(FSIM_EINVAL, "fsim_set_rays: %d hull planes (at most %d)", n_planes, FSIM_CAM_MAX_PLANES);
  CamMountTables mt;
  { int rc_ = cam_mount_tables(s, mt); if (rc_) return rc_; }
  RayState c;
  c.nsens = n_sensors; c.nrays = n_rays; c.nplanes = n_planes;
  std::vector<float> mrow((size_t)CCW_WORDS * n_sensors, 0.0f), srow((size_t)RSW_WORDS * n_sensors, 0.0f), udir((size_t)3 * n_rays);
  std::vector<int> jobs;
  int next = 0;
  for (int i = 0; i < n_sensors; i++) {
    const fsim_ray_sensor_t &k = sensors[i];
    if (k.body < -1 || k.body >= m.nbody) FAIL(FSIM_EINVAL, "ray sensor %d: unknown body %d (the model has %d bodies)", i, k.body, m.nbody);
    if (!(k.tmin >= 0.0f) || !(k.tmax > k.tmin) || !std::isfinite(k.tmax)) FAIL(FSIM_EINVAL, "ray sensor %d: needs 0 <= tmin < tmax < inf (got %g, %g)", i, k.tmin, k.tmax);
    if (k.n_rays < 1) FAIL(FSIM_EINVAL, "ray sensor %d: %d rays (at least 1)", i, k.n_rays);
    if (k.first_ray != next || k.n_rays > n_rays - next)
      FAIL(FSIM_EINVAL, "ray sensor %d: slice %d + %d is not contiguous with the slices before it (next ray %d of %d)", i, k.first_ray, k.n_rays, next, n_rays);
    for (int g = m.ncg; g < 96; g++)
      if ((k.exclude[g >> 5] >> (g & 31)) & 1u) FAIL(FSIM_EINVAL, "ray sensor %d: exclude bit %d set (the model has %d colliding geoms)", i, g, m.ncg);
    if (cam_mount_row(mt, k.body, k.pos, k.quat, mrow.data() + CCW_WORDS * i)) FAIL(FSIM_EINVAL, "ray sensor %d: bad pose", i);
    float *r = srow.data() + RSW_WORDS * i;
    r[RSW_TMIN] = k.tmin; r[RSW_TMAX] = k.tmax;
    for (int j = 0; j < 3; j++) memcpy(r + RSW_EX + j, &k.exclude[j], 4);
    for (int f = 0; f < k.n_rays; f += 64) { jobs.push_back(i); jobs.push_back(next + f); jobs.push_back(std::min(64, k.n_rays - f)); }
    next += k.n_rays;
  }
  if (next != n_rays) FAIL(FSIM_EINVAL, "fsim_set_rays: the sensors' slices cover %d of the %d rays", next, n_rays);
  for (int i = 0; i < n_rays; i++) { // unit directions, normalised in double
    const double x = dirs[3 * i], y = dirs[3 * i + 1], z = dirs[3 * i + 2], l = sqrt(x * x + y * y + z * z);
    if (!std::isfinite(l) || !(l > 0.0)) FAIL(FSIM_EINVAL, "fsim_set_rays: direction %d is zero or not finite (%g, %g, %g)", i, x, y, z);
    udir[3 * i] = (float)(x / l); udir[3 * i + 1] = (float)(y / l); udir[3 * i + 2] = (float)(z / l);
  }
  std::vector<float> cg;
  { int rc_ = cam_geom_rows(m, mt, "fsim_set_rays", n_planes, hull_planes, hull_adr, hull_num, cg); if (rc_) return rc_; }
  c.njobs = (int)jobs.size() / 3;
  c.pstride = (CAM_PW * (m.ncg + n_sensors) + 3) / 4 * 4;
  return sensor_install(s, "fsim_set_rays", s->ray, c, [&](DevTables &t) {
    t.put(&c.d_mounts, mrow.data(), mrow.size());
    t.put(&c.d_sens, srow.data(), srow.size());
    t.put(&c.d_dirs, udir.data(), udir.size());
    t.put(&c.d_jobs, jobs.data(), jobs.size());
    t.put(&c.d_cg, cg.data(), cg.size());
    t.put(&c.d_planes, hull_planes, (size_t)4 * n_planes);
    t.put(&c.d_pose, nullptr, (size_t)s->n_envs * c.pstride);
  });
}

extern "C" int fsim_cast_rays(fsim_t *s, float *dist_dev, int32_t *geom_dev, float *normal_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_cast_rays: null handle");
  if (!s->ray) FAIL(FSIM_EINVAL, "fsim_cast_rays: no rays set (fsim_set_rays)");
  if (!dist_dev && !geom_dev && !normal_dev) FAIL(FSIM_EINVAL, "fsim_cast_rays: no output (distance, geom and normal all NULL)");
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const RayState &k = *s->ray;
  const DModel &m = s->m;
  hipLaunchKernelGGL(k_cam_pose, dim3(s->n_envs), dim3(64), 0, s->stream, cam_pose_args(s, k.nsens, k.pstride), s->d_state, k.d_mounts, k.d_pose);
  HIPCHK(hipGetLastError());
  RayArgs ra{};
  ra.ncg = m.ncg; ra.nrays = k.nrays; ra.nplanes = k.nplanes; ra.pstride = k.pstride; ra.njobs = k.njobs;
  ra.upe = (k.njobs + RAY_JPW - 1) / RAY_JPW;
  const size_t nunits = (size_t)s->n_envs * ra.upe, nblk = (nunits + RAY_WAVES - 1) / RAY_WAVES;
  if (nunits > 0x7fffffff) FAIL(FSIM_EINVAL, "fsim_cast_rays: %zu units", nunits);
  ra.nunits = (int)nunits;
  const size_t lds = 4 * ((size_t)4 * k.nplanes + (size_t)RAY_WAVES * CAM_GW * m.ncg); // at most 47 KB (1024 planes, 96 geoms)
  hipLaunchKernelGGL(k_ray_cast, dim3((unsigned)nblk), dim3(64 * RAY_WAVES), lds, s->stream, ra, k.d_pose, k.d_cg, k.d_planes, k.d_sens, k.d_jobs, k.d_dirs,
                     dist_dev, geom_dev, normal_dev);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
