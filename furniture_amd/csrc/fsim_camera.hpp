// fsim_camera.hpp -- batched depth / segmentation cameras (include/fsim_camera.h).  Included at the end of fsim.hip: the host part
// uses the handle (struct fsim), settle() and the blob readers.
//
// Two launches per fsim_render, both on the handle's stream:
//   k_cam_pose  one wave per env: qpos of the env record (read only) -> world pose of every colliding geom and of every camera, with
//               the arithmetic of fs_kinematics + fs_collide (pointer doubling up the reduced tree, qnormalized on free joints and on
//               every composition, geom pose = body pose (x) geom offset), into the handle's scratch buffer.  Its body-pose stages (A)
//               and (B) are the functions of fsim_kin.hpp, which k_cam_twist, k_frame_state, k_dynamics and k_momenta call too;
//   k_cam_ray   one 256-thread workgroup per (env, camera, 32 x 32 pixel tile): the env's geom table is staged in LDS, each wave culls
//               it against the frustum of its 16 x 16 quarter into a wave-uniform list (bounding spheres; planes always kept) and each
//               lane casts the rays of four pixels of one column against that list in closed form, in the geom's frame.
// No atomics: every pixel is written once, by one lane, and an env's image depends on nothing but its record and the camera set.
// What fsim_points.hpp, fsim_voxels.hpp and fsim_normals.hpp share is here too, as plain functions: CamView and cam_stage_views for
// their kernels, cam_view and cam_render_images (with the handle's one image scratch) for their host parts.
#include "../../include/fsim_camera.h"

#define CAM_PW 12 // scratch words per pose: position 3, rotation 9 (row-major, local -> world)
#define CAM_SW 8  // static words per colliding geom (d_cg): size 3, rbound, type, first hull plane, hull planes, model geom id
#define CAM_GW 20 // LDS words per staged geom: the pose, then the static words
#define CAM_TILE 32
enum { CGW_POS = 0, CGW_MAT = 3, CGW_SIZE = 12, CGW_RB = 15, CGW_TYPE = 16, CGW_PADR = 17, CGW_PNUM = 18, CGW_ID = 19 };
enum { CCW_RBODY = 0, CCW_CURSOR = 1, CCW_POS = 2, CCW_QUAT = 5, CCW_WORDS = 12 }; // d_cams rows (ints as float bits)

struct CamPoseArgs {
  KinArgs kin;
  const int *cg_body, *cg_cursor;
  const float *cg_pos, *cg_mat, *cursor_pos0;
  int ncg, ncam, ecpos /* Cursor agent: EC_POS of the record, else -1 */, pstride;
};

__global__ __launch_bounds__(64) void k_cam_pose(CamPoseArgs a, const float *__restrict__ state, const float *__restrict__ cams,
                                                 float *__restrict__ pose) {
  __shared__ float sp[3 * 32], sq[4 * 32];
  __shared__ int sanc[32];
  const int e = blockIdx.x, b = threadIdx.x;
  const float *rec = state + (size_t)e * a.kin.stride;
  float *out = pose + (size_t)e * a.pstride;
  // (A) joint transform relative to the parent, (B) world poses by pointer doubling up the tree: fsim_kin.hpp
  V3 P;
  Q4 Q;
  const KinLane l = kin_joint_pose(a.kin, rec, b, &P, &Q);
  kin_world_poses(a.kin, l, b, sp, sq, sanc, &P, &Q);
  if (b < a.kin.nr) { stv3(sp + 3 * b, P); stq(sq + 4 * b, Q); }
  __syncthreads();
  // (C) colliding geoms (fs_collide): body pose (x) geom offset; cursor boxes follow the env's cursor position
  for (int g = b; g < a.ncg; g += 64) {
    const int gb = a.cg_body[g];
    const M3 Rb = q2m(ldq(sq + 4 * gb));
    V3 gp = ldv3(sp + 3 * gb) + mulv(Rb, ldv3(a.cg_pos + 3 * g));
    if (a.ecpos >= 0) {
      const int cm = a.cg_cursor[g];
      if (cm) { const int k = (cm & 1) ? 0 : 1; gp = gp + ldv3(rec + a.ecpos + 3 * k) - ldv3(a.cursor_pos0 + 3 * k); }
    }
    stv3(out + CAM_PW * g, gp);
    stm3(out + CAM_PW * g + 3, mulm(Rb, ldm3(a.cg_mat + 9 * g)));
  }
  // cameras: reduced body pose (x) the host-composed (body_relpos, body_relquat) (x) camera pose
  if (b < a.ncam) {
    const float *cw = cams + CCW_WORDS * b;
    const int rb = __float_as_int(cw[CCW_RBODY]), cur = __float_as_int(cw[CCW_CURSOR]);
    const Q4 qb = ldq(sq + 4 * rb);
    V3 cp = ldv3(sp + 3 * rb) + qrot(qb, ldv3(cw + CCW_POS));
    if (cur >= 0 && a.ecpos >= 0) cp = cp + ldv3(rec + a.ecpos + 3 * cur) - ldv3(a.cursor_pos0 + 3 * cur);
    stv3(out + CAM_PW * (a.ncg + b), cp);
    stm3(out + CAM_PW * (a.ncg + b) + 3, q2m(qnormalized(qmul(qb, ldq(cw + CCW_QUAT)))));
  }
}

struct CamRayArgs {
  int ncg, ncam, W, H, ntx, nty, nplanes, pstride;
  float slope[FSIM_CAM_MAX]; // tan(fovy / 2) / (H / 2): camera-frame x / y per pixel at unit depth
  float znear[FSIM_CAM_MAX], zfar[FSIM_CAM_MAX];
};

// What a kernel that reads the rendered images needs of the camera set (cam_view fills it): k_pts_gather, k_vox_bin, k_cam_normal
struct CamView {
  int ncam, W, H, npix /* ncam * W * H */, ncg, pstride;
  float slope[FSIM_CAM_MAX];
};

// Stage what pts_point reads in LDS: the camera rows of the env's pose scratch (P: already at them, pose + e * pstride + CAM_PW * ncg)
// as cpose [FSIM_CAM_MAX][CAM_PW] and the slopes as cslope [FSIM_CAM_MAX].  The caller's barrier follows.
DEV void cam_stage_views(float *cpose, float *cslope, const float *P, const CamView &v, int tid, int nt) {
  for (int i = tid; i < CAM_PW * v.ncam; i += nt) cpose[i] = P[i];
  if (tid < FSIM_CAM_MAX) cslope[tid] = v.slope[tid];
}

#define CAM_INF 3.0e38f
// [t0, t1]: the ray o + t d (geom frame) inside the solid; false: it misses.  Planes are infinite half-spaces (as they collide) whose
// only surface point on the ray is z = 0.
DEV bool cam_interval_z(float oz, float dz, float h, float &t0, float &t1) { // slab |z| <= h
  if (fabsf(dz) < 1e-30f) { t0 = -CAM_INF; t1 = CAM_INF; return fabsf(oz) <= h; }
  const float inv = 1.0f / dz, ta = (-h - oz) * inv, tb = (h - oz) * inv;
  t0 = fminf(ta, tb); t1 = fmaxf(ta, tb);
  return true;
}
DEV bool cam_interval_sphere(V3 o, V3 d, float r, float &t0, float &t1) { // closest approach first: no cancellation in b^2 - ac
  const float dd = dot(d, d), tc = -dot(o, d) / dd;
  const V3 p = o + d * tc;
  const float h2 = r * r - dot(p, p);
  if (h2 < 0.0f) return false;
  const float dt = sqrtf(h2 / dd);
  t0 = tc - dt; t1 = tc + dt;
  return true;
}
DEV bool cam_interval_tube(V3 o, V3 d, float r, float &t0, float &t1) { // infinite cylinder x^2 + y^2 <= r^2
  const float a = d.x * d.x + d.y * d.y;
  if (a < 1e-30f) { t0 = -CAM_INF; t1 = CAM_INF; return o.x * o.x + o.y * o.y <= r * r; }
  const float tc = -(o.x * d.x + o.y * d.y) / a, px = o.x + tc * d.x, py = o.y + tc * d.y, h2 = r * r - (px * px + py * py);
  if (h2 < 0.0f) return false;
  const float dt = sqrtf(h2 / a);
  t0 = tc - dt; t1 = tc + dt;
  return true;
}
DEV bool cam_interval(int type, V3 o, V3 d, const float *G, const float *planes, float &t0, float &t1) {
  const float s0 = G[CGW_SIZE], s1 = G[CGW_SIZE + 1], s2 = G[CGW_SIZE + 2];
  if (type == GT_PLANE) {
    if (fabsf(d.z) < 1e-30f) return false;
    t0 = t1 = -o.z / d.z;
    return true;
  }
  if (type == GT_SPHERE) return cam_interval_sphere(o, d, s0, t0, t1);
  if (type == GT_CYLINDER) {
    float a0, a1, b0, b1;
    if (!cam_interval_tube(o, d, s0, a0, a1) || !cam_interval_z(o.z, d.z, s1, b0, b1)) return false;
    t0 = fmaxf(a0, b0); t1 = fminf(a1, b1);
    return t0 <= t1;
  }
  if (type == GT_CAPSULE) { // convex union of the tube segment and the two end spheres: one interval, [min entry, max exit]
    bool hit = false;
    float a0, a1, b0, b1;
    t0 = CAM_INF; t1 = -CAM_INF;
    if (cam_interval_tube(o, d, s0, a0, a1) && cam_interval_z(o.z, d.z, s1, b0, b1) && fmaxf(a0, b0) <= fminf(a1, b1)) {
      t0 = fmaxf(a0, b0); t1 = fminf(a1, b1); hit = true;
    }
    for (int k = 0; k < 2; k++)
      if (cam_interval_sphere(v3(o.x, o.y, o.z - (k ? -s1 : s1)), d, s0, a0, a1)) { t0 = fminf(t0, a0); t1 = fmaxf(t1, a1); hit = true; }
    return hit;
  }
  if (type == GT_BOX) {
    float a0, a1;
    t0 = -CAM_INF; t1 = CAM_INF;
    if (!cam_interval_z(o.x, d.x, s0, a0, a1)) return false;
    t0 = fmaxf(t0, a0); t1 = fminf(t1, a1);
    if (!cam_interval_z(o.y, d.y, s1, a0, a1)) return false;
    t0 = fmaxf(t0, a0); t1 = fminf(t1, a1);
    if (!cam_interval_z(o.z, d.z, s2, a0, a1)) return false;
    t0 = fmaxf(t0, a0); t1 = fminf(t1, a1);
    return t0 <= t1;
  }
  if (type == GT_MESH) { // half-space clipping against the hull's face planes n . x <= c
    const int p0 = __float_as_int(G[CGW_PADR]), np = __float_as_int(G[CGW_PNUM]);
    t0 = -CAM_INF; t1 = CAM_INF;
    for (int k = 0; k < np; k++) {
      const float *pl = planes + 4 * (p0 + k);
      const V3 n = ldv3(pl);
      const float nd = dot(n, d), rest = pl[3] - dot(n, o);
      if (fabsf(nd) < 1e-30f) { if (rest < 0.0f) return false; continue; }
      const float t = rest / nd;
      if (nd > 0.0f) t1 = fminf(t1, t); else t0 = fmaxf(t0, t);
    }
    return t0 <= t1;
  }
  return false;
}

__global__ __launch_bounds__(256) void k_cam_ray(CamRayArgs a, const float *__restrict__ pose, const float *__restrict__ cgtab,
                                                 const float *__restrict__ planes_g, float *__restrict__ depth, int *__restrict__ seg) {
  extern __shared__ float cam_lds[];
  float *G = cam_lds;                                     // [ncg][CAM_GW]
  float *PL = G + CAM_GW * a.ncg;                         // [nplanes][4]
  int *lists = reinterpret_cast<int *>(PL + 4 * a.nplanes); // [4 waves][FSIM_CAM_MAX_GEOMS]
  int blk = blockIdx.x;
  const int tx = blk % a.ntx; blk /= a.ntx;
  const int ty = blk % a.nty; blk /= a.nty;
  const int cam = blk % a.ncam, e = blk / a.ncam;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const float *P = pose + (size_t)e * a.pstride;
  // stage the env's geom table and the hull planes (k_cam_normal holds the same three loops: moved into a shared function, the compiler
  // unrolled them differently here and the smallest render measured slower, so they stay written out -- DESIGN.md 11)
  for (int i = tid; i < CAM_PW * a.ncg; i += 256) G[CAM_GW * (i / CAM_PW) + i % CAM_PW] = P[i];
  for (int i = tid; i < CAM_SW * a.ncg; i += 256) G[CAM_GW * (i / CAM_SW) + CAM_PW + i % CAM_SW] = cgtab[i];
  for (int i = tid; i < 4 * a.nplanes; i += 256) PL[i] = planes_g[i];
  __syncthreads();
  const V3 co = ldv3(P + CAM_PW * (a.ncg + cam));
  const M3 Rc = ldm3(P + CAM_PW * (a.ncg + cam) + 3);
  const float s = a.slope[cam], zn = a.znear[cam], zf = a.zfar[cam];
  // this wave's 16 x 16 quarter of the tile: pixel columns x0 .. x1, rows y0 .. y1 (empty past the image's edge)
  const int x0 = tx * CAM_TILE + (w & 1) * 16, y0 = ty * CAM_TILE + (w >> 1) * 16;
  const int x1 = min(x0 + 15, a.W - 1), y1 = min(y0 + 15, a.H - 1);
  const bool live = x0 < a.W && y0 < a.H;
  // ray of pixel (i, j) in the camera frame: (cx(i), cy(j), -1), so that t along it IS the depth along the optical axis
  const float hw = 0.5f * a.W, hh = 0.5f * a.H;
  const float xl = (x0 + 0.5f - hw) * s, xr = (x1 + 0.5f - hw) * s, yt = (hh - y0 - 0.5f) * s, yb = (hh - y1 - 0.5f) * s;
  // cull: a geom's bounding sphere against the four side planes (through the camera centre and the outer pixel centres) and the
  // depth range; ballot order keeps the list in geom order
  int *list = lists + FSIM_CAM_MAX_GEOMS * w;
  int nl = 0;
  for (int g0 = 0; g0 < a.ncg; g0 += 64) {
    const int g = g0 + lane;
    bool keep = false;
    if (live && g < a.ncg) {
      const float *Gg = G + CAM_GW * g;
      if (__float_as_int(Gg[CGW_TYPE]) == GT_PLANE) keep = true;
      else {
        const V3 c = multv(Rc, ldv3(Gg + CGW_POS) - co); // centre in the camera frame
        const float r = Gg[CGW_RB] * 1.0001f + 1e-5f;
        keep = -c.z + r >= zn && -c.z - r <= zf &&
               (c.x + xl * c.z) * rsqrtf(1.0f + xl * xl) >= -r && (-c.x - xr * c.z) * rsqrtf(1.0f + xr * xr) >= -r &&
               (c.y + yb * c.z) * rsqrtf(1.0f + yb * yb) >= -r && (-c.y - yt * c.z) * rsqrtf(1.0f + yt * yt) >= -r;
      }
    }
    const unsigned long long mask = __ballot(keep);
    if (keep) list[nl + __popcll(mask & ((1ull << lane) - 1ull))] = g;
    nl += __popcll(mask);
  }
  __syncthreads();
  if (!live) return;
  // lane -> column x0 + (lane & 15), rows y0 + (lane >> 4) + 4 k
  const int px = x0 + (lane & 15), pyb = y0 + (lane >> 4);
  const float cx = (px + 0.5f - hw) * s;
  float best[4];
  int id[4];
  for (int k = 0; k < 4; k++) { best[k] = CAM_INF; id[k] = -1; }
  for (int li = 0; li < nl; li++) {
    const float *Gg = G + CAM_GW * list[li];
    const M3 Rg = ldm3(Gg + CGW_MAT);
    const V3 o = multv(Rg, co - ldv3(Gg + CGW_POS)); // camera centre in the geom frame
    const M3 M = mulm(M3{{Rg.m[0], Rg.m[3], Rg.m[6], Rg.m[1], Rg.m[4], Rg.m[7], Rg.m[2], Rg.m[5], Rg.m[8]}}, Rc); // camera -> geom frame
    const int type = __float_as_int(Gg[CGW_TYPE]), gid = __float_as_int(Gg[CGW_ID]);
    for (int k = 0; k < 4; k++) {
      const float cy = (hh - (pyb + 4 * k) - 0.5f) * s;
      const V3 d = mulv(M, v3(cx, cy, -1.0f));
      float t0, t1;
      if (!cam_interval(type, o, d, Gg, PL, t0, t1)) continue;
      const float t = t0 >= zn ? t0 : t1; // the nearest surface point at or beyond the near plane
      if (t >= zn && t <= zf && t < best[k]) { best[k] = t; id[k] = gid; }
    }
  }
  if (px > x1) return;
  const size_t img = ((size_t)e * a.ncam + cam) * a.H;
  for (int k = 0; k < 4; k++) {
    const int py = pyb + 4 * k;
    if (py > y1) break;
    const size_t o = (img + py) * a.W + px;
    if (depth) depth[o] = id[k] >= 0 ? best[k] : zf;
    if (seg) seg[o] = id[k];
  }
}

// ------------------------------------------------------------------------------------------ host
static float cam_bits(int v) { float f; memcpy(&f, &v, 4); return f; }
struct CamState {
  int ncam = 0, W = 0, H = 0, nplanes = 0, pstride = 0;
  float slope[FSIM_CAM_MAX] = {}, znear[FSIM_CAM_MAX] = {}, zfar[FSIM_CAM_MAX] = {};
  float *d_cams = nullptr, *d_cg = nullptr, *d_planes = nullptr, *d_pose = nullptr;
  float *d_depth = nullptr; int *d_seg = nullptr; // image scratch of the derived observations (cam_render_images), [n_envs * npix]
};

static void flw_free(fsim *s); // fsim_flow.hpp
static void cam_free(fsim *s) {
  if (!s->cam) return;
  hipFree(s->cam->d_cams); hipFree(s->cam->d_cg); hipFree(s->cam->d_planes); hipFree(s->cam->d_pose);
  hipFree(s->cam->d_depth); hipFree(s->cam->d_seg);
  delete s->cam;
  s->cam = nullptr;
}

// What fsim_set_cameras and fsim_set_rays (fsim_rays.hpp) read of the model blob to place a body-mounted frame and to build the static
// geom rows
struct CamMountTables {
  std::vector<int> body_red, cg_type, cg_orig, cursor_body;
  std::vector<float> relpos, relquat, cg_size, cg_rbound;
};

static int cam_mount_tables(const fsim *s, CamMountTables &t) {
  if (!blob_i(s->blob, "body_red", t.body_red) || !blob_f(s->blob, "body_relpos", t.relpos) || !blob_f(s->blob, "body_relquat", t.relquat) ||
      !blob_i(s->blob, "cg_type", t.cg_type) || !blob_i(s->blob, "cg_orig", t.cg_orig) || !blob_f(s->blob, "cg_size", t.cg_size) ||
      !blob_f(s->blob, "cg_rbound", t.cg_rbound))
    return FSIM_EINVAL;
  if (s->m.agent == 2 && !blob_i(s->blob, "cursor_bodyid", t.cursor_body)) return FSIM_EINVAL;
  return FSIM_OK;
}

// k_cam_pose's arguments for the handle's model: nframes mounted frames (cameras, sensors) behind the geoms, pstride words per env
static CamPoseArgs cam_pose_args(const fsim *s, int nframes, int pstride) {
  const DModel &m = s->m;
  return CamPoseArgs{kin_args(s), m.cg_body, m.cg_cursor, m.cg_pos, m.cg_mat, m.cursor_pos0,
                     m.ncg, nframes, m.agent == 2 ? s->ly.env + E_GROUP + m.nparts + EC_POS : -1, pstride};
}

// One d_cams row (CCW_*) of a frame (pos, quat wxyz) given in the frame of model body `body` (-1: the world), composed in double.
// Nonzero: a pose that is not finite or has no orientation.
static int cam_mount_row(const CamMountTables &t, int body, const float *pos, const float *quat, float *r) {
  double q[4] = {quat[0], quat[1], quat[2], quat[3]}, p[3] = {pos[0], pos[1], pos[2]};
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!(qn > 1e-12) || !std::isfinite(qn) || !std::isfinite(p[0] + p[1] + p[2])) return 1;
  for (double &x : q) x /= qn;
  int rbody = 0, cur = -1;
  if (body >= 0) { // (body_relpos, body_relquat) of the body in its reduced body (x) the frame's pose, in double
    const int b = body;
    const double rp[3] = {t.relpos[3 * b], t.relpos[3 * b + 1], t.relpos[3 * b + 2]}, rq[4] = {t.relquat[4 * b], t.relquat[4 * b + 1], t.relquat[4 * b + 2], t.relquat[4 * b + 3]};
    const double u[3] = {rq[1], rq[2], rq[3]};
    const double tt[3] = {2 * (u[1] * p[2] - u[2] * p[1]), 2 * (u[2] * p[0] - u[0] * p[2]), 2 * (u[0] * p[1] - u[1] * p[0])};
    const double np_[3] = {rp[0] + p[0] + rq[0] * tt[0] + (u[1] * tt[2] - u[2] * tt[1]), rp[1] + p[1] + rq[0] * tt[1] + (u[2] * tt[0] - u[0] * tt[2]),
                           rp[2] + p[2] + rq[0] * tt[2] + (u[0] * tt[1] - u[1] * tt[0])};
    const double nq[4] = {rq[0] * q[0] - rq[1] * q[1] - rq[2] * q[2] - rq[3] * q[3], rq[0] * q[1] + rq[1] * q[0] + rq[2] * q[3] - rq[3] * q[2],
                          rq[0] * q[2] - rq[1] * q[3] + rq[2] * q[0] + rq[3] * q[1], rq[0] * q[3] + rq[1] * q[2] - rq[2] * q[1] + rq[3] * q[0]};
    for (int j = 0; j < 3; j++) p[j] = np_[j];
    for (int j = 0; j < 4; j++) q[j] = nq[j];
    rbody = t.body_red[b];
    for (size_t j = 0; j < t.cursor_body.size(); j++)
      if (t.cursor_body[j] == b) cur = (int)j; // a cursor moves with the env's cursor position, not with its (world) body
  }
  r[CCW_RBODY] = cam_bits(rbody); r[CCW_CURSOR] = cam_bits(cur);
  for (int j = 0; j < 3; j++) r[CCW_POS + j] = (float)p[j];
  for (int j = 0; j < 4; j++) r[CCW_QUAT + j] = (float)q[j];
  return 0;
}

// The static rows (CAM_SW words) of every colliding geom, with the hull-plane slices checked; who: the caller's name for the messages
static int cam_geom_rows(const DModel &m, const CamMountTables &t, const char *who, int n_planes, const float *hull_planes, const int32_t *hull_adr,
                         const int32_t *hull_num, std::vector<float> &cg) {
  cg.assign((size_t)CAM_SW * m.ncg, 0.0f);
  for (int g = 0; g < m.ncg; g++) {
    float *r = cg.data() + CAM_SW * g;
    for (int j = 0; j < 3; j++) r[j] = t.cg_size[3 * g + j];
    r[3] = t.cg_rbound[g];
    int adr = 0, num = 0;
    if (t.cg_type[g] == GT_MESH) {
      if (!hull_adr || !hull_num || !hull_planes) FAIL(FSIM_EINVAL, "%s: colliding geom %d is a convex mesh and no hull planes were given", who, g);
      adr = hull_adr[g]; num = hull_num[g];
      if (num < 4 || adr < 0 || adr + num > n_planes) FAIL(FSIM_EINVAL, "%s: hull planes of colliding geom %d out of range (%d + %d of %d)", who, g, adr, num, n_planes);
    }
    r[4] = cam_bits(t.cg_type[g]); r[5] = cam_bits(adr); r[6] = cam_bits(num); r[7] = cam_bits(t.cg_orig[g]);
  }
  for (int i = 0; i < 4 * n_planes; i++)
    if (!std::isfinite(hull_planes[i])) FAIL(FSIM_EINVAL, "%s: hull plane table holds a non-finite value", who);
  return FSIM_OK;
}

extern "C" int fsim_set_cameras(fsim_t *s, int n_cam, const fsim_camera_t *cams, int n_planes, const float *hull_planes, const int32_t *hull_adr,
                                const int32_t *hull_num) {
  if (!s || !cams) FAIL(FSIM_EINVAL, "fsim_set_cameras: null argument");
  if (n_cam < 1 || n_cam > FSIM_CAM_MAX) FAIL(FSIM_EINVAL, "fsim_set_cameras: %d cameras (1 .. %d)", n_cam, FSIM_CAM_MAX);
  const DModel &m = s->m;
  if (m.ncg > FSIM_CAM_MAX_GEOMS) FAIL(FSIM_EINVAL, "fsim_set_cameras: %d colliding geoms (the ray pass stages at most %d)", m.ncg, FSIM_CAM_MAX_GEOMS);
  if (n_planes < 0 || n_planes > FSIM_CAM_MAX_PLANES) FAIL(FSIM_EINVAL, "fsim_set_cameras: %d hull planes (at most %d)", n_planes, FSIM_CAM_MAX_PLANES);
  CamMountTables mt;
  { int rc_ = cam_mount_tables(s, mt); if (rc_) return rc_; }
  CamState c;
  c.ncam = n_cam; c.W = cams[0].width; c.H = cams[0].height; c.nplanes = n_planes;
  std::vector<float> crow((size_t)CCW_WORDS * n_cam, 0.0f);
  for (int i = 0; i < n_cam; i++) {
    const fsim_camera_t &k = cams[i];
    if (k.body < -1 || k.body >= m.nbody) FAIL(FSIM_EINVAL, "camera %d: unknown body %d (the model has %d bodies)", i, k.body, m.nbody);
    if (!(k.fovy_deg > 0.0f && k.fovy_deg < 180.0f)) FAIL(FSIM_EINVAL, "camera %d: fovy %g not in (0, 180) degrees", i, k.fovy_deg);
    if (!(k.znear > 0.0f) || !(k.zfar > k.znear) || !std::isfinite(k.zfar)) FAIL(FSIM_EINVAL, "camera %d: needs 0 < znear < zfar (got %g, %g)", i, k.znear, k.zfar);
    if (k.width < 1 || k.height < 1 || k.width > FSIM_CAM_MAX_SIZE || k.height > FSIM_CAM_MAX_SIZE)
      FAIL(FSIM_EINVAL, "camera %d: size %d x %d (1 .. %d each)", i, k.width, k.height, FSIM_CAM_MAX_SIZE);
    if (k.width != c.W || k.height != c.H) FAIL(FSIM_EINVAL, "camera %d: size %d x %d differs from camera 0's %d x %d", i, k.width, k.height, c.W, c.H);
    if (cam_mount_row(mt, k.body, k.pos, k.quat, crow.data() + CCW_WORDS * i)) FAIL(FSIM_EINVAL, "camera %d: bad pose", i);
    c.slope[i] = (float)(tan(k.fovy_deg * (3.14159265358979323846 / 360.0)) / (0.5 * c.H));
    c.znear[i] = k.znear; c.zfar[i] = k.zfar;
  }
  std::vector<float> cg;
  { int rc_ = cam_geom_rows(m, mt, "fsim_set_cameras", n_planes, hull_planes, hull_adr, hull_num, cg); if (rc_) return rc_; }
  c.pstride = (CAM_PW * (m.ncg + n_cam) + 3) / 4 * 4;
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; }
  HIPCHK(hipStreamSynchronize(s->stream)); // (a render in flight still reads the old tables)
  cam_free(s);
  flw_free(s); // (the twist scratch of fsim_render_flow is sized by the camera set)
  s->cam = new CamState(c);
  CamState &k = *s->cam;
  HIPCHK(hipMalloc(&k.d_cams, crow.size() * 4));
  HIPCHK(hipMalloc(&k.d_cg, cg.size() * 4));
  HIPCHK(hipMalloc(&k.d_planes, (size_t)4 * std::max(n_planes, 1) * 4));
  HIPCHK(hipMalloc(&k.d_pose, (size_t)s->n_envs * k.pstride * 4));
  HIPCHK(hipMemcpy(k.d_cams, crow.data(), crow.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(k.d_cg, cg.data(), cg.size() * 4, hipMemcpyHostToDevice));
  if (n_planes) HIPCHK(hipMemcpy(k.d_planes, hull_planes, (size_t)16 * n_planes, hipMemcpyHostToDevice));
  return FSIM_OK;
}

extern "C" int fsim_render(fsim_t *s, float *depth_dev, int32_t *seg_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_render: null handle");
  if (!s->cam) FAIL(FSIM_EINVAL, "fsim_render: no cameras set (fsim_set_cameras)");
  if (!depth_dev && !seg_dev) FAIL(FSIM_EINVAL, "fsim_render: no output (depth and segmentation both NULL)");
  HIPCHK(hipSetDevice(s->device));
  { int rc_ = settle(s); if (rc_) return rc_; } // the state fsim_sync leaves: overflowed envs re-stepped first
  const CamState &k = *s->cam;
  const DModel &m = s->m;
  hipLaunchKernelGGL(k_cam_pose, dim3(s->n_envs), dim3(64), 0, s->stream, cam_pose_args(s, k.ncam, k.pstride), s->d_state, k.d_cams, k.d_pose);
  HIPCHK(hipGetLastError());
  CamRayArgs ra{};
  ra.ncg = m.ncg; ra.ncam = k.ncam; ra.W = k.W; ra.H = k.H; ra.ntx = (k.W + CAM_TILE - 1) / CAM_TILE; ra.nty = (k.H + CAM_TILE - 1) / CAM_TILE;
  ra.nplanes = k.nplanes; ra.pstride = k.pstride;
  for (int i = 0; i < FSIM_CAM_MAX; i++) { ra.slope[i] = k.slope[i]; ra.znear[i] = k.znear[i]; ra.zfar[i] = k.zfar[i]; }
  const size_t lds = 4 * ((size_t)CAM_GW * m.ncg + 4 * k.nplanes + 4 * FSIM_CAM_MAX_GEOMS);
  const size_t nblk = (size_t)s->n_envs * k.ncam * ra.ntx * ra.nty;
  if (nblk > 0x7fffffff) FAIL(FSIM_EINVAL, "fsim_render: %zu workgroups", nblk);
  hipLaunchKernelGGL(k_cam_ray, dim3((unsigned)nblk), dim3(256), lds, s->stream, ra, k.d_pose, k.d_cg, k.d_planes, depth_dev, seg_dev);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}

static CamView cam_view(const fsim *s) {
  const CamState &k = *s->cam;
  CamView v{};
  v.ncam = k.ncam; v.W = k.W; v.H = k.H; v.npix = k.ncam * k.W * k.H; v.ncg = s->m.ncg; v.pstride = k.pstride;
  for (int i = 0; i < FSIM_CAM_MAX; i++) v.slope[i] = k.slope[i];
  return v;
}

// The render of fsim_render_points / _voxels / _normals (cameras set, device current): fsim_render into the caller's images, and for a
// NULL one into the handle's image scratch -- one for the three of them, allocated on first use.  It lives as long as the camera set:
// the image size changes with fsim_set_cameras alone, which waits for the stream and then frees it (cam_free).  *depth, *seg: the
// images to read.
static int cam_render_images(fsim *s, float *depth_dev, int32_t *seg_dev, const float **depth, const int **seg) {
  CamState &k = *s->cam;
  const size_t nimg = (size_t)s->n_envs * k.ncam * k.W * k.H;
  if (!depth_dev && !k.d_depth) HIPCHK(hipMalloc(&k.d_depth, nimg * 4));
  if (!seg_dev && !k.d_seg) HIPCHK(hipMalloc(&k.d_seg, nimg * 4));
  float *d = depth_dev ? depth_dev : k.d_depth;
  int *g = seg_dev ? seg_dev : k.d_seg;
  *depth = d; *seg = g;
  return fsim_render(s, d, g); // settles, then k_cam_pose + k_cam_ray
}
