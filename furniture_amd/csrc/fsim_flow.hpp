// fsim_flow.hpp -- optical-flow and surface-velocity images from the cameras (include/fsim_flow.h).  Included at the end of fsim.hip,
// after fsim_normals.hpp: the host part renders through cam_render_images (fsim_render: k_cam_pose, k_cam_ray, as they are); the pixel
// kernel stages the camera poses with cam_stage_views and back-projects through pts_point, the function k_pts_gather, k_vox_bin and
// k_cam_normal call.
//
// After fsim_render's two launches, on the same stream:
//   k_cam_twist  one wave per env, like k_cam_pose: qpos of the env record (read only) -> world pose of every reduced body (stages (A)
//                and (B) of k_cam_pose: fsim_kin.hpp), qvel -> each body's own joint twist expressed about the WORLD ORIGIN, so that
//                the twists of a chain add; one more pointer-doubling round set over r_parent sums them with plain sums (stages (T)
//                and (U), in fsim_kin.hpp too: k_frame_state runs them as well).  Out:
//                6 words (v at the origin of the pose row, w) per colliding geom and per camera, [n_envs][ncg + ncam][6].
//   k_cam_flow   one 256-thread workgroup per (env, camera, chunk of up to FLW_CHUNK pixels), the shape of k_cam_normal.  The geom
//                origins, the geom and camera twists, the camera poses and the model-geom-id -> colliding-geom table are staged in LDS
//                once; then every lane takes one pixel per round from coalesced reads of depth and seg and evaluates the header's
//                formulas.  Each output is three dword stores per lane (12-byte stride between lanes), the layout DESIGN.md 14 measured
//                faster than staging through LDS for the normal image.
// No atomics, no scratch: every word is written once, and an env's output depends on nothing but its record, its images and its poses.
#include "../../include/fsim_flow.h"

#define FLW_THREADS 256 // k_cam_flow
#define FLW_CHUNK 2048  // pixels per workgroup: eight rounds share one staging of the tables
#define FLW_TW 6        // twist words: v (at the row's origin), w

struct FlwTwistArgs {
  CamPoseArgs p;
  int tstride /* twist words per env */;
};

__global__ __launch_bounds__(64) void k_cam_twist(FlwTwistArgs t, const float *__restrict__ state, const float *__restrict__ cams,
                                                  const float *__restrict__ pose, float *__restrict__ twist) {
  __shared__ float sp[3 * 32], sq[4 * 32], sv[3 * 32], sw[3 * 32];
  __shared__ int sanc[32];
  const CamPoseArgs &a = t.p;
  const int e = blockIdx.x, b = threadIdx.x;
  const float *rec = state + (size_t)e * a.kin.stride;
  const float *P0 = pose + (size_t)e * a.pstride; // what k_cam_pose wrote for this env in this very call
  float *out = twist + (size_t)e * t.tstride;
  // (A) + (B): k_cam_pose keeps the geoms' and cameras' poses only, and the joint twists need every reduced body's; then (T) the body's
  //     own joint twist about the world origin and (U) its sum up the tree: fsim_kin.hpp
  V3 P, v0, w;
  Q4 Q;
  const KinLane l = kin_joint_pose(a.kin, rec, b, &P, &Q);
  kin_world_poses(a.kin, l, b, sp, sq, sanc, &P, &Q);
  kin_joint_twist(a.kin, l, rec, P, Q, &v0, &w);
  kin_sum_twists(a.kin, l, b, sv, sw, sanc, v0, w);
  __syncthreads();
  // (V) per colliding geom and per camera: the twist of its reduced body, taken at the origin of its pose row.  The cursor offset in
  //     that origin is a teleport between steps: it moves the point, it adds no velocity (the cursor bodies hang on reduced body 0).
  for (int g = b; g < a.ncg + a.ncam; g += 64) {
    const int rb = g < a.ncg ? a.cg_body[g] : __float_as_int(cams[CCW_WORDS * (g - a.ncg) + CCW_RBODY]);
    const V3 wb = ldv3(sw + 3 * rb);
    stv3(out + FLW_TW * g, ldv3(sv + 3 * rb) + cross(wb, ldv3(P0 + CAM_PW * g)));
    stv3(out + FLW_TW * g + 3, wb);
  }
}

struct FlwArgs {
  CamView v;
  int hw /* W * H */, ngeom, nchunk, tstride;
};

__global__ __launch_bounds__(FLW_THREADS) void k_cam_flow(FlwArgs a, const float *__restrict__ pose, const float *__restrict__ twist,
                                                          const unsigned char *__restrict__ idtab_g, const float *__restrict__ depth,
                                                          const int *__restrict__ seg, float *__restrict__ flow, float *__restrict__ velocity) {
  extern __shared__ float flw_lds[];
  const int nrow = a.v.ncg + a.v.ncam;
  float *gpos = flw_lds;                         // [ncg][3]
  float *tw = gpos + 3 * a.v.ncg;                // [ncg + ncam][FLW_TW]
  float *cpose = tw + FLW_TW * nrow;             // [FSIM_CAM_MAX][CAM_PW]
  float *cslope = cpose + FSIM_CAM_MAX * CAM_PW; // [FSIM_CAM_MAX]
  unsigned char *idtab = reinterpret_cast<unsigned char *>(cslope + FSIM_CAM_MAX); // [ngeom]
  int blk = blockIdx.x;
  const int chunk = blk % a.nchunk; blk /= a.nchunk;
  const int cam = blk % a.v.ncam, e = blk / a.v.ncam, tid = threadIdx.x;
  const float *P = pose + (size_t)e * a.v.pstride;
  const float *T = twist + (size_t)e * a.tstride;
  for (int i = tid; i < 3 * a.v.ncg; i += FLW_THREADS) gpos[i] = P[CAM_PW * (i / 3) + i % 3];
  for (int i = tid; i < FLW_TW * nrow; i += FLW_THREADS) tw[i] = T[i];
  cam_stage_views(cpose, cslope, P + CAM_PW * a.v.ncg, a.v, tid, FLW_THREADS);
  for (int i = tid; i < a.ngeom; i += FLW_THREADS) idtab[i] = idtab_g[i];
  __syncthreads();
  const V3 pc = ldv3(cpose + CAM_PW * cam);
  const M3 Rc = ldm3(cpose + CAM_PW * cam + 3);
  const V3 vc = ldv3(tw + FLW_TW * (a.v.ncg + cam)), wc = ldv3(tw + FLW_TW * (a.v.ncg + cam) + 3);
  const float s = cslope[cam], hw = 0.5f * a.v.W, hh = 0.5f * a.v.H;
  const int c0 = chunk * FLW_CHUNK, len = min(FLW_CHUNK, a.hw - c0); // this workgroup's pixels of the (env, camera) image
  const size_t img = (size_t)e * a.v.npix + (size_t)cam * a.hw + c0;    // the first of them, in pixels of the whole batch
  for (int r0 = 0; r0 < len; r0 += FLW_THREADS) {
    const int r = r0 + tid;
    if (r >= len) break;
    V3 f = v3(0.0f, 0.0f, 0.0f), u = v3(0.0f, 0.0f, 0.0f);
    const int g = seg[img + r];
    const float d = depth[img + r];
    if (g >= 0 && g < a.ngeom) {
      const int ci = idtab[g];
      if (ci != NRM_NOGEOM) { // (always: the ray pass names colliding geoms only)
        const V3 q = pts_point(cpose, cslope, a.v.W, a.v.H, cam * a.hw + c0 + r, d);
        u = ldv3(tw + FLW_TW * ci) + cross(ldv3(tw + FLW_TW * ci + 3), q - ldv3(gpos + 3 * ci));
        if (flow) {
          const V3 X = multv(Rc, u - vc - cross(wc, q - pc)); // camera-frame rate of the material point
          const int row = (c0 + r) / a.v.W, col = (c0 + r) - row * a.v.W;
          const float cx = (col + 0.5f - hw) * s, cy = (hh - row - 0.5f) * s;
          const float dd = -X.z, inv = 1.0f / (d * s);
          f = v3((X.x - cx * dd) * inv, -((X.y - cy * dd) * inv), dd);
        }
      }
    }
    if (flow) stv3(flow + 3 * (img + r), f); // (a wave's 64 pixels: 768 contiguous bytes over three dword stores)
    if (velocity) stv3(velocity + 3 * (img + r), u);
  }
}

// ------------------------------------------------------------------------------------------ host
struct FlwState {
  float *d_twist = nullptr;         // [n_envs][ncg + ncam][FLW_TW]
  unsigned char *d_idtab = nullptr; // [ngeom] model geom id -> colliding geom (nrm_idtab)
};

static void flw_free(fsim *s) { // (fsim_set_cameras calls it after its stream wait, fsim_destroy after its own)
  if (!s->flw) return;
  hipFree(s->flw->d_twist); hipFree(s->flw->d_idtab);
  delete s->flw;
  s->flw = nullptr;
}

extern "C" int fsim_render_flow(fsim_t *s, float *depth_dev, int32_t *seg_dev, float *flow_dev, float *velocity_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_render_flow: null handle");
  if (!s->cam) FAIL(FSIM_EINVAL, "fsim_render_flow: no cameras set (fsim_set_cameras)");
  if (!flow_dev && !velocity_dev) FAIL(FSIM_EINVAL, "fsim_render_flow: no output (flow and velocity both NULL)");
  const CamState &k = *s->cam;
  const DModel &m = s->m;
  if (m.nr > 32) FAIL(FSIM_EINVAL, "fsim_render_flow: %d reduced bodies (the twist pass holds at most 32)", m.nr);
  const int hw = k.W * k.H, nrow = m.ncg + k.ncam;
  const int nchunk = (hw + FLW_CHUNK - 1) / FLW_CHUNK;
  const size_t nblk = (size_t)s->n_envs * k.ncam * nchunk;
  if (nblk > 0x7fffffff) FAIL(FSIM_EINVAL, "fsim_render_flow: %zu workgroups", nblk);
  const size_t lds = 4 * ((size_t)3 * m.ncg + (size_t)FLW_TW * nrow + FSIM_CAM_MAX * CAM_PW + FSIM_CAM_MAX) + (size_t)s->ngeom;
  if (lds > 65536) FAIL(FSIM_EINVAL, "fsim_render_flow: %d geoms need %zu bytes of LDS (at most 65536)", s->ngeom, lds);
  HIPCHK(hipSetDevice(s->device));
  if (!s->flw) { // first use with this camera set: the id table and the twist scratch
    std::vector<unsigned char> idtab;
    { int rc_ = nrm_idtab(s, idtab); if (rc_) return rc_; }
    FlwState f;
    HIPCHK(hipMalloc(&f.d_idtab, idtab.size()));
    if (hipMalloc(&f.d_twist, (size_t)s->n_envs * nrow * FLW_TW * 4) != hipSuccess) { hipFree(f.d_idtab); FAIL(FSIM_EHIP, "fsim_render_flow: no memory for the twist scratch"); }
    if (hipMemcpy(f.d_idtab, idtab.data(), idtab.size(), hipMemcpyHostToDevice) != hipSuccess) { hipFree(f.d_idtab); hipFree(f.d_twist); FAIL(FSIM_EHIP, "fsim_render_flow: id table upload failed"); }
    s->flw = new FlwState(f);
  }
  const FlwState &v = *s->flw;
  const float *depth;
  const int *seg;
  { int rc_ = cam_render_images(s, depth_dev, seg_dev, &depth, &seg); if (rc_) return rc_; }
  FlwTwistArgs ta{};
  ta.p = cam_pose_args(s, k.ncam, k.pstride);
  ta.p.ecpos = -1;
  ta.tstride = nrow * FLW_TW;
  hipLaunchKernelGGL(k_cam_twist, dim3(s->n_envs), dim3(64), 0, s->stream, ta, s->d_state, k.d_cams, k.d_pose, v.d_twist);
  HIPCHK(hipGetLastError());
  FlwArgs fa{};
  fa.v = cam_view(s); fa.hw = hw; fa.ngeom = s->ngeom; fa.nchunk = nchunk; fa.tstride = ta.tstride;
  hipLaunchKernelGGL(k_cam_flow, dim3((unsigned)nblk), dim3(FLW_THREADS), lds, s->stream, fa, k.d_pose, v.d_twist, v.d_idtab, depth, seg, flow_dev, velocity_dev);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
