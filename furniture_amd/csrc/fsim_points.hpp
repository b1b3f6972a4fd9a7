// fsim_points.hpp -- point-cloud observations built from the cameras (include/fsim_points.h).  Included at the end of fsim.hip, after
// fsim_camera.hpp: the host part renders through cam_render_images (fsim_render: k_cam_pose, k_cam_ray, as they are) and the kernel
// stages the camera poses k_cam_pose leaves in the handle's pose scratch with cam_stage_views.  The kept-pixel rule (pts_seg_kept,
// pts_in_box) and the keep-table / box helpers of the settings calls are here for fsim_voxels.hpp as well.
//
// After fsim_render's two launches, on the same stream:
//   k_pts_gather  one 256-thread workgroup per env: back-projects every pixel of the env's images to the world frame, applies the
//                 kept-pixel test and compacts the kept pixels, in (camera, row, column) order, into the env's candidate buffer
//                 (xyz + pix) and its count -- __ballot + mbcnt within a wave, a double-buffered LDS prefix across the four waves.
//                 Dense mode: it writes the outputs directly, and nothing else runs.
//   k_pts_fps     one 512-thread workgroup per env (sampled mode): the env's candidates and their dmin live in VGPRs (candidate
//                 j * 512 + tid in slot j of thread tid, PER slots); per row every lane updates its dmin and takes its best, the wave
//                 reduces the 64-bit key (dmin bits << 32 | ~index) with __shfl_xor, and the eight wave winners -- key and xyz --
//                 meet in a double-buffered LDS slot: one barrier per row.
// No atomics: an env's output depends on nothing but its images, its camera poses and the settings.
#include "../../include/fsim_points.h"

#define PTS_GTHREADS 256 // k_pts_gather
#define PTS_FTHREADS 512 // k_pts_fps

struct PtsGatherArgs {
  CamView v;
  int dense;
  float lo[3], hi[3]; // crop box (+-inf: none)
};

// The world point of pixel p = cam*H*W + row*W + col at depth d (the header's formula): k_cam_ray's ray of pixel (col, row), turned and
// moved by the camera pose k_cam_pose leaves (cpose: CAM_PW words per camera, cslope: the cameras' slopes).  k_pts_gather and k_vox_bin
// (fsim_voxels.hpp) both call it, so a voxel's points are the dense map's bit for bit.  It is written out operation by operation, the
// fused multiply-adds exactly where hipcc's default contraction put them when k_pts_gather held this code inline (every other product
// and sum rounded on its own): left to the contraction, the same source compiled into two kernels can fuse different products (the
// SLP vectorizer pairs the rows differently), and the two kernels' points then differ in the last bit.
DEV V3 pts_point(const float *cpose, const float *cslope, int W, int H, int p, float d) {
#pragma clang fp contract(off)
  const int hw_ = W * H;
  const float hw = 0.5f * W, hh = 0.5f * H;
  const int cam = p / hw_, rem = p - cam * hw_, row = rem / W, col = rem - row * W;
  const float s = cslope[cam];
  const float cx = (col + 0.5f - hw) * s, cy = (hh - row - 0.5f) * s; // k_cam_ray's ray of pixel (col, row)
  const float *c = cpose + CAM_PW * cam, *R = c + 3;                  // position, rotation (row-major)
  const float m0 = __builtin_fmaf(R[1], cy, R[0] * cx) - R[2];        // R (cx, cy, -1)
  const float m1 = __builtin_fmaf(R[3], cx, R[4] * cy) - R[5];
  const float m2 = __builtin_fmaf(R[6], cx, R[7] * cy) - R[8];
  return v3(__builtin_fmaf(m0, d, c[0]), __builtin_fmaf(m1, d, c[1]), __builtin_fmaf(m2, d, c[2])); // pos + (R ray) * depth
}

// The kept-pixel rule of the header, in its two halves: the pixel sees a geom of the keep table (k_vox_bin asks this one first and
// back-projects only then), and its world point lies in the closed box.
DEV bool pts_seg_kept(int g, const unsigned char *keep) { return g >= 0 && keep[g]; }
DEV bool pts_in_box(V3 q, const float *lo, const float *hi) {
  return q.x >= lo[0] && q.y >= lo[1] && q.z >= lo[2] && q.x <= hi[0] && q.y <= hi[1] && q.z <= hi[2];
}

__global__ __launch_bounds__(PTS_GTHREADS) void k_pts_gather(PtsGatherArgs a, const float *__restrict__ pose, const float *__restrict__ depth,
                                                             const int *__restrict__ seg, const unsigned char *__restrict__ keep,
                                                             float *__restrict__ xyz, int *__restrict__ pseg, f4_t *__restrict__ cand,
                                                             int *__restrict__ count) {
  __shared__ float cpose[FSIM_CAM_MAX * CAM_PW], cslope[FSIM_CAM_MAX];
  __shared__ int wcnt[2][PTS_GTHREADS / 64];
  const int e = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  cam_stage_views(cpose, cslope, pose + (size_t)e * a.v.pstride + CAM_PW * a.v.ncg, a.v, tid, PTS_GTHREADS);
  __syncthreads();
  const size_t base = (size_t)e * a.v.npix;
  int total = 0, buf = 0;
  for (int p0 = 0; p0 < a.v.npix; p0 += PTS_GTHREADS) {
    const int p = p0 + tid;
    bool kept = false;
    V3 q = v3(0.0f, 0.0f, 0.0f);
    if (p < a.v.npix) {
      const int g = seg[base + p];
      q = pts_point(cpose, cslope, a.v.W, a.v.H, p, depth[base + p]);
      kept = pts_seg_kept(g, keep) && pts_in_box(q, a.lo, a.hi);
      if (a.dense) {
        stv3(xyz + 3 * (base + p), q);
        pseg[base + p] = kept ? g : -1;
      }
    }
    // order-preserving compaction: lanes below in this wave (mbcnt), then the waves below in this workgroup (LDS prefix)
    const unsigned long long m = __ballot(kept);
    if (lane == 0) wcnt[buf][w] = __popcll(m);
    __syncthreads(); // (double-buffered: the next chunk writes the other half, so one barrier per chunk)
    int off = 0, tot = 0;
    for (int k = 0; k < PTS_GTHREADS / 64; k++) {
      const int c = wcnt[buf][k];
      off += k < w ? c : 0;
      tot += c;
    }
    if (kept && !a.dense) {
      const int at = total + off + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      f4_t v;
      v.x = q.x; v.y = q.y; v.z = q.z; v.w = __int_as_float(p);
      cand[base + at] = v;
    }
    total += tot;
    buf ^= 1;
  }
  if (tid == 0) count[e] = total;
}

// dist2 of the header: ((dx*dx + dy*dy) + dz*dz), every operation rounded on its own (hipcc contracts by default)
DEV float pts_dist2(float x, float y, float z, float px, float py, float pz) {
#pragma clang fp contract(off)
  const float dx = x - px, dy = y - py, dz = z - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

template <int PER>
__global__ __launch_bounds__(PTS_FTHREADS) void k_pts_fps(int npix, int n_points, const f4_t *__restrict__ cand, const int *__restrict__ count,
                                                          const int *__restrict__ seg, float *__restrict__ xyz, int *__restrict__ pseg,
                                                          int *__restrict__ pix) {
  __shared__ unsigned long long skey[2][PTS_FTHREADS / 64];
  __shared__ float sxyz[2][PTS_FTHREADS / 64][4];
  __shared__ int sel[FSIM_PTS_MAX_POINTS]; // candidate index of every row
  const int e = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  const size_t base = (size_t)e * npix;
  const int K = count[e], M = min(K, n_points);
  float x[PER], y[PER], z[PER], d[PER];
#pragma unroll
  for (int j = 0; j < PER; j++) { // slots past the env's count: dmin -1, never chosen (they load candidate 0, inside the buffer)
    const int c = j * PTS_FTHREADS + tid;
    const bool ok = c < K;
    const f4_t v = cand[base + (ok ? c : 0)];
    x[j] = ok ? v.x : 0.0f; y[j] = ok ? v.y : 0.0f; z[j] = ok ? v.z : 0.0f;
    d[j] = ok ? __int_as_float(0x7f800000) : -1.0f;
  }
  float px = 0.0f, py = 0.0f, pz = 0.0f; // the previous row: row 0 is candidate 0
  if (K > 0) {
    const f4_t v = cand[base];
    px = v.x; py = v.y; pz = v.z;
  }
  if (tid == 0) sel[0] = 0;
  int buf = 0;
  for (int r = 1; r < M; r++) {
    float best = -1.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
    int bj = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) { // ascending j, strict >: the lane's smallest index wins its ties
      if (j * PTS_FTHREADS < K) { // (uniform: slots j and up hold no candidate of this env when it fails)
        const float d2 = pts_dist2(x[j], y[j], z[j], px, py, pz);
        d[j] = d2 < d[j] ? d2 : d[j];
        const bool gt = d[j] > best;
        best = gt ? d[j] : best; bj = gt ? j : bj;
        bx = gt ? x[j] : bx; by = gt ? y[j] : by; bz = gt ? z[j] : bz;
      }
    }
    // dmin >= 0: its float bits order as unsigned; ~index makes the smaller index the larger key.  0: no candidate in this lane
    const unsigned long long key = best >= 0.0f ? ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)~(unsigned)(bj * PTS_FTHREADS + tid) : 0ull;
    unsigned long long wk = key;
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long t = __shfl_xor(wk, o);
      wk = t > wk ? t : wk;
    }
    if (key == wk) { // the wave's winner (keys of candidates are unique; a wave without one: every lane writes 0)
      skey[buf][w] = key;
      sxyz[buf][w][0] = bx; sxyz[buf][w][1] = by; sxyz[buf][w][2] = bz;
    }
    __syncthreads(); // (double-buffered: row r + 1 writes the other slot, so one barrier per row)
    unsigned long long gk = skey[buf][0];
    int gw = 0;
    for (int k = 1; k < PTS_FTHREADS / 64; k++) {
      const unsigned long long t = skey[buf][k];
      if (t > gk) { gk = t; gw = k; }
    }
    px = sxyz[buf][gw][0]; py = sxyz[buf][gw][1]; pz = sxyz[buf][gw][2];
    if (tid == 0) sel[r] = (int)~(unsigned)gk;
    buf ^= 1;
  }
  __syncthreads();
  for (int r = tid; r < n_points; r += PTS_FTHREADS) {
    const size_t o = (size_t)e * n_points + r;
    if (K == 0) {
      stv3(xyz + 3 * o, v3(0.0f, 0.0f, 0.0f));
      pseg[o] = -1; pix[o] = -1;
      continue;
    }
    const f4_t v = cand[base + sel[r < M ? r : 0]]; // rows K .. N-1 repeat row 0
    const int p = __float_as_int(v.w);
    stv3(xyz + 3 * o, v3(v.x, v.y, v.z));
    pix[o] = p;
    pseg[o] = seg[base + p];
  }
}

// ------------------------------------------------------------------------------------------ host
struct PtsState {
  int n_points = 0;
  float lo[3], hi[3];
  unsigned char *d_keep = nullptr; // [ngeom]
  f4_t *d_cand = nullptr;          // candidates (sampled mode), [n_envs * npix]
  size_t cap_cand = 0;             // elements allocated
};

static void pts_free(fsim *s) {
  if (!s->pts) return;
  hipFree(s->pts->d_keep); hipFree(s->pts->d_cand);
  delete s->pts;
  s->pts = nullptr;
}

// the finite half of the two box rules (who: the entry point, for the message)
static int pts_box_finite(const char *who, const float *box) {
  for (int i = 0; i < 6; i++)
    if (!std::isfinite(box[i])) FAIL(FSIM_EINVAL, "%s: box bound %d is not finite", who, i);
  return FSIM_OK;
}

// The geom_keep table of fsim_set_points / fsim_set_voxels on the device, [max(ngeom, 1)] bytes (NULL: every geom kept): *d_keep is
// allocated by the first call.  The caller has waited for the stream: a render in flight still reads the old table.
static int pts_upload_keep(fsim *s, const uint8_t *geom_keep, unsigned char **d_keep) {
  std::vector<unsigned char> keep(std::max(s->ngeom, 1), 1);
  if (geom_keep)
    for (int g = 0; g < s->ngeom; g++) keep[g] = geom_keep[g] ? 1 : 0;
  if (!*d_keep) HIPCHK(hipMalloc(d_keep, keep.size()));
  HIPCHK(hipMemcpy(*d_keep, keep.data(), keep.size(), hipMemcpyHostToDevice));
  return FSIM_OK;
}

extern "C" int fsim_set_points(fsim_t *s, int n_points, const uint8_t *geom_keep, const float *box) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_set_points: null handle");
  if (n_points < 0 || n_points > FSIM_PTS_MAX_POINTS) FAIL(FSIM_EINVAL, "fsim_set_points: n_points %d (0 .. %d)", n_points, FSIM_PTS_MAX_POINTS);
  if (box) {
    if (pts_box_finite("fsim_set_points", box)) return FSIM_EINVAL;
    for (int i = 0; i < 3; i++)
      if (box[i] > box[3 + i]) FAIL(FSIM_EINVAL, "fsim_set_points: box lo %g > hi %g on axis %d", box[i], box[3 + i], i);
  }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream)); // (a render in flight still reads the old keep table)
  if (!s->pts) s->pts = new PtsState();
  PtsState &p = *s->pts;
  p.n_points = n_points;
  for (int i = 0; i < 3; i++) {
    p.lo[i] = box ? box[i] : -INFINITY;
    p.hi[i] = box ? box[3 + i] : INFINITY;
  }
  return pts_upload_keep(s, geom_keep, &p.d_keep);
}

extern "C" int fsim_render_points(fsim_t *s, float *depth_dev, int32_t *seg_dev, float *xyz_dev, int32_t *pseg_dev, int32_t *pix_dev,
                                  int32_t *count_dev) {
  if (!s) FAIL(FSIM_EINVAL, "fsim_render_points: null handle");
  if (!s->pts) FAIL(FSIM_EINVAL, "fsim_render_points: no points settings (fsim_set_points)");
  if (!s->cam) FAIL(FSIM_EINVAL, "fsim_render_points: no cameras set (fsim_set_cameras)");
  PtsState &p = *s->pts;
  const CamState &k = *s->cam;
  const long npix = (long)k.ncam * k.W * k.H; // checked here: fsim_set_cameras may have changed the size since fsim_set_points
  if (npix > FSIM_PTS_MAX_PIXELS)
    FAIL(FSIM_EINVAL, "fsim_render_points: %d camera(s) of %d x %d = %ld pixels per env (at most %d)", k.ncam, k.W, k.H, npix, FSIM_PTS_MAX_PIXELS);
  if (!xyz_dev || !pseg_dev || !count_dev || (p.n_points > 0 && !pix_dev)) FAIL(FSIM_EINVAL, "fsim_render_points: a NULL output");
  HIPCHK(hipSetDevice(s->device));
  const size_t nimg = (size_t)s->n_envs * npix;
  if (p.n_points > 0 && p.cap_cand < nimg) { // scratch, allocated on first use and grown with the image size
    HIPCHK(hipStreamSynchronize(s->stream));
    hipFree(p.d_cand);
    p.d_cand = nullptr; p.cap_cand = 0;
    HIPCHK(hipMalloc(&p.d_cand, nimg * sizeof(f4_t)));
    p.cap_cand = nimg;
  }
  const float *depth;
  const int *seg;
  { int rc_ = cam_render_images(s, depth_dev, seg_dev, &depth, &seg); if (rc_) return rc_; }
  PtsGatherArgs ga{};
  ga.v = cam_view(s); ga.dense = p.n_points == 0;
  for (int i = 0; i < 3; i++) { ga.lo[i] = p.lo[i]; ga.hi[i] = p.hi[i]; }
  hipLaunchKernelGGL(k_pts_gather, dim3(s->n_envs), dim3(PTS_GTHREADS), 0, s->stream, ga, k.d_pose, depth, seg, p.d_keep,
                     ga.dense ? xyz_dev : nullptr, ga.dense ? pseg_dev : nullptr, p.d_cand, count_dev);
  HIPCHK(hipGetLastError());
  if (ga.dense) return FSIM_OK;
  // candidate slots per thread: the fewest that hold every pixel (fewer VGPRs, more workgroups per CU for small images)
  if (npix <= 8 * PTS_FTHREADS)
    hipLaunchKernelGGL(k_pts_fps<8>, dim3(s->n_envs), dim3(PTS_FTHREADS), 0, s->stream, (int)npix, p.n_points, p.d_cand, count_dev, seg, xyz_dev, pseg_dev, pix_dev);
  else if (npix <= 16 * PTS_FTHREADS)
    hipLaunchKernelGGL(k_pts_fps<16>, dim3(s->n_envs), dim3(PTS_FTHREADS), 0, s->stream, (int)npix, p.n_points, p.d_cand, count_dev, seg, xyz_dev, pseg_dev, pix_dev);
  else
    hipLaunchKernelGGL(k_pts_fps<32>, dim3(s->n_envs), dim3(PTS_FTHREADS), 0, s->stream, (int)npix, p.n_points, p.d_cand, count_dev, seg, xyz_dev, pseg_dev, pix_dev);
  HIPCHK(hipGetLastError());
  return FSIM_OK;
}
