/* fsim_oracle_collide.inc -- P3 collision (included by fsim_oracle.c; test infrastructure).
 *
 * Pair filtering: static candidate list (same-weld-body, parent-child and <exclude>
 * filters applied by the model compiler) x the run-time mutable contype/conaffinity
 * masks the env rewrites (furniture/env/furniture.py:866-878, 1441-1461, 1586-1595),
 * then bounding spheres, then a primitive narrow phase.  Contact convention: frame
 * row 0 = normal pointing from geom1 to geom2, dist < 0 = penetration, pos = midpoint.
 */

typedef struct { real dist, pos[3], n[3]; } CPoint;

static void make_frame(real *f) {
  real *x = f, *y = f + 3, *z = f + 6;
  normalize3(x);
  if (x[1] > -0.5 && x[1] < 0.5) { y[0] = 0; y[1] = 1; y[2] = 0; } else { y[0] = 0; y[1] = 0; y[2] = 1; }
  real d = dot3(x, y);
  addscl3(y, y, x, -d);
  normalize3(y);
  cross3(z, x, y);
}

static inline void col(real *c, const real *R, int k) { c[0] = R[k]; c[1] = R[3 + k]; c[2] = R[6 + k]; }

/* ---- plane vs X (geom1 = plane) */
static int plane_sphere(const real *pp, const real *pR, const real *sp, real r, real margin, CPoint *out) {
  real n[3], d[3];
  col(n, pR, 2); sub3(d, sp, pp);
  real dist = dot3(d, n) - r;
  if (dist > margin) return 0;
  out->dist = dist; copy3(out->n, n);
  addscl3(out->pos, sp, n, -(r + 0.5 * dist));
  return 1;
}
static int plane_box(const real *pp, const real *pR, const real *bp, const real *bR, const real *size, real margin, CPoint *out) {
  real n[3], d[3];
  col(n, pR, 2); sub3(d, bp, pp);
  real dist0 = dot3(d, n);
  int cnt = 0;
  for (int i = 0; i < 8; i++) {
    real v[3] = {(i & 1) ? size[0] : -size[0], (i & 2) ? size[1] : -size[1], (i & 4) ? size[2] : -size[2]}, c[3];
    mulMV(c, bR, v);
    real ld = dot3(n, c);
    if (dist0 + ld > margin || ld > 0) continue;
    out[cnt].dist = dist0 + ld; copy3(out[cnt].n, n);
    real t[3];
    addscl3(t, c, n, -0.5 * out[cnt].dist);
    add3(out[cnt].pos, t, bp);
    if (++cnt >= 4) return 4;
  }
  return cnt;
}
static int plane_cylinder(const real *pp, const real *pR, const real *cp, const real *cR, const real *size, real margin, CPoint *out) {
  real n[3], axis[3], vec[3], d[3];
  col(n, pR, 2); col(axis, cR, 2);
  real prjaxis = dot3(n, axis);
  if (prjaxis > 0) { scl3(axis, axis, -1); prjaxis = -prjaxis; }
  sub3(d, cp, pp);
  real dist0 = dot3(d, n);
  scl3(vec, axis, prjaxis); sub3(vec, vec, n);
  real len2 = dot3(vec, vec);
  if (len2 >= 1e-12) scl3(vec, vec, size[0] / sqrt(len2));
  else { col(vec, cR, 0); scl3(vec, vec, size[0]); }
  real prjvec = dot3(vec, n);
  scl3(axis, axis, size[1]); prjaxis *= size[1];
  int cnt = 0;
  if (dist0 + prjaxis + prjvec > margin) return 0;
  out[0].dist = dist0 + prjaxis + prjvec; copy3(out[0].n, n);
  add3(out[0].pos, cp, vec); add3(out[0].pos, out[0].pos, axis); addscl3(out[0].pos, out[0].pos, n, -0.5 * out[0].dist);
  cnt = 1;
  if (dist0 - prjaxis + prjvec <= margin) {
    out[cnt].dist = dist0 - prjaxis + prjvec; copy3(out[cnt].n, n);
    add3(out[cnt].pos, cp, vec); sub3(out[cnt].pos, out[cnt].pos, axis); addscl3(out[cnt].pos, out[cnt].pos, n, -0.5 * out[cnt].dist);
    cnt++;
  }
  real prjvec1 = -0.5 * prjvec;
  if (dist0 + prjaxis + prjvec1 <= margin) {
    real v1[3];
    cross3(v1, vec, axis); normalize3(v1); scl3(v1, v1, size[0] * sqrt(3.0) * 0.5);
    for (int sgn = 1; sgn >= -1; sgn -= 2) {
      out[cnt].dist = dist0 + prjaxis + prjvec1; copy3(out[cnt].n, n);
      addscl3(out[cnt].pos, cp, v1, (real)sgn); add3(out[cnt].pos, out[cnt].pos, axis);
      addscl3(out[cnt].pos, out[cnt].pos, vec, -0.5); addscl3(out[cnt].pos, out[cnt].pos, n, -0.5 * out[cnt].dist);
      cnt++;
    }
  }
  return cnt;
}

/* ---- sphere vs X (geom1 = sphere) */
static int sphere_sphere(const real *p1, real r1, const real *p2, real r2, real margin, CPoint *out) {
  real d[3];
  sub3(d, p2, p1);
  real len = norm3(d), dist = len - r1 - r2;
  if (dist > margin) return 0;
  if (len < MINVAL) { d[0] = 1; d[1] = 0; d[2] = 0; } else scl3(d, d, 1.0 / len);
  out->dist = dist; copy3(out->n, d);
  addscl3(out->pos, p1, d, r1 + 0.5 * dist);
  return 1;
}
/* closest-feature helper: local centre c against a solid given by (clamped closest point q, inside flag) */
static int sphere_vs_local(const real *sp, real r, const real *oR, const real *c, const real *q, int inside,
                           const real *outdir_local, real pen, real margin, CPoint *out) {
  real nl[3], dist;
  if (!inside) {
    sub3(nl, q, c);
    real d = normalize3(nl);
    dist = d - r;
  } else {
    scl3(nl, outdir_local, -1); /* from sphere towards the solid's interior */
    dist = -pen - r;
  }
  if (dist > margin) return 0;
  mulMV(out->n, oR, nl);
  out->dist = dist;
  addscl3(out->pos, sp, out->n, r + 0.5 * dist);
  return 1;
}
static int sphere_box(const real *sp, real r, const real *bp, const real *bR, const real *size, real margin, CPoint *out) {
  real d[3], c[3], q[3], od[3] = {0, 0, 0};
  sub3(d, sp, bp); mulMTV(c, bR, d);
  int inside = 1;
  for (int k = 0; k < 3; k++) { q[k] = c[k] < -size[k] ? -size[k] : (c[k] > size[k] ? size[k] : c[k]); if (q[k] != c[k]) inside = 0; }
  real pen = 0;
  if (inside) {
    int kb = 0; pen = RSEL(1e300, 1e30);
    for (int k = 0; k < 3; k++) { real p = size[k] - fabs(c[k]); if (p < pen) { pen = p; kb = k; } }
    od[kb] = c[kb] >= 0 ? 1 : -1;
  }
  return sphere_vs_local(sp, r, bR, c, q, inside, od, pen, margin, out);
}
static int sphere_cylinder(const real *sp, real r, const real *cp, const real *cR, const real *size, real margin, CPoint *out) {
  real d[3], c[3], q[3], od[3] = {0, 0, 0};
  sub3(d, sp, cp); mulMTV(c, cR, d);
  real rho = sqrt(c[0] * c[0] + c[1] * c[1]), rc = size[0], h = size[1];
  int inside = (rho <= rc) && (fabs(c[2]) <= h);
  real pen = 0;
  if (inside) {
    real pr = rc - rho, pz = h - fabs(c[2]);
    if (pz < pr) { pen = pz; od[2] = c[2] >= 0 ? 1 : -1; }
    else { pen = pr; if (rho > MINVAL) { od[0] = c[0] / rho; od[1] = c[1] / rho; } else od[0] = 1; }
    copy3(q, c);
  } else {
    real sc = rho > rc ? rc / rho : 1.0;
    q[0] = c[0] * sc; q[1] = c[1] * sc; q[2] = c[2] < -h ? -h : (c[2] > h ? h : c[2]);
  }
  return sphere_vs_local(sp, r, cR, c, q, inside, od, pen, margin, out);
}

/* ---- box vs box: separating-axis test + face manifold.
 * The face manifold is the vertex set of (reference face rectangle) x (projected incident face quad): quad vertices
 * inside the rectangle, quad-edge x rectangle-side crossings, rectangle corners strictly inside the quad -- the same
 * points a Sutherland-Hodgman clip produces, enumerated without polygon buffers (the device kernel does the same). */
static int box_box(const real *p1, const real *R1, const real *s1, const real *p2, const real *R2, const real *s2, real margin, CPoint *out) {
  real A[3][3], B[3][3], d[3];
  for (int k = 0; k < 3; k++) { col(A[k], R1, k); col(B[k], R2, k); }
  sub3(d, p2, p1);
  real best = -RSEL(1e300, 1e30); int bestType = -1, bi = 0, bj = 0; real bestL[3] = {0, 0, 0};
  real C[3][3], AC[3][3];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { C[i][j] = dot3(A[i], B[j]); AC[i][j] = fabs(C[i][j]) + 1e-12; }
  /* face axes of box 1 */
  for (int i = 0; i < 3; i++) {
    real t = dot3(d, A[i]);
    real sep = fabs(t) - (s1[i] + s2[0] * AC[i][0] + s2[1] * AC[i][1] + s2[2] * AC[i][2]);
    if (sep > margin) return 0;
    if (sep > best) { best = sep; bestType = 0; bi = i; scl3(bestL, A[i], t < 0 ? -1.0 : 1.0); }
  }
  for (int j = 0; j < 3; j++) {
    real t = dot3(d, B[j]);
    real sep = fabs(t) - (s2[j] + s1[0] * AC[0][j] + s1[1] * AC[1][j] + s1[2] * AC[2][j]);
    if (sep > margin) return 0;
    if (sep > best) { best = sep; bestType = 1; bj = j; scl3(bestL, B[j], t < 0 ? -1.0 : 1.0); }
  }
  /* edge-edge axes; must beat the best face axis by a margin to be chosen (avoids jitter) */
  real bestE = -RSEL(1e300, 1e30); int ei = 0, ej = 0; real eL[3] = {0, 0, 0};
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
    real L[3];
    cross3(L, A[i], B[j]);
    real len = norm3(L);
    if (len < 1e-6) continue;
    scl3(L, L, 1.0 / len);
    real t = dot3(d, L), ra = 0, rb = 0;
    for (int k = 0; k < 3; k++) { ra += s1[k] * fabs(dot3(A[k], L)); rb += s2[k] * fabs(dot3(B[k], L)); }
    real sep = fabs(t) - (ra + rb);
    if (sep > margin) return 0;
    if (sep > bestE) { bestE = sep; ei = i; ej = j; scl3(eL, L, t < 0 ? -1.0 : 1.0); }
  }
  if (bestE > best + 1e-6 + 0.05 * fabs(best)) {
    /* edge-edge contact: support edges along eL */
    real n[3]; copy3(n, eL);
    real pa[3], pb[3];
    copy3(pa, p1); copy3(pb, p2);
    for (int k = 0; k < 3; k++) {
      if (k != ei) addscl3(pa, pa, A[k], dot3(A[k], n) > 0 ? s1[k] : -s1[k]);
      if (k != ej) addscl3(pb, pb, B[k], dot3(B[k], n) > 0 ? -s2[k] : s2[k]);
    }
    /* closest points of lines pa + s*A[ei], pb + t*B[ej] */
    real w[3]; sub3(w, pa, pb);
    real b = dot3(A[ei], B[ej]), dd = dot3(A[ei], w), e = dot3(B[ej], w), den = 1 - b * b;
    real sa = 0, tb = 0;
    if (den > 1e-12) { sa = (b * e - dd) / den; tb = (e - b * dd) / den; }
    sa = sa < -s1[ei] ? -s1[ei] : (sa > s1[ei] ? s1[ei] : sa);
    tb = tb < -s2[ej] ? -s2[ej] : (tb > s2[ej] ? s2[ej] : tb);
    addscl3(pa, pa, A[ei], sa); addscl3(pb, pb, B[ej], tb);
    out[0].dist = bestE; copy3(out[0].n, n);
    out[0].pos[0] = 0.5 * (pa[0] + pb[0]); out[0].pos[1] = 0.5 * (pa[1] + pb[1]); out[0].pos[2] = 0.5 * (pa[2] + pb[2]);
    return 1;
  }
  /* face contact */
  const real *pr, *pi_, *sr, *si; real (*Rr)[3], (*Ri)[3]; real nr[3]; int ka;
  if (bestType == 0) { pr = p1; pi_ = p2; sr = s1; si = s2; Rr = A; Ri = B; ka = bi; copy3(nr, bestL); }
  else { pr = p2; pi_ = p1; sr = s2; si = s1; Rr = B; Ri = A; ka = bj; scl3(nr, bestL, -1); }
  /* nr: outward normal of the reference face (points towards the incident box) */
  int kinc = 0; real mind = RSEL(1e300, 1e30); real sgninc = 1;
  for (int k = 0; k < 3; k++) { real t = dot3(Ri[k], nr); if (-fabs(t) < mind) { mind = -fabs(t); kinc = k; sgninc = t > 0 ? -1 : 1; } }
  int k1 = (kinc + 1) % 3, k2 = (kinc + 2) % 3, u1 = (ka + 1) % 3, u2 = (ka + 2) % 3;
  real fc[3];
  addscl3(fc, pi_, Ri[kinc], sgninc * si[kinc]);
  real rc[3];
  addscl3(rc, pr, nr, sr[ka]); /* reference face centre */
  real E1[3], E2[3], rcen[3];
  scl3(E1, Ri[k1], si[k1]); scl3(E2, Ri[k2], si[k2]);
  sub3(rcen, fc, rc);
  real cx = dot3(rcen, Rr[u1]), cy = dot3(rcen, Rr[u2]);
  real e1x = dot3(E1, Rr[u1]), e1y = dot3(E1, Rr[u2]), e2x = dot3(E2, Rr[u1]), e2y = dot3(E2, Rr[u2]);
  real hu = sr[u1], hv = sr[u2];
  real ninc[3]; scl3(ninc, Ri[kinc], sgninc);
  real denom = dot3(ninc, nr);
  real nout[3];
  if (bestType == 0) copy3(nout, nr); else scl3(nout, nr, -1); /* from geom1 to geom2 */
  int cnt = 0;
  real cand[12][2]; int ncand = 0;
  static const real SX[4] = {1, -1, -1, 1}, SY[4] = {1, 1, -1, -1};
  for (int q = 0; q < 4; q++) {
    real ax = cx + SX[q] * e1x + SY[q] * e2x, ay = cy + SX[q] * e1y + SY[q] * e2y;
    if (fabs(ax) <= hu && fabs(ay) <= hv && ncand < 12) { cand[ncand][0] = ax; cand[ncand][1] = ay; ncand++; }
    int q1 = (q + 1) & 3;
    real bx = cx + SX[q1] * e1x + SY[q1] * e2x, by = cy + SX[q1] * e1y + SY[q1] * e2y;
    for (int side = 0; side < 4; side++) {
      int xs = side < 2;
      real sg = (side & 1) ? -1.0 : 1.0, lim = xs ? hu : hv, olim = xs ? hv : hu;
      real da = sg * (xs ? ax : ay) - lim, db = sg * (xs ? bx : by) - lim;
      if (!((da < 0 && db > 0) || (da > 0 && db < 0))) continue;
      real t = da / (da - db);
      real px = ax + t * (bx - ax), py = ay + t * (by - ay);
      real o = fabs(xs ? py : px);
      if ((xs ? (o <= olim) : (o < olim)) && ncand < 12) { cand[ncand][0] = px; cand[ncand][1] = py; ncand++; }
    }
  }
  real det = e1x * e2y - e1y * e2x;
  if (fabs(det) > 1e-12) {
    for (int q = 0; q < 4; q++) {
      real x = SX[q] * hu - cx, y = SY[q] * hv - cy;
      real a = (x * e2y - y * e2x) / det, b = (e1x * y - e1y * x) / det;
      if (fabs(a) < 1.0 && fabs(b) < 1.0 && ncand < 12) { cand[ncand][0] = x + cx; cand[ncand][1] = y + cy; ncand++; }
    }
  }
  /* lift the 2-D points back onto the incident face plane and measure depth */
  for (int i = 0; i < ncand && cnt < 8; i++) {
    real q[3];
    addscl3(q, rc, Rr[u1], cand[i][0]); addscl3(q, q, Rr[u2], cand[i][1]);
    /* q + h*nr lies on incident plane: (q + h nr - fc).ninc = 0 */
    real t[3]; sub3(t, fc, q);
    real h = fabs(denom) > 1e-9 ? dot3(t, ninc) / denom : 0.0;
    if (h > margin) continue;
    real pos[3];
    addscl3(pos, q, nr, 0.5 * h);
    out[cnt].dist = h; copy3(out[cnt].n, nout); copy3(out[cnt].pos, pos);
    cnt++;
  }
  return cnt;
}

/* plane - capsule: the two end spheres of the capsule against the plane (MuJoCo's mjc_PlaneCapsule; robots/baxter/robot.xml:61 is the one
 * capsule of the in-scope assets) */
static int plane_capsule(const real *pp, const real *pR, const real *cp, const real *cR, const real *size, real margin, CPoint *out) {
  real ax[3], e[3];
  int cnt = 0;
  col(ax, cR, 2);
  for (int k = 0; k < 2; k++) {
    for (int q = 0; q < 3; q++) e[q] = cp[q] + (k ? -1.0 : 1.0) * size[1] * ax[q];
    cnt += plane_sphere(pp, pR, e, size[0], margin, out + cnt);
  }
  return cnt;
}

/* plane - convex mesh: the hull's lowest vertex, then the vertices a slightly tilted "down" picks in three directions 120 degrees apart
 * (the scheme of MuJoCo's mjc_PlaneConvex); every distinct vertex within the margin is a contact, at most four */
static void mesh_support(const real *verts, int n, const real *dl, real *pl);
static int plane_mesh(const real *pp, const real *pR, const real *mp, const real *mR, const real *verts, int n, real margin, CPoint *out) {
  real nw[3], t1[3], t2[3], prev[4][3];
  int seen = 0, cnt = 0;
  col(nw, pR, 2); col(t1, pR, 0); col(t2, pR, 1);
  for (int k = 0; k < 4; k++) {
    real dw[3] = {-nw[0], -nw[1], -nw[2]}, dl[3], vl[3], vw[3], d[3];
    if (k > 0) { real a = 2.0943951023931953 * (k - 1); for (int q = 0; q < 3; q++) dw[q] += (t1[q] * cos(a) + t2[q] * sin(a)) * 1e-3; }
    mulMTV(dl, mR, dw);
    mesh_support(verts, n, dl, vl);
    int dup = 0;
    for (int j = 0; j < seen; j++) if (prev[j][0] == vl[0] && prev[j][1] == vl[1] && prev[j][2] == vl[2]) dup = 1;
    if (dup) continue;
    for (int q = 0; q < 3; q++) prev[seen][q] = vl[q];
    seen++;
    mulMV(vw, mR, vl); add3(vw, vw, mp);
    sub3(d, vw, pp);
    real dist = dot3(d, nw);
    if (dist > margin) continue;
    out[cnt].dist = dist;
    for (int q = 0; q < 3; q++) { out[cnt].pos[q] = vw[q] - 0.5 * dist * nw[q]; out[cnt].n[q] = nw[q]; }
    cnt++;
  }
  return cnt;
}

/* ---- generic convex pair via Minkowski portal refinement (cylinder-box, cylinder-cylinder; every pair with a capsule or a convex mesh in it) */
typedef struct { int type; const real *pos, *R, *size; const real *verts; int nvert; } Shape; /* verts / nvert: hull of a convex mesh */
/* the hull vertex furthest along the local direction dl (first one on ties) */
static void mesh_support(const real *verts, int n, const real *dl, real *pl) {
  real best = -RSEL(1e300, 1e30);
  pl[0] = pl[1] = pl[2] = 0;
  for (int i = 0; i < n; i++) {
    real d = dot3(verts + 3 * i, dl);
    if (d > best) { best = d; pl[0] = verts[3 * i]; pl[1] = verts[3 * i + 1]; pl[2] = verts[3 * i + 2]; }
  }
}
static void support(const Shape *sh, const real *dir, real *out) {
  real dl[3], pl[3];
  mulMTV(dl, sh->R, dir);
  if (sh->type == G_MESH) mesh_support(sh->verts, sh->nvert, dl, pl);
  else if (sh->type == G_BOX) {
    for (int k = 0; k < 3; k++) pl[k] = dl[k] >= 0 ? sh->size[k] : -sh->size[k];
  } else if (sh->type == G_CYLINDER) {
    real rho = sqrt(dl[0] * dl[0] + dl[1] * dl[1]);
    if (rho > 1e-12) { pl[0] = dl[0] / rho * sh->size[0]; pl[1] = dl[1] / rho * sh->size[0]; } else { pl[0] = pl[1] = 0; }
    pl[2] = dl[2] >= 0 ? sh->size[1] : -sh->size[1];
  } else { /* sphere; capsule = sphere swept along the local z axis: the same point plus the end of the segment the direction favours */
    real n = norm3(dl);
    if (n > 1e-12) scl3(pl, dl, sh->size[0] / n); else { pl[0] = pl[1] = pl[2] = 0; }
    if (sh->type == G_CAPSULE) pl[2] += dl[2] >= 0 ? sh->size[1] : -sh->size[1];
  }
  mulMV(out, sh->R, pl);
  add3(out, out, sh->pos);
}
typedef struct { real v[3], a[3], b[3]; } SupPt; /* v = b - a in the Minkowski difference B (-) A */
static void msupport(const Shape *A, const Shape *B, const real *dir, SupPt *s) {
  real nd[3];
  scl3(nd, dir, -1);
  support(A, nd, s->a); support(B, dir, s->b);
  sub3(s->v, s->b, s->a);
}
static int mpr_convex(const Shape *A, const Shape *B, CPoint *out) {
  /* returns 1 with depth/normal(A->B)/pos when the shapes interpenetrate */
  SupPt v0, v1, v2, v3, v4;
  real n[3], t[3], t2[3];
  copy3(v0.a, A->pos); copy3(v0.b, B->pos); sub3(v0.v, v0.b, v0.a);
  if (dot3(v0.v, v0.v) < 1e-20) v0.v[0] = 1e-5;
  scl3(n, v0.v, -1); normalize3(n);
  msupport(A, B, n, &v1);
  if (dot3(v1.v, n) <= 0) return 0;
  cross3(n, v1.v, v0.v);
  if (dot3(n, n) < 1e-20) {
    /* origin on the ray v0->v1: penetration along that ray */
    sub3(n, v1.v, v0.v); normalize3(n);
    out->dist = -dot3(v1.v, n); copy3(out->n, n); /* placeholder sign fixed below */
    scl3(out->n, n, -1);
    out->pos[0] = 0.5 * (v1.a[0] + v1.b[0]); out->pos[1] = 0.5 * (v1.a[1] + v1.b[1]); out->pos[2] = 0.5 * (v1.a[2] + v1.b[2]);
    return 1;
  }
  normalize3(n);
  msupport(A, B, n, &v2);
  if (dot3(v2.v, n) <= 0) return 0;
  sub3(t, v1.v, v0.v); sub3(t2, v2.v, v0.v); cross3(n, t, t2);
  if (dot3(n, v0.v) > 0) { SupPt tmp = v1; v1 = v2; v2 = tmp; scl3(n, n, -1); }
  for (int it = 0;; it++) {
    if (it > 64) return 0;
    normalize3(n);
    msupport(A, B, n, &v3);
    if (dot3(v3.v, n) <= 0) return 0;
    cross3(t, v1.v, v3.v);
    if (dot3(t, v0.v) < 0) { v2 = v3; sub3(t, v1.v, v0.v); sub3(t2, v3.v, v0.v); cross3(n, t, t2); continue; }
    cross3(t, v3.v, v2.v);
    if (dot3(t, v0.v) < 0) { v1 = v3; sub3(t, v3.v, v0.v); sub3(t2, v2.v, v0.v); cross3(n, t, t2); continue; }
    break;
  }
  int hit = 0;
  for (int it = 0; it < 64; it++) {
    sub3(t, v2.v, v1.v); sub3(t2, v3.v, v1.v); cross3(n, t, t2);
    if (normalize3(n) == 0) return 0;
    real dpl = dot3(n, v1.v);
    if (dpl >= 0) hit = 1;
    msupport(A, B, n, &v4);
    real delta = dot3(v4.v, n) - dot3(v3.v, n);
    if (dot3(v4.v, n) < 0 && !hit) return 0;
    if (delta <= RSEL(1e-7, 1e-6) || it == 63) {
      if (!hit) return 0;
      /* barycentric weights of the origin's projection in the portal */
      real b0, b1, b2, b3, c[3];
      cross3(c, v1.v, v2.v); b0 = dot3(c, v3.v);
      cross3(c, v3.v, v2.v); b1 = dot3(c, v0.v);
      cross3(c, v0.v, v1.v); b2 = dot3(c, v3.v);
      cross3(c, v2.v, v1.v); b3 = dot3(c, v0.v);
      real sum = b0 + b1 + b2 + b3;
      if (sum <= 0) {
        b0 = 0;
        cross3(c, v2.v, v3.v); b1 = dot3(c, n);
        cross3(c, v3.v, v1.v); b2 = dot3(c, n);
        cross3(c, v1.v, v2.v); b3 = dot3(c, n);
        sum = b1 + b2 + b3;
      }
      real pa[3], pb[3];
      for (int k = 0; k < 3; k++) {
        pa[k] = (b0 * v0.a[k] + b1 * v1.a[k] + b2 * v2.a[k] + b3 * v3.a[k]) / sum;
        pb[k] = (b0 * v0.b[k] + b1 * v1.b[k] + b2 * v2.b[k] + b3 * v3.b[k]) / sum;
      }
      /* n points out of the Minkowski difference B(-)A along the exit direction, i.e. moving B by +depth*n... */
      out->dist = -dpl;
      scl3(out->n, n, -1); /* from A towards B is opposite to the exit direction of (B - A) relative to origin */
      for (int k = 0; k < 3; k++) out->pos[k] = 0.5 * (pa[k] + pb[k]);
      return 1;
    }
    cross3(t, v4.v, v0.v);
    if (dot3(v1.v, t) > 0) { if (dot3(v2.v, t) > 0) v1 = v4; else v3 = v4; }
    else { if (dot3(v3.v, t) > 0) v2 = v4; else v1 = v4; }
  }
  return 0;
}

/* ---- contact record assembly (parameter mixing: equal priority -> max friction, solmix-weighted solref/solimp) */
static void add_contact(osim_t *s, int g1, int g2, const CPoint *c, real margin, real gap) {
  Model *m = &s->m;
  if (s->ncon >= MAXCON) { s->ndropped++; return; }
  Contact *k = &s->contact[s->ncon];
  k->dist = c->dist; copy3(k->pos, c->pos); copy3(k->frame, c->n);
  memset(k->frame + 3, 0, 6 * sizeof(real));
  make_frame(k->frame);
  k->includemargin = margin - gap;
  real f1 = m->geom_friction[3 * g1], f2 = m->geom_friction[3 * g2];
  k->mu = f1 > f2 ? f1 : f2;
  real mix = m->geom_solmix[g1] / (m->geom_solmix[g1] + m->geom_solmix[g2]);
  for (int i = 0; i < 2; i++) k->solref[i] = mix * m->geom_solref[2 * g1 + i] + (1 - mix) * m->geom_solref[2 * g2 + i];
  for (int i = 0; i < 5; i++) k->solimp[i] = mix * m->geom_solimp[5 * g1 + i] + (1 - mix) * m->geom_solimp[5 * g2 + i];
  k->geom1 = g1; k->geom2 = g2;
  int d1 = m->geom_condim[g1], d2 = m->geom_condim[g2];
  k->dim = d1 > d2 ? d1 : d2;
  if (k->mu < MINVAL) k->dim = 1; /* frictionless pair: normal row only */
  k->efc_address = -1;
  s->contact_geom1[s->ncon] = g1; s->contact_geom2[s->ncon] = g2;
  s->ncon++;
}

/* ---- the narrow phase of ONE pair: geom 1 has the lower type number (the caller orders the pair); verts / n: hull vertices of a G_MESH geom
 * (geom frame).  Returns the number of contacts written to out (at most 8), or -1 when no routine serves the two types.  collide() and
 * osim_narrowphase (the per-pair entry the narrow-phase tests call) share this one copy. */
static int narrowphase_pair(int t1, const real *p1, const real *R1, const real *s1, const real *verts1, int n1,
                            int t2, const real *p2, const real *R2, const real *s2, const real *verts2, int n2, real margin, CPoint *cp) {
  if (t1 == G_PLANE && t2 == G_SPHERE) return plane_sphere(p1, R1, p2, s2[0], margin, cp);
  if (t1 == G_PLANE && t2 == G_BOX) return plane_box(p1, R1, p2, R2, s2, margin, cp);
  if (t1 == G_PLANE && t2 == G_CYLINDER) return plane_cylinder(p1, R1, p2, R2, s2, margin, cp);
  if (t1 == G_SPHERE && t2 == G_SPHERE) return sphere_sphere(p1, s1[0], p2, s2[0], margin, cp);
  if (t1 == G_SPHERE && t2 == G_BOX) return sphere_box(p1, s1[0], p2, R2, s2, margin, cp);
  if (t1 == G_SPHERE && t2 == G_CYLINDER) return sphere_cylinder(p1, s1[0], p2, R2, s2, margin, cp);
  if (t1 == G_BOX && t2 == G_BOX) return box_box(p1, R1, s1, p2, R2, s2, margin, cp);
  if (t1 == G_PLANE && t2 == G_CAPSULE) return plane_capsule(p1, R1, p2, R2, s2, margin, cp);
  if (t1 == G_PLANE && t2 == G_MESH && verts2 && n2 > 0) return plane_mesh(p1, R1, p2, R2, verts2, n2, margin, cp);
  if ((t1 == G_CYLINDER && t2 == G_BOX) || (t1 == G_CYLINDER && t2 == G_CYLINDER) ||
      ((t1 == G_CAPSULE || t2 == G_CAPSULE || t2 == G_MESH) && t1 != G_PLANE && t1 != G_ELLIPSOID && t2 != G_ELLIPSOID &&
       (t1 != G_MESH || (verts1 && n1 > 0)) && (t2 != G_MESH || (verts2 && n2 > 0)))) {
    /* sphere / capsule / cylinder / box / mesh against a capsule or a convex mesh: the portal routine with their support functions.
     * It takes no margin: such a pair is a contact only once the two shapes interpenetrate (the device's np_mpr does the same) */
    Shape A = {t1, p1, R1, s1, t1 == G_MESH ? verts1 : NULL, t1 == G_MESH ? n1 : 0}, B = {t2, p2, R2, s2, t2 == G_MESH ? verts2 : NULL, t2 == G_MESH ? n2 : 0};
    return mpr_convex(&A, &B, cp);
  }
  return -1;
}

static void collide(osim_t *s) {
  Model *m = &s->m;
  s->ncon = 0;
  for (int p = 0; p < m->npair; p++) {
    int g1 = m->pair_geom[2 * p], g2 = m->pair_geom[2 * p + 1];
    int ct1 = m->geom_contype[g1], ca1 = m->geom_conaffinity[g1], ct2 = m->geom_contype[g2], ca2 = m->geom_conaffinity[g2];
    if (!((ct1 & ca2) || (ct2 & ca1))) continue;
    if (m->geom_type[g1] > m->geom_type[g2]) { int t = g1; g1 = g2; g2 = t; }
    int t1 = m->geom_type[g1], t2 = m->geom_type[g2];
    real margin = m->geom_margin[g1] > m->geom_margin[g2] ? m->geom_margin[g1] : m->geom_margin[g2];
    real gap = m->geom_gap[g1] > m->geom_gap[g2] ? m->geom_gap[g1] : m->geom_gap[g2];
    const real *p1 = s->geom_xpos + 3 * g1, *p2 = s->geom_xpos + 3 * g2, *R1 = s->geom_xmat + 9 * g1, *R2 = s->geom_xmat + 9 * g2;
    const real *s1 = m->geom_size + 3 * g1, *s2 = m->geom_size + 3 * g2;
    if (t1 != G_PLANE) {
      real d[3]; sub3(d, p2, p1);
      real bound = m->geom_rbound[g1] + m->geom_rbound[g2] + margin;
      if (dot3(d, d) > bound * bound) continue;
    } else {
      real n[3], d[3]; col(n, R1, 2); sub3(d, p2, p1);
      if (dot3(d, n) > m->geom_rbound[g2] + margin) continue;
    }
    CPoint cp[16];
    const real *v1 = NULL, *v2 = NULL;
    int n1 = 0, n2 = 0;
    if (t1 == G_MESH && m->mesh_vert) { v1 = m->mesh_vert + 3 * m->geom_meshadr[g1]; n1 = m->geom_meshnum[g1]; }
    if (t2 == G_MESH && m->mesh_vert) { v2 = m->mesh_vert + 3 * m->geom_meshadr[g2]; n2 = m->geom_meshnum[g2]; }
    int n = narrowphase_pair(t1, p1, R1, s1, v1, n1, t2, p2, R2, s2, v2, n2, margin, cp);
    if (n < 0) { fprintf(stderr, "fsim_oracle: no narrow-phase routine for geom types %d x %d (the model compiler refuses such pairs)\n", t1, t2); abort(); }
    for (int i = 0; i < n; i++) add_contact(s, g1, g2, &cp[i], margin, gap);
  }
}
