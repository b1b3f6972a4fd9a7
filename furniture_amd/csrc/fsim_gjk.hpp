// fsim_gjk.hpp -- the signed distance of one pair of convex shapes, with witness points (include/fsim_pairs.h: "Contract per pair").
// Includable on its own (tests/pair_distance_probe.hip calls gjk_pair case by case); fsim_pairs.hpp runs it one pair per lane.
//
//   plane pairs        the closed form d = -h_X(-n) - n . p_plane;
//   everything else    an fp32 GJK distance iteration on the CORES (sphere: its centre, capsule: its axis segment, the others themselves)
//                      with np_support of fsim_collide.hpp; while the cores are apart the answer is the core distance minus the radii;
//   cores intersecting the hand-off to np_mpr on the whole solids with a recording emitter.
//
// The iteration works on the Minkowski difference B - A in coordinates relative to A's centre (at a small gap the coordinates are then of
// the size of the shapes, not of the scene: the rounding of a support point is that much smaller).  The simplex is the four named
// registers s0 .. s3 with their weights; nothing is indexed dynamically, so nothing lives in scratch.  Per iteration: the support point w
// along -n; stop when dist - n . w <= GJK_ABS + GJK_REL * dist (n . w is the separation of the two cores along n: a lower bound of their
// distance, dist an upper bound); else w joins the simplex, the point of the simplex nearest the origin is found (segment, triangle, or the
// four faces of a tetrahedron: Ericson's region tests), the vertices with weight 0 leave.  The new direction does not
// come from normalising that nearest point, whose direction is lost to rounding when the gap is small: for a triangle it is the triangle's
// normal, for a segment the nearest point made orthogonal to the segment a second time.  A step that ends farther away (beyond rounding) ends the
// iteration with the previous answer.  An origin inside the tetrahedron, or nearer than GJK_TOUCH: the cores intersect.
#pragma once
#include "fsim_collide.hpp"

#define GJK_MAXIT 40
#define GJK_ABS 1e-6f
#define GJK_REL 1e-5f
#define GJK_TOUCH 1e-6f // cores nearer than this count as intersecting: the portal routine decides
enum { GJK_BR_PLANE = 0, GJK_BR_APART = 1, GJK_BR_PORTAL = 2, GJK_BR_CAP = 3 /* apart, iteration cap reached */, GJK_BR_NONE = 4 /* portal silent: the iteration's last answer */ };

struct PairOut { float d; V3 n, from, to; int iters, branch; };

struct GjkRec { // the emitter np_mpr writes its one contact to (np_mpr takes its emitter const: the record is mutable)
  mutable float dist = 0.0f;
  mutable V3 pos = {0.0f, 0.0f, 0.0f}, n = {1.0f, 0.0f, 0.0f};
  mutable int cnt = 0;
  DEV void operator()(int, float d_, V3 p_, V3 n_) const { dist = d_; pos = p_; n = n_; cnt++; }
};

// weights (u, v, w) of the point of the triangle a b c nearest the origin
DEV void gjk_tri(V3 a, V3 b, V3 c, float &u, float &v, float &w) {
  const V3 ab = b - a, ac = c - a;
  const float d1 = -dot(ab, a), d2 = -dot(ac, a);
  if (d1 <= 0.0f && d2 <= 0.0f) { u = 1.0f; v = 0.0f; w = 0.0f; return; }
  const float d3 = -dot(ab, b), d4 = -dot(ac, b);
  if (d3 >= 0.0f && d4 <= d3) { u = 0.0f; v = 1.0f; w = 0.0f; return; }
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { v = d1 / fmaxf(d1 - d3, 1e-38f); u = 1.0f - v; w = 0.0f; return; }
  const float d5 = -dot(ab, c), d6 = -dot(ac, c);
  if (d6 >= 0.0f && d5 <= d6) { u = 0.0f; v = 0.0f; w = 1.0f; return; }
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { w = d2 / fmaxf(d2 - d6, 1e-38f); u = 1.0f - w; v = 0.0f; return; }
  const float va = d3 * d6 - d5 * d4;
  if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) { w = (d4 - d3) / fmaxf((d4 - d3) + (d5 - d6), 1e-38f); v = 1.0f - w; u = 0.0f; return; }
  const float inv = 1.0f / fmaxf(va + vb + vc, 1e-38f);
  v = vb * inv; w = vc * inv; u = 1.0f - v - w;
}

DEV bool gjk_same(V3 a, V3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// The distance of the cores A, B (B given relative to A's centre, A at the origin) -> true: apart, with dist > 0, the unit direction n from
// A to B and the nearest points pa, pb; false: they intersect (or touch within GJK_TOUCH); dist, n, pa, pb then hold the last answer the
// iteration had.
template <bool MESH> DEV bool gjk_cores(const Shape &A, const Shape &B, float &dist, V3 &n, V3 &pa, V3 &pb, int &iters, bool &capped) {
  Sup s0, s1, s2, s3;
  s0.a = A.pos; s0.b = B.pos; s0.v = s0.b - s0.a; // (both centres lie inside their cores)
  s1 = s0; s2 = s0; s3 = s0;
  int m = 1;
  pa = s0.a; pb = s0.b;
  dist = norm(s0.v);
  n = v3(1.0f, 0.0f, 0.0f);
  iters = 0;
  capped = false;
  if (dist < GJK_TOUCH) return false;
  n = s0.v * (1.0f / dist);
  for (int it = 0; it < GJK_MAXIT; it++) {
    iters = it + 1;
    const Sup w = np_msup_t<MESH>(A, B, -n); // a: A's point farthest along n, b: B's farthest along -n
    if (dist - dot(n, w.v) <= GJK_ABS + GJK_REL * dist) return true;
    if (gjk_same(w.v, s0.v) || (m > 1 && gjk_same(w.v, s1.v)) || (m > 2 && gjk_same(w.v, s2.v))) return true; // (a polytope's vertex again: nothing nearer exists)
    float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f, l3 = 0.0f;
    if (m == 1) {
      s1 = w;
      const V3 e = s1.v - s0.v;
      l1 = fminf(fmaxf(-dot(s0.v, e) / fmaxf(dot(e, e), 1e-38f), 0.0f), 1.0f);
      l0 = 1.0f - l1;
    } else if (m == 2) {
      s2 = w;
      gjk_tri(s0.v, s1.v, s2.v, l0, l1, l2);
    } else {
      s3 = w;
      // The origin is inside when it is on the tetrahedron's side of all four faces -- of a tetrahedron with a volume to speak of: the
      // sides of a flat one are rounding.  Outside, the nearest point is the nearest of the four faces' nearest points; all four are
      // solved, whatever the side tests say (a wrong side test must not hide the face that holds the answer).
      const V3 e1 = s1.v - s0.v, e2 = s2.v - s0.v, e3 = s3.v - s0.v;
      bool inside = fabsf(dot(e3, cross(e1, e2))) > 1e-5f * sqrtf(dot(e1, e1) * dot(e2, e2) * dot(e3, e3));
      float best = 3.0e38f;
#pragma unroll 1
      for (int f = 0; f < 4; f++) { // faces (0 1 2 | 3), (0 1 3 | 2), (0 2 3 | 1), (1 2 3 | 0)
        const V3 a = f == 3 ? s1.v : s0.v, b = f >= 2 ? s2.v : s1.v, c = f == 0 ? s2.v : s3.v;
        const V3 d = f == 0 ? s3.v : (f == 1 ? s2.v : (f == 2 ? s1.v : s0.v));
        const V3 fn = cross(b - a, c - a);
        if (!(-dot(a, fn) * dot(d - a, fn) > 0.0f)) inside = false;
        float u, v, ww;
        gjk_tri(a, b, c, u, v, ww);
        // The squared distance of this face's nearest point.  Inside the face it is the plane's, not |a u + b v + c w|^2: on a sliver (a
        // curved rim seen from a parallel face makes them) the weights are ill-conditioned along the sliver and that point lies off the foot.
        const V3 p = a * u + b * v + c * ww;
        const float f2 = dot(fn, fn), fa = dot(fn, a);
        const float q = u > 0.0f && v > 0.0f && ww > 0.0f && f2 > 1e-30f ? fa * fa / f2 : dot(p, p);
        if (q < best) {
          best = q;
          l0 = f < 3 ? u : 0.0f;
          l1 = f < 2 ? v : (f == 3 ? u : 0.0f);
          l2 = f == 0 ? ww : (f == 1 ? 0.0f : v);
          l3 = f == 0 ? 0.0f : ww;
        }
      }
      if (inside) return false;
    }
    // the vertices with a weight stay: at most three
    Sup t0 = s0, t1 = s0, t2 = s0;
    float k0 = 0.0f, k1 = 0.0f, k2 = 0.0f;
    int mm = 0;
#define GJK_PUSH(S, L) if (L > 0.0f) { if (mm == 0) { t0 = S; k0 = L; } else if (mm == 1) { t1 = S; k1 = L; } else { t2 = S; k2 = L; } mm++; }
    GJK_PUSH(s0, l0) GJK_PUSH(s1, l1) GJK_PUSH(s2, l2) GJK_PUSH(s3, l3)
#undef GJK_PUSH
    if (mm == 0) return false; // (not a number somewhere: no answer from here)
    s0 = t0; s1 = t1; s2 = t2; m = mm;
    V3 v = s0.v * k0, nn;
    float nd;
    if (m == 1) {
      nd = norm(v);
      nn = v;
    } else if (m == 2) {
      v = v + s1.v * k1;
      const V3 e = s1.v - s0.v;
      const float ie = 1.0f / fmaxf(dot(e, e), 1e-38f);
      nn = v - e * (dot(e, v) * ie);
      nn = nn - e * (dot(e, nn) * ie);
      nd = norm(nn);
    } else {
      v = v + s1.v * k1 + s2.v * k2;
      const V3 e1 = s1.v - s0.v, e2 = s2.v - s0.v;
      nn = cross(e1, e2);
      const float q = dot(nn, nn);
      if (q > 1e-10f * dot(e1, e1) * dot(e2, e2)) {
        const float h = dot(nn, s0.v) / q; // the origin's foot on the triangle's plane is h * nn
        // the weights again, from the foot (Cramer's rule in the plane): on a sliver the region tests' weights can leave the point they
        // combine to far from the foot along the sliver, and the two witness points would not face each other
        const V3 r = nn * h - s0.v;
        k1 = fminf(fmaxf(dot(cross(r, e2), nn) / q, 0.0f), 1.0f);
        k2 = fminf(fmaxf(dot(cross(e1, r), nn) / q, 0.0f), 1.0f - k1);
        k0 = 1.0f - k1 - k2;
        nn = nn * h;
        nd = fabsf(h) * sqrtf(q);
      } else { // a sliver: no plane to speak of
        nn = v;
        nd = norm(v);
      }
    }
    if (nd < GJK_TOUCH) return false;
    // farther: the previous answer stands.  (Equal within rounding is not "farther": far apart, a turn of the direction that still
    // matters to the separation along it moves the distance by less than an ulp.)
    if (!(nd <= dist * (1.0f + 2e-6f))) return true;
    dist = nd;
    n = nn * (1.0f / nd);
    pa = s0.a * k0; pb = s0.b * k0;
    if (m > 1) { pa = pa + s1.a * k1; pb = pb + s1.b * k1; }
    if (m > 2) { pa = pa + s2.a * k2; pb = pb + s2.b * k2; }
  }
  capped = true;
  return true;
}

DEV V3 gjk_sel(bool c, V3 a, V3 b) { return v3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }
DEV Shape gjk_pick(bool c, const Shape &a, const Shape &b) { // c ? a : b
  Shape s;
  s.type = c ? a.type : b.type; s.pos = gjk_sel(c, a.pos, b.pos); s.size = gjk_sel(c, a.size, b.size);
#pragma unroll
  for (int i = 0; i < 9; i++) s.R.m[i] = c ? a.R.m[i] : b.R.m[i];
  s.verts = c ? a.verts : b.verts; s.nvert = c ? a.nvert : b.nvert;
  return s;
}

// include/fsim_pairs.h, "Contract per pair".  Not both planes (the caller's pair list holds no such pair).
template <bool MESH> DEV PairOut gjk_pair(const Shape &A0, const Shape &B0) {
  PairOut o;
  o.iters = 0;
  if (A0.type == GT_PLANE || B0.type == GT_PLANE) {
    const bool pa_ = A0.type == GT_PLANE;
    const Shape X = gjk_pick(pa_, B0, A0); // (picked member by member: a reference picked at run time would put both shapes in scratch)
    const V3 np = gjk_sel(pa_, colv(A0.R, 2), colv(B0.R, 2)), pp = gjk_sel(pa_, A0.pos, B0.pos);
    const V3 low = np_support<MESH>(X, -np);
    o.d = dot(np, low - pp);
    o.n = gjk_sel(pa_, np, -np);
    const V3 foot = low - np * o.d;
    o.from = gjk_sel(pa_, foot, low);
    o.to = gjk_sel(pa_, low, foot);
    o.branch = GJK_BR_PLANE;
    return o;
  }
  // relative to A's centre; the cores: no radius
  Shape A = A0, B = B0;
  A.pos = v3(0.0f, 0.0f, 0.0f);
  B.pos = B0.pos - A0.pos;
  const bool ra_ = A.type == GT_SPHERE || A.type == GT_CAPSULE, rb_ = B.type == GT_SPHERE || B.type == GT_CAPSULE;
  const float ra = ra_ ? A.size.x : 0.0f, rb = rb_ ? B.size.x : 0.0f;
  Shape Ac = A, Bc = B;
  if (ra_) Ac.size.x = 0.0f;
  if (rb_) Bc.size.x = 0.0f;
  float dist;
  V3 n, pa, pb;
  bool capped;
  const bool apart = gjk_cores<MESH>(Ac, Bc, dist, n, pa, pb, o.iters, capped);
  o.branch = apart ? (capped ? GJK_BR_CAP : GJK_BR_APART) : GJK_BR_NONE;
  if (!apart) {
    GjkRec e;
    np_mpr<GjkRec, MESH>(e, A, B);
    const float md = e.dist;
    const V3 mp = e.pos;
    V3 mn = e.n;
    if (e.cnt > 0 && isfinite(md) && isfinite(mp.x + mp.y + mp.z) && dot(mn, mn) > 1e-12f) {
      mn = normalized(mn);
      o.d = md;
      o.n = mn;
      o.from = A0.pos + mp - mn * (0.5f * md);
      o.to = A0.pos + mp + mn * (0.5f * md);
      o.branch = GJK_BR_PORTAL;
      return o;
    }
  }
  o.d = dist - ra - rb;
  o.n = n;
  o.from = A0.pos + pa + n * ra;
  o.to = A0.pos + pb - n * rb;
  return o;
}
