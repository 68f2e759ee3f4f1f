// Perspective view of a resident plane: a hidden-surface render of the height field (dbm_grid_perspective, dbm_grid_minmax, and the host
// entry dbm_grid_perspective_host, here; the frame, the view and the product `plot_3d_view` are deepbedmap_amd/perspective.py).
// Reference: deepbedmap.py:258-295, `plot_3d_view`: fig.grdview(..., surftype="sim", plane=zmin, zscale=0.01, perspective=[202.5, 60]).
// The rule below is this project's own -- GMT's pixels are not claimed -- and is stated once more, with the reasons, in DESIGN.md 6o.
//
// Scene (index units).  Node (r, c) of the float32 plane (H, W) sits at east = c, north = -r, height h = ((double)z - level) * zfac.  A
// cell of four finite nodes a = (r, c), b = (r, c + 1), d = (r + 1, c), e = (r + 1, c + 1) is two triangles: 0 = (a, b, d) where
// fx + fy <= 1, 1 = (e, d, b) elsewhere; height and colour are linear on each from its own vertices.  Another cell is a hole.  Facade: a
// vertical two-sided wall between height 0 and the boundary profile on the four outer edges, where both nodes of a segment are finite.
// View (orthographic).  A pixel (i, j) has sx = sx0 + (j + 0.5) step, sy = sy0 - (i + 0.5) step; its ray is the points G + q (sin A,
// cos A) at height q tan E, G = sx (-cos A, sin A) + (sy / sin E) (-sin A, -cos A), the viewer at q -> +inf.  In grid coordinates
// (x = east, y = -north): x(q) = ox + q dx, y(q) = oy + q dy with dx = sin A, dy = -cos A (persp_ray).
// Pixel.  Every operation is ONE IEEE float64 operation, never an FMA (persp_cell, persp_wall, persp_colour: the ONE text of the rule,
// run by the kernel, by the host entry and restated in NumPy by tests/perspective_restatement.py):
//   slab     per axis with a non-zero direction q1 = (c - ox) / dx, q2 = ((c + 1) - ox) / dx, [min, max]; a zero direction needs
//            c <= ox <= c + 1; q_lo = the larger minimum, q_hi = the smaller maximum; the cell is met if q_lo <= q_hi.
//   triangle 0: al0 = ox - c, be0 = oy - r, s1 = hb - ha, s2 = hd - ha, num = (ha + s1 al0) + s2 be0, den = (tan E - s1 dx) - s2 dy,
//            q = num / den; counts if den != 0, q_lo <= q <= q_hi and side(q) <= 1; al = al0 + q dx, be = be0 + q dy.
//            1: al0 = (c + 1) - ox, be0 = (r + 1) - oy, s1 = hd - he, s2 = hb - he, num = (he + s1 al0) + s2 be0, den = (tan E + s1 dx)
//            + s2 dy, q = num / den; counts if den != 0, q_lo <= q <= q_hi and side(q) > 1; al = al0 - q dx, be = be0 - q dy.
//   side     fx + fy as ONE monotone function of q for both triangles: side(q) = ((ox + oy) - (c + r)) + q (dx + dy).  A ray that runs
//            along the cells' diagonals (A = 45 degrees) has a side that does not move with q, so every cell gives it to the same
//            triangle and the surface has no crack there; two sums rounded apart, one per triangle, would refuse both.
//   wall     along row rw (0 or H - 1), dy != 0: q = (rw - oy) / dy, x = ox + q dx, hr = q tan E; for a segment c with c <= x <= c + 1
//            and finite nodes, p = ha + (hb - ha) (x - c); counts if min(0, p) <= hr <= max(0, p).  Along a column alike with x and y
//            exchanged.
//   visible  the largest q that counts; among equal q the smallest id: a wall is -2, triangle t of cell (r, c) is 2 (r (W - 1) + c) + t;
//            no hit: -1.
//   colour   u = (c0 + (c1 - c0) al) + (c2 - c0) be per channel on the drape's bytes at the triangle's vertices in the order above;
//            byte = floor(u + 0.5) clamped to 0 .. 255, alpha 255.  A wall takes `facade`, a miss `background` (four bytes each).
// The image is a function of this definition and never of the order or the skipping of the traversal: a traversal may leave out a cell
// only where it has shown that no q of that cell can be the visible one.
//
// Device traversal.  One thread per pixel, workgroups of 16 x 16 pixels: neighbouring rays are parallel and one `step` apart, so a
// workgroup's gathers fall on a few neighbouring cells of a plane that stays in L2.  A prepass (persp_blocks_kernel, persp_range_kernel)
// reduces z to the maxima of blocks of 8 x 8 and of 64 x 64 cells (their 9 x 9 and 65 x 65 nodes; -inf: no finite node) and to the
// plane's range.  The ray is clipped to the footprint and to the heights [min(0, hmin) - M, max(0, hmax) + M].  It walks strips of 64,
// then 8, then 1 cells along the axis it moves faster on, from the viewer's side (one loop with a level, persp_walk): a strip's interval [s_lo, s_hi] comes from its two
// grid lines by the slab formula, so by the monotonicity of IEEE subtraction and division it contains the interval of every cell in
// the strip, bit for bit.  Across the strip the ray covers rows floor(v_min - eps) .. floor(v_max + eps).  A strip is skipped when
// every block the ray covers in it has h(max) + M < max(s_lo, Q_lo) tan E, the ray's lowest height there; the walk stops once a hit is
// held with q > s_hi: every remaining cell has q_hi <= s_hi, strictly below it.  M = 2^-30 (1 + max |h| + tan E) (2 + W + H + |ox| +
// |oy|) bounds what rounding can add to the height of a q that counts over the heights of its triangle (the residual num - q den
// carries a few units of 2^-53 of those magnitudes: DESIGN.md 6o); eps = 2^-40 (2 + W + H + |ox| + |oy|).
// The host entry walks plainly: every column strip of one cell along the faster axis, the rows floor(v_min) - 1 .. floor(v_max) + 1 of
// each, no clipping, no blocks, no stop.
#include "api_common.h"
#include "data_prims.h"
#include <cstring>
#include <thread>

namespace {

constexpr int PERSP_TILE = 16;                 // pixels of a workgroup, each way
constexpr int PERSP_PRE_THREADS = 64;          // prepass: one thread per 8 x 8 block of a 64 x 64 block
constexpr int PERSP_FOLD_THREADS = 256;
constexpr int MINMAX_THREADS = 256, MINMAX_MAX_GROUPS = 1024;

#define PERSP_INF __builtin_huge_val()

struct PerspRay {
  double ox, oy, dx, dy;   // x(q) = ox + q dx (east, columns), y(q) = oy + q dy (rows)
  double oxy, dxy;         // ox + oy, dx + dy: the side of a cell's diagonal
};

struct PerspBest {
  double q;
  int id;
  double al, be;
};

__host__ __device__ inline PerspRay persp_ray(const PerspView& v, long i, long j) {
#pragma clang fp contract(off)
  const double sx = v.sx0 + ((double)j + 0.5) * v.step;
  const double sy = v.sy0 - ((double)i + 0.5) * v.step;
  const double t = sy / v.sin_e;
  const double a = sx * v.cos_a, b = t * v.sin_a;
  const double c = sx * v.sin_a, d = t * v.cos_a;
  PerspRay ray;
  ray.ox = (-a) - b;        // east of G
  ray.oy = -(c - d);        // minus north of G
  ray.dx = v.sin_a;
  ray.dy = -v.cos_a;
  ray.oxy = ray.ox + ray.oy;
  ray.dxy = ray.dx + ray.dy;
  return ray;
}

__host__ __device__ inline bool persp_finite(float z) { return z - z == 0.0f; }

__host__ __device__ inline double persp_height(const PerspView& v, float z) {
#pragma clang fp contract(off)
  return ((double)z - v.level) * v.zfac;
}

__host__ __device__ inline void persp_take(PerspBest& best, double q, int id, double al, double be) {
  if (q > best.q || (q == best.q && id < best.id)) {
    best.q = q; best.id = id; best.al = al; best.be = be;
  }
}

// one axis of the slab: narrows [lo, hi] to the q with k0 <= o + q d <= k1; false if the axis alone shows the strip is missed
__host__ __device__ inline bool persp_slab(double o, double d, double k0, double k1, double& lo, double& hi) {
#pragma clang fp contract(off)
  if (d != 0.0) {
    const double q1 = (k0 - o) / d, q2 = (k1 - o) / d;
    const double mn = q1 < q2 ? q1 : q2, mx = q1 < q2 ? q2 : q1;
    lo = mn > lo ? mn : lo;
    hi = mx < hi ? mx : hi;
    return true;
  }
  return k0 <= o && o <= k1;
}

// The cell (r, c), 0 <= r < H - 1, 0 <= c < W - 1: its two triangles against the ray.
__host__ __device__ inline void persp_cell(const float* plane, long W, long r, long c, const PerspView& v, const PerspRay& ray, PerspBest& best) {
#pragma clang fp contract(off)
  const float za = plane[r * W + c], zb = plane[r * W + c + 1], zd = plane[(r + 1) * W + c], ze = plane[(r + 1) * W + c + 1];
  if (!(persp_finite(za) && persp_finite(zb) && persp_finite(zd) && persp_finite(ze))) return;   // a hole
  const double x0 = (double)c, x1 = (double)(c + 1), y0 = (double)r, y1 = (double)(r + 1);
  double lo = -PERSP_INF, hi = PERSP_INF;
  if (!persp_slab(ray.ox, ray.dx, x0, x1, lo, hi)) return;
  if (!persp_slab(ray.oy, ray.dy, y0, y1, lo, hi)) return;
  if (!(lo <= hi)) return;
  const double ha = persp_height(v, za), hb = persp_height(v, zb), hd = persp_height(v, zd), he = persp_height(v, ze);
  const int id = 2 * (int)(r * (W - 1) + c);
  const double side0 = ray.oxy - (double)(c + r);
  {
    const double al0 = ray.ox - x0, be0 = ray.oy - y0;
    const double s1 = hb - ha, s2 = hd - ha;
    const double p1 = s1 * al0, p2 = s2 * be0;
    const double num = (ha + p1) + p2;
    const double d1 = s1 * ray.dx, d2 = s2 * ray.dy;
    const double den = (v.tan_e - d1) - d2;
    if (den != 0.0) {
      const double q = num / den;
      if (lo <= q && q <= hi) {
        const double qa = q * ray.dx, qb = q * ray.dy, qs = q * ray.dxy;
        if (side0 + qs <= 1.0) persp_take(best, q, id, al0 + qa, be0 + qb);
      }
    }
  }
  {
    const double al0 = x1 - ray.ox, be0 = y1 - ray.oy;
    const double s1 = hd - he, s2 = hb - he;
    const double p1 = s1 * al0, p2 = s2 * be0;
    const double num = (he + p1) + p2;
    const double d1 = s1 * ray.dx, d2 = s2 * ray.dy;
    const double den = (v.tan_e + d1) + d2;
    if (den != 0.0) {
      const double q = num / den;
      if (lo <= q && q <= hi) {
        const double qa = q * ray.dx, qb = q * ray.dy, qs = q * ray.dxy;
        if (side0 + qs > 1.0) persp_take(best, q, id + 1, al0 - qa, be0 - qb);
      }
    }
  }
}

// One wall: the nodes base[k * stride], k = 0 .. n - 1, along the axis `u` at the coordinate w of the other axis `v`.
__host__ __device__ inline void persp_wall(const float* base, long stride, long n, double w, double ou, double du, double ov, double dv,
                                           const PerspView& view, PerspBest& best) {
#pragma clang fp contract(off)
  if (dv == 0.0) return;
  const double q = (w - ov) / dv;
  const double qd = q * du;
  const double u = ou + qd;
  const double hr = q * view.tan_e;
  if (!(u >= 0.0 && u <= (double)(n - 1))) return;
  const long k0 = (long)floor(u);
  for (long k = k0 - 1; k <= k0; ++k) {   // the segments that hold u: two at a node
    if (k < 0 || k > n - 2) continue;
    if (!((double)k <= u && u <= (double)(k + 1))) continue;
    const float za = base[k * stride], zb = base[(k + 1) * stride];
    if (!(persp_finite(za) && persp_finite(zb))) continue;
    const double ha = persp_height(view, za), hb = persp_height(view, zb);
    const double t = u - (double)k;
    const double rise = (hb - ha) * t;
    const double p = ha + rise;
    const double mn = p < 0.0 ? p : 0.0, mx = p < 0.0 ? 0.0 : p;
    if (mn <= hr && hr <= mx) persp_take(best, q, -2, 0.0, 0.0);
  }
}

__host__ __device__ inline void persp_walls(const float* plane, long H, long W, const PerspView& v, const PerspRay& ray, PerspBest& best) {
  persp_wall(plane, 1, W, 0.0, ray.ox, ray.dx, ray.oy, ray.dy, v, best);                                // north edge: row 0
  persp_wall(plane + (H - 1) * W, 1, W, (double)(H - 1), ray.ox, ray.dx, ray.oy, ray.dy, v, best);      // south edge
  persp_wall(plane, W, H, 0.0, ray.oy, ray.dy, ray.ox, ray.dx, v, best);                                // west edge: column 0
  persp_wall(plane + (W - 1), W, H, (double)(W - 1), ray.oy, ray.dy, ray.ox, ray.dx, v, best);          // east edge
}

// the pixel of the visible hit, little endian r, g, b, a
__host__ __device__ inline uint32_t persp_rgba(const uint8_t (&c)[4]) {
  return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
}

__host__ __device__ inline uint32_t persp_colour(const uint8_t* drape, int channels, long W, const PerspBest& best, uint32_t facade,
                                                 uint32_t background) {
#pragma clang fp contract(off)
  if (best.id == -1) return background;
  if (best.id == -2) return facade;
  const long cell = best.id >> 1, r = cell / (W - 1), c = cell % (W - 1);
  const bool upper = (best.id & 1) == 0;
  const long n0 = upper ? r * W + c : (r + 1) * W + c + 1;
  const long n1 = upper ? r * W + c + 1 : (r + 1) * W + c;
  const long n2 = upper ? (r + 1) * W + c : r * W + c + 1;
  uint32_t p = 0xFF000000u;
  for (int ch = 0; ch < 3; ++ch) {
    const double c0 = (double)drape[n0 * channels + ch], c1 = (double)drape[n1 * channels + ch], c2 = (double)drape[n2 * channels + ch];
    const double t1 = (c1 - c0) * best.al, t2 = (c2 - c0) * best.be;
    const double u = (c0 + t1) + t2;
    const double w = floor(u + 0.5);
    p |= (uint32_t)(w < 0.0 ? 0.0 : (w > 255.0 ? 255.0 : w)) << (8 * ch);
  }
  return p;
}

// ---- the prepass: block maxima at two levels and the plane's range ----
struct PerspRange {
  float mn, mx;   // over the finite samples: +inf, -inf if there is none
};
__device__ __forceinline__ PerspRange persp_range_merge(const PerspRange& a, const PerspRange& b) {
  return PerspRange{a.mn < b.mn ? a.mn : b.mn, a.mx > b.mx ? a.mx : b.mx};
}

// workgroup B = block (B / n64x, B % n64x) of 64 x 64 cells; thread t its 8 x 8 block (t / 8, t % 8)
__global__ __launch_bounds__(PERSP_PRE_THREADS) void persp_blocks_kernel(PerspLaunch a) {
  const long BY = blockIdx.x / a.n64x, BX = blockIdx.x % a.n64x;
  const long Y8 = BY * 8 + threadIdx.x / 8, X8 = BX * 8 + threadIdx.x % 8;
  PerspRange v{__builtin_huge_valf(), -__builtin_huge_valf()};
  if (Y8 < a.n8y && X8 < a.n8x) {
    const long r1 = Y8 * 8 + 8 < a.H - 1 ? Y8 * 8 + 8 : a.H - 1, c1 = X8 * 8 + 8 < a.W - 1 ? X8 * 8 + 8 : a.W - 1;   // nodes, inclusive
    for (long r = Y8 * 8; r <= r1; ++r)
      for (long c = X8 * 8; c <= c1; ++c) {
        const float z = a.plane[r * a.W + c];
        if (persp_finite(z)) v = persp_range_merge(v, PerspRange{z, z});
      }
    a.max8[Y8 * a.n8x + X8] = v.mx;
  }
  v = block_reduce<PERSP_PRE_THREADS>(v, persp_range_merge);
  if (threadIdx.x == 0) {
    a.max64[blockIdx.x] = v.mx;
    a.part[2 * (long)blockIdx.x] = v.mn;
    a.part[2 * (long)blockIdx.x + 1] = v.mx;
  }
}

__global__ __launch_bounds__(PERSP_FOLD_THREADS) void persp_range_kernel(PerspLaunch a) {
  const PerspRange v = fold_partials<PERSP_FOLD_THREADS>(a.n64x * a.n64y, PerspRange{__builtin_huge_valf(), -__builtin_huge_valf()},
                                                         [&](long k) { return PerspRange{a.part[2 * k], a.part[2 * k + 1]}; }, persp_range_merge);
  if (threadIdx.x == 0) {
    a.zrange[0] = v.mn;
    a.zrange[1] = v.mx;
  }
}

// ---- the traversal of one ray on the device (host and device text: perspective_render_host can run it on host threads, so that the
// skipping is checked against the plain walk, and its indexing under a sanitizer, without a GPU) ----
struct PerspWalk {
  const PerspLaunch& a;
  const PerspRay& ray;
  bool xmajor;
  double ou, du, ov, dv;   // the axis the ray moves faster on (u) and the other (v)
  long NU, NV;             // cells along each
  double Qlo, Qhi, M, eps;
};

// the strip of cells [u0, u1) along u: false if the walk is over; else `skip` says whether nothing in it can count.  On the way out
// qs = the lowest q of the strip inside the clip, [n_lo, n_hi] the blocks of `size` cells the ray covers across it.
__host__ __device__ inline bool persp_strip(const PerspWalk& w, const PerspBest& best, long u0, long u1, long size, long blocks, bool& skip,
                                            double& qs, long& n_lo, long& n_hi) {
#pragma clang fp contract(off)
  double s_lo = -PERSP_INF, s_hi = PERSP_INF;
  persp_slab(w.ou, w.du, (double)u0, (double)u1, s_lo, s_hi);   // (du is not zero)
  if (best.id != -1 && best.q > s_hi) return false;             // every remaining q_hi lies strictly below the hit that is held
  skip = true;
  qs = s_lo > w.Qlo ? s_lo : w.Qlo;
  const double qe = s_hi < w.Qhi ? s_hi : w.Qhi;
  if (!(qs <= qe)) return true;
  const double va = w.ov + qs * w.dv, vb = w.ov + qe * w.dv;
  const double v_min = (va < vb ? va : vb) - w.eps, v_max = (va < vb ? vb : va) + w.eps;
  const double top = (double)(blocks * size);
  if (!(v_max >= 0.0 && v_min < top)) return true;
  n_lo = v_min <= 0.0 ? 0 : (long)floor(v_min / (double)size);
  n_hi = v_max >= top ? blocks - 1 : (long)floor(v_max / (double)size);
  if (n_hi > blocks - 1) n_hi = blocks - 1;
  skip = n_lo > n_hi;
  return true;
}

// true if some block of `maxima` (row length nx in the plane's own orientation) in strip position m, rows n_lo .. n_hi, may hold a q
// that counts at a ray height of `floor_h` or more
__host__ __device__ inline bool persp_blocks_reach(const PerspWalk& w, const float* maxima, long nx, long m, long n_lo, long n_hi, double floor_h) {
#pragma clang fp contract(off)
  for (long n = n_lo; n <= n_hi; ++n) {
    const float mx = maxima[w.xmajor ? n * nx + m : m * nx + n];
    if (!(mx > -__builtin_huge_valf())) continue;
    if (!(persp_height(w.a.v, mx) + w.M < floor_h)) return true;
  }
  return false;
}

__host__ __device__ inline void persp_walk(const PerspLaunch& a, const PerspRay& ray, PerspBest& best) {
#pragma clang fp contract(off)
  const PerspView& v = a.v;
  const float zmin = a.zrange[0], zmax = a.zrange[1];
  if (!(zmin <= zmax)) return;   // no finite node
  const double h_lo = persp_height(v, zmin), h_hi = persp_height(v, zmax);
  const double size = 2.0 + (double)a.W + (double)a.H + fabs(ray.ox) + fabs(ray.oy);
  const double habs = fabs(h_lo) > fabs(h_hi) ? fabs(h_lo) : fabs(h_hi);
  PerspWalk w{a, ray};
  w.M = 9.3132257461547852e-10 * (1.0 + habs + v.tan_e) * size;   // 2^-30
  w.eps = 9.0949470177292824e-13 * size;                          // 2^-40
  double f_lo = -PERSP_INF, f_hi = PERSP_INF;                     // the footprint
  if (!persp_slab(ray.ox, ray.dx, 0.0, (double)(a.W - 1), f_lo, f_hi)) return;
  if (!persp_slab(ray.oy, ray.dy, 0.0, (double)(a.H - 1), f_lo, f_hi)) return;
  const double q_top = ((h_hi > 0.0 ? h_hi : 0.0) + w.M) / v.tan_e, q_bottom = ((h_lo < 0.0 ? h_lo : 0.0) - w.M) / v.tan_e;
  w.Qlo = f_lo > q_bottom ? f_lo : q_bottom;
  w.Qhi = f_hi < q_top ? f_hi : q_top;
  if (!(w.Qlo <= w.Qhi)) return;
  w.xmajor = fabs(ray.dx) >= fabs(ray.dy);
  w.ou = w.xmajor ? ray.ox : ray.oy; w.du = w.xmajor ? ray.dx : ray.dy;
  w.ov = w.xmajor ? ray.oy : ray.ox; w.dv = w.xmajor ? ray.dy : ray.dx;
  w.NU = (w.xmajor ? a.W : a.H) - 1; w.NV = (w.xmajor ? a.H : a.W) - 1;
  // the cells along u that the clipped ray covers
  const double ua = w.ou + w.Qlo * w.du, ub = w.ou + w.Qhi * w.du;
  const double u_min = (ua < ub ? ua : ub) - w.eps, u_max = (ua < ub ? ub : ua) + w.eps;
  if (!(u_max >= 0.0 && u_min < (double)w.NU)) return;
  const long m_lo = u_min <= 0.0 ? 0 : (long)floor(u_min);
  long m_hi = u_max >= (double)w.NU ? w.NU - 1 : (long)floor(u_max);
  if (m_hi > w.NU - 1) m_hi = w.NU - 1;
  if (m_lo > m_hi) return;
  const long dir = w.du > 0.0 ? -1 : 1;   // q falls along the walk
  const long first = dir < 0 ? m_hi : m_lo, last = dir < 0 ? m_lo : m_hi;
  // ONE loop over the three levels (2: strips of 64 cells, 1: of 8, 0: of 1): at cell m the strip of the current level that holds m is
  // tested; one that may hold the visible hit is entered a level down, at level 0 its cells are run; then m moves past the strip and
  // the level rises again wherever m enters a new coarser strip.
  long m = first;
  int level = 2;
  while (dir * (m - last) <= 0) {
    const long size = level == 2 ? 64 : (level == 1 ? 8 : 1);
    const long a0 = (m / size) * size, b0 = a0 + size < w.NU ? a0 + size : w.NU;
    const long blocks = level == 2 ? (w.xmajor ? a.n64y : a.n64x) : (level == 1 ? (w.xmajor ? a.n8y : a.n8x) : w.NV);
    bool skip;
    double qs;
    long n_lo, n_hi;
    if (!persp_strip(w, best, a0, b0, size, blocks, skip, qs, n_lo, n_hi)) return;
    if (!skip && level > 0)
      skip = !persp_blocks_reach(w, level == 2 ? a.max64 : a.max8, level == 2 ? a.n64x : a.n8x, a0 / size, n_lo, n_hi, qs * v.tan_e);
    if (!skip && level > 0) {
      --level;   // the same m, a finer strip
      continue;
    }
    if (!skip)
      for (long n = n_lo; n <= n_hi; ++n) persp_cell(a.plane, a.W, w.xmajor ? n : m, w.xmajor ? m : n, v, ray, best);
    m = dir > 0 ? b0 : a0 - 1;
    const long edge = dir > 0 ? m : m + 1;   // the grid line that was crossed
    if (level == 0 && edge % 8 == 0) level = 1;
    if (level == 1 && edge % 64 == 0) level = 2;
  }
}

__global__ __launch_bounds__(PERSP_TILE* PERSP_TILE) void grid_perspective_kernel(PerspLaunch a) {
  const long tiles_x = (a.Wo + PERSP_TILE - 1) / PERSP_TILE;
  const long j = (blockIdx.x % tiles_x) * PERSP_TILE + threadIdx.x, i = (blockIdx.x / tiles_x) * PERSP_TILE + threadIdx.y;
  if (i >= a.Ho || j >= a.Wo) return;
  PerspBest best{-PERSP_INF, -1, 0.0, 0.0};
  if (a.H >= 2 && a.W >= 2) {
    const PerspRay ray = persp_ray(a.v, i, j);
    if (a.facade_on) persp_walls(a.plane, a.H, a.W, a.v, ray, best);
    persp_walk(a, ray, best);
  }
  const long at = i * a.Wo + j;   // below 2^31
  ((uint32_t*)a.out)[at] = persp_colour(a.drape, a.channels, a.W, best, persp_rgba(a.facade), persp_rgba(a.background));
  if (a.hits) a.hits[at] = best.id;
}

// ---- dbm_grid_minmax ----
struct MinMax {
  long long n;
  float mn, mx;
};
__device__ __forceinline__ MinMax minmax_merge(const MinMax& a, const MinMax& b) {
  return MinMax{a.n + b.n, a.mn < b.mn ? a.mn : b.mn, a.mx > b.mx ? a.mx : b.mx};
}
__device__ __forceinline__ MinMax minmax_none() { return MinMax{0, __builtin_huge_valf(), -__builtin_huge_valf()}; }

__global__ __launch_bounds__(MINMAX_THREADS) void minmax_partials_kernel(const float* plane, long n, MinMax* part) {
  MinMax v = minmax_none();
  for (long p = (long)blockIdx.x * MINMAX_THREADS + threadIdx.x; p < n; p += (long)gridDim.x * MINMAX_THREADS) {
    const float z = plane[p];
    if (persp_finite(z)) v = minmax_merge(v, MinMax{1, z, z});
  }
  v = block_reduce<MINMAX_THREADS>(v, minmax_merge);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ __launch_bounds__(MINMAX_THREADS) void minmax_fold_kernel(const MinMax* part, int groups, double* out) {
  const MinMax v = fold_partials<MINMAX_THREADS>((long)groups, minmax_none(), [&](long k) { return part[k]; }, minmax_merge);
  if (threadIdx.x != 0) return;
  out[0] = (double)v.n;
  out[1] = v.n > 0 ? (double)v.mn : __builtin_nan("");
  out[2] = v.n > 0 ? (double)v.mx : __builtin_nan("");
}

struct MinMaxLayout {
  double* out;
  MinMax* part;
  int groups;
  MinMaxLayout(Carver& carve, long H, long W) {
    groups = grid_stride_blocks(H * W, MINMAX_THREADS, MINMAX_MAX_GROUPS);
    out = carve.take<double>(3);
    part = carve.take<MinMax>((size_t)groups);
  }
};

// the workspace of launch_grid_perspective: the two levels of maxima, the 64-blocks' ranges, the plane's range
struct PerspLayout {
  float *max8, *max64, *part, *zrange;
  PerspLayout(Carver& carve, const PerspLaunch& a) {
    max8 = carve.take<float>((size_t)(a.n8x * a.n8y));
    max64 = carve.take<float>((size_t)(a.n64x * a.n64y));
    part = carve.take<float>(2 * (size_t)(a.n64x * a.n64y));
    zrange = carve.take<float>(2);
  }
};

void persp_block_counts(PerspLaunch& a) {
  a.n8x = a.W >= 2 ? (a.W - 1 + 7) / 8 : 0;
  a.n8y = a.H >= 2 ? (a.H - 1 + 7) / 8 : 0;
  a.n64x = (a.n8x + 7) / 8;
  a.n64y = (a.n8y + 7) / 8;
}

}  // namespace

size_t grid_minmax_workspace(long H, long W) {
  Carver measure(nullptr);
  MinMaxLayout layout(measure, H, W);
  return measure.bytes();
}

void launch_grid_minmax(const float* plane, long H, long W, void* ws, hipStream_t s) {
  Carver carve(ws);
  const MinMaxLayout layout(carve, H, W);
  hipLaunchKernelGGL(minmax_partials_kernel, dim3((unsigned)layout.groups), dim3(MINMAX_THREADS), 0, s, plane, H * W, layout.part);
  hipLaunchKernelGGL(minmax_fold_kernel, dim3(1), dim3(MINMAX_THREADS), 0, s, layout.part, layout.groups, layout.out);
  DBM_HIP(hipGetLastError());
}

size_t grid_perspective_workspace(const PerspLaunch& launch) {
  PerspLaunch a = launch;
  persp_block_counts(a);
  if (a.n8x == 0 || a.n8y == 0) return 0;
  Carver measure(nullptr);
  PerspLayout layout(measure, a);
  return measure.bytes();
}

void launch_grid_perspective(const PerspLaunch& launch, void* ws, hipStream_t s) {
  PerspLaunch a = launch;
  persp_block_counts(a);
  if (a.n8x > 0 && a.n8y > 0) {
    Carver carve(ws);
    const PerspLayout layout(carve, a);
    a.max8 = layout.max8; a.max64 = layout.max64; a.part = layout.part; a.zrange = layout.zrange;
    hipLaunchKernelGGL(persp_blocks_kernel, dim3((unsigned)(a.n64x * a.n64y)), dim3(PERSP_PRE_THREADS), 0, s, a);
    hipLaunchKernelGGL(persp_range_kernel, dim3(1), dim3(PERSP_FOLD_THREADS), 0, s, a);
  }
  const long tiles = ((a.Wo + PERSP_TILE - 1) / PERSP_TILE) * ((a.Ho + PERSP_TILE - 1) / PERSP_TILE);   // below 2^31 / 256 + ...
  hipLaunchKernelGGL(grid_perspective_kernel, dim3((unsigned)tiles), dim3(PERSP_TILE, PERSP_TILE), 0, s, a);
  DBM_HIP(hipGetLastError());
}

// what dbm_grid_perspective and dbm_grid_perspective_host refuse alike (status 1); fills the view
void perspective_check_arguments(const char* who, const void* plane, long H, long W, const void* drape, int drape_channels, const double* view,
                                 long Wo, long Ho, const void* background, const void* out, PerspView& v) {
  const std::string w(who);
  DBM_CHECK(plane != nullptr && drape != nullptr && out != nullptr, w + ": NULL plane, drape or output");
  DBM_CHECK(view != nullptr && background != nullptr, w + ": NULL view or background");
  DBM_CHECK(drape_channels == 3 || drape_channels == 4, w + ": drape_channels must be 3 (RGB) or 4 (RGBA)");
  DBM_CHECK(H >= 1 && W >= 1, w + ": empty plane");
  DBM_CHECK(H < (1L << 31) && W < (1L << 31) && H * W < (1L << 31), w + ": H W must stay below 2^31 samples");
  DBM_CHECK(2 * (H - 1) * (W - 1) < (1L << 31), w + ": the ids 2 (r (W - 1) + c) + t of the triangles must stay below 2^31");
  DBM_CHECK(Wo >= 1 && Ho >= 1, w + ": empty image");
  DBM_CHECK(Wo < (1L << 31) && Ho < (1L << 31) && Wo * Ho < (1L << 31), w + ": Wo Ho must stay below 2^31 pixels");
  for (int k = 0; k < 9; ++k) DBM_CHECK(std::isfinite(view[k]), w + ": the view's values must be finite (value " + std::to_string(k) + ")");
  v.sin_a = view[0]; v.cos_a = view[1]; v.sin_e = view[2]; v.tan_e = view[3]; v.level = view[4]; v.zfac = view[5];
  v.sx0 = view[6]; v.sy0 = view[7]; v.step = view[8];
  DBM_CHECK(std::fabs(v.sin_a * v.sin_a + v.cos_a * v.cos_a - 1.0) <= 1e-6, w + ": sin A and cos A must be those of one angle");
  DBM_CHECK(v.sin_e > 0.0 && v.tan_e > 0.0, w + ": sin E and tan E must be positive");
  DBM_CHECK(v.zfac > 0.0, w + ": zfac must be positive");
  DBM_CHECK(v.step > 0.0, w + ": step must be positive");
}

// The host render: a's pointers are HOST pointers.  skipping = false: the plain walk (dbm_grid_perspective_host).  skipping = true: the
// device's own traversal over block maxima made here by a plain loop (tools/perspective_twin_check.cpp).
void perspective_render_host(const PerspLaunch& launch, bool skipping, int nthreads) {
  PerspLaunch a = launch;
  const long H = a.H, W = a.W;
  persp_block_counts(a);
  std::vector<float> max8, max64, zrange(2);
  if (skipping && H >= 2 && W >= 2) {
    max8.assign((size_t)(a.n8x * a.n8y), -__builtin_huge_valf());
    max64.assign((size_t)(a.n64x * a.n64y), -__builtin_huge_valf());
    zrange[0] = __builtin_huge_valf(); zrange[1] = -__builtin_huge_valf();
    for (long r = 0; r < H; ++r)
      for (long c = 0; c < W; ++c) {
        const float z = a.plane[r * W + c];
        if (!persp_finite(z)) continue;
        zrange[0] = z < zrange[0] ? z : zrange[0];
        zrange[1] = z > zrange[1] ? z : zrange[1];
        // node (r, c) belongs to the blocks of the cells (r - 1 .. r, c - 1 .. c)
        for (long cr = r > 0 ? r - 1 : 0; cr <= r && cr < H - 1; ++cr)
          for (long cc = c > 0 ? c - 1 : 0; cc <= c && cc < W - 1; ++cc) {
            float& m8 = max8[(size_t)((cr / 8) * a.n8x + cc / 8)];
            float& m64 = max64[(size_t)((cr / 64) * a.n64x + cc / 64)];
            m8 = z > m8 ? z : m8;
            m64 = z > m64 ? z : m64;
          }
      }
    a.max8 = max8.data(); a.max64 = max64.data(); a.zrange = zrange.data();
  }
  if (nthreads < 1) nthreads = 1;
  if (nthreads > a.Ho) nthreads = (int)a.Ho;
  auto work = [&](int t0) {
    for (long i = t0; i < a.Ho; i += nthreads)
      for (long j = 0; j < a.Wo; ++j) {
        PerspBest best{-PERSP_INF, -1, 0.0, 0.0};
        if (H >= 2 && W >= 2) {
          const PerspRay ray = persp_ray(a.v, i, j);
          if (a.facade_on) persp_walls(a.plane, H, W, a.v, ray, best);
          if (skipping) {
            persp_walk(a, ray, best);
          } else {
            // the plain walk: every strip of one cell along the faster axis, the rows the line covers across it and one more each way
            const bool xmajor = std::fabs(ray.dx) >= std::fabs(ray.dy);
            const double ou = xmajor ? ray.ox : ray.oy, du = xmajor ? ray.dx : ray.dy, ov = xmajor ? ray.oy : ray.ox, dv = xmajor ? ray.dy : ray.dx;
            const long NU = (xmajor ? W : H) - 1, NV = (xmajor ? H : W) - 1;
            for (long m = 0; m < NU; ++m) {
              const double va = ov + (((double)m - ou) / du) * dv, vb = ov + (((double)(m + 1) - ou) / du) * dv;
              const double lo = std::floor(va < vb ? va : vb) - 1.0, hi = std::floor(va < vb ? vb : va) + 1.0;
              if (!(hi >= 0.0 && lo <= (double)(NV - 1))) continue;
              const long n_lo = lo < 0.0 ? 0 : (long)lo, n_hi = hi > (double)(NV - 1) ? NV - 1 : (long)hi;
              for (long n = n_lo; n <= n_hi; ++n) persp_cell(a.plane, W, xmajor ? n : m, xmajor ? m : n, a.v, ray, best);
            }
          }
        }
        const uint32_t p = persp_colour(a.drape, a.channels, W, best, persp_rgba(a.facade), persp_rgba(a.background));
        std::memcpy(a.out + 4 * (i * a.Wo + j), &p, 4);
        if (a.hits) a.hits[i * a.Wo + j] = best.id;
      }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nthreads; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& t : th) t.join();
}

extern "C" int dbm_grid_perspective_host(const float* plane, long H, long W, const uint8_t* drape, int drape_channels, const double* view, long Wo,
                                         long Ho, const uint8_t* facade_rgba, const uint8_t* background_rgba, uint8_t* out, int32_t* hits,
                                         int nthreads) {
  DBM_API_BEGIN(nullptr)
  PerspLaunch a{};
  perspective_check_arguments("dbm_grid_perspective_host", plane, H, W, drape, drape_channels, view, Wo, Ho, background_rgba, out, a.v);
  a.plane = plane;
  a.H = H; a.W = W;
  a.drape = drape;
  a.channels = drape_channels;
  a.Wo = Wo; a.Ho = Ho;
  a.facade_on = facade_rgba != nullptr;
  if (facade_rgba) std::memcpy(a.facade, facade_rgba, 4);
  std::memcpy(a.background, background_rgba, 4);
  a.out = out;
  a.hits = hits;
  perspective_render_host(a, false, nthreads);
  DBM_API_END
}
