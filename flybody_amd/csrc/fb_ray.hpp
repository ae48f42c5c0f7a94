// Batched ray casting (fb_batch_ray): MuJoCo's mj_ray / mj_multiRay and the rangefinder sensor for many rays in many live
// environments, against the model's geoms as the last step, reset or fb_batch_forward left them (FB_GEOM_XPOS / FB_GEOM_XMAT) and against an
// optional caller-supplied height field.  The kernel only READS the environments' rows.
//
// SHAPE.  One lane per ray, FB_RAY_PER_LANE rays per lane one after the other; no cross-lane operation, no atomics, no global scratch.  A
// 1-D grid of 256-thread workgroups; a workgroup belongs to ONE frame and works a tile of FB_RAY_TILE of its rays, which amortises the
// staging: the frame's VISIBLE geoms (the host compacts the list by geom_mask and bodyexclude) go into LDS as RayGeom records -- world
// position, rotation, size, bounding radius, type, id: 136 B in FP64, 9.9 KB for the fly's 73 geoms -- in chunks of FB_RAY_CHUNK, so a
// larger model loops.  Every lane then walks the same list: all lanes read the same LDS address (a broadcast, no bank conflict), the type
// branch is wave-uniform, and a bounding-sphere test on rbound stands in front of the exact intersection.
//
// ARITHMETIC runs at the batch's precision; the FP32 build shares the code, so no discriminant is formed as |o|^2 - r^2: every quadratic
// is solved from the closest-approach vector q = p + tc v (|q|^2 against r^2), whose error does not grow with the distance of the origin.
// The direction is normalised on entry and the result divided by |dir| at the end: distances are in units of |dir| as in mj_ray.
//
// NO FAULT FOR ANY INPUT.  Every loop is bounded by an argument the host validated (n_vis <= ngeom, FB_RAY_PER_LANE, nrow + ncol + 2 cells of
// the terrain walk); every index into the height samples is clamped as a real BEFORE it becomes an integer (NaN goes to 0); a zero or
// non-finite ray is a miss before anything is indexed with it; comparisons are written so that a NaN ends a loop instead of continuing it.
#pragma once
#include "fb_types.hpp"

#define FB_RAY_THREADS 256
#define FB_RAY_PER_LANE 4
#define FB_RAY_TILE (FB_RAY_THREADS*FB_RAY_PER_LANE)      // rays of one workgroup
#define FB_RAY_CHUNK 96                                   // geoms staged at a time (13 KB of LDS in FP64)
#define FB_RAY_MAXGRID 4096                               // nrow, ncol of a terrain

template <typename real>
struct RayGeom { real pos[3], mat[9], size[3], rbound; int type, id; };

template <typename real>
struct RayArgs {
  const real* rarena;             // the environments' rows; row stride and the offsets of the four pose arrays in it
  unsigned nreal, o_gxpos, o_gxmat, o_xpos, o_xquat;
  const real *geom_size, *geom_rbound; const int* geom_type;      // model tables
  const int* vis; int n_vis;      // visible geoms, ascending
  const int* frame_env;           // [n_frames]
  const int* frame_terrain;       // [n_frames], or null: terrain 0
  const double* rays; float* dist; int* geomid;
  int n_frames, n_ray, per_frame, body, ngeom, tiles;   // tiles: workgroups per frame
  real cutoff;                    // > 0, +inf: none
  // terrain (data null: none)
  const float* hdata; int nrow, ncol;
  real rx, ry, elev, base, tpos[3];
};

#define FBR __device__ __forceinline__

// False for NaN and +-inf.  By comparison only: `x - x == 0` is not safe on the device, where the compiler fuses the subtraction into the
// multiply-adds that formed x (fma(a, b, c - x) is the rounding residue of x, not 0) and a finite ray tests as non-finite.
template <typename real> FBR bool ray_finite(real x) { return x > -(real)INFINITY && x < (real)INFINITY; }
FBR double ray_sqrt(double x) { return x > 0 ? sqrt(x) : 0.0; }
FBR float ray_sqrt(float x) { return x > 0 ? sqrtf(x) : 0.0f; }
// candidate distance t: kept when 0 <= t < best (a NaN fails both)
template <typename real> FBR void ray_take(real t, real& best) { if (t >= 0 && t < best) best = t; }

// |p + t v|^2 = r2 in `dim` dimensions (v need not be unit: a = |v|^2 > 0): tc, the parameter of closest approach, and s, the half-length of the
// chord, from q = p + tc v.  False: no real root.
template <typename real>
FBR bool ray_chord(const real* p, const real* v, int dim, real r2, real& tc, real& s) {
  real a = 0, b = 0;
  for (int k = 0; k < dim; k++) { a += v[k]*v[k]; b += p[k]*v[k]; }
  if (!(a > 0)) return false;
  tc = -b/a;
  real q2 = 0;
  for (int k = 0; k < dim; k++) { const real q = p[k] + tc*v[k]; q2 += q*q; }
  const real d = r2 - q2;
  if (!(d >= 0)) return false;
  s = ray_sqrt(d/a);
  return ray_finite(tc);
}

// Smallest t >= 0 with p + t v on the geom's boundary, in the geom's frame (v unit); `best` where there is none below it.
template <typename real>
FBR real ray_geom_local(int type, const real* size, const real* p, const real* v, real best) {
  real tc, s;
  if (type == GEOM_PLANE) {
    if (v[2] < 0) {
      const real t = -p[2]/v[2];
      const real x = p[0] + t*v[0], y = p[1] + t*v[1];
      const bool in = (!(size[0] > 0) || (x >= -size[0] && x <= size[0])) && (!(size[1] > 0) || (y >= -size[1] && y <= size[1]));
      if (in) ray_take(t, best);
    }
  } else if (type == GEOM_SPHERE) {
    if (ray_chord(p, v, 3, size[0]*size[0], tc, s)) { ray_take(tc + s, best); ray_take(tc - s, best); }
  } else if (type == GEOM_ELLIPSOID) {
    if (size[0] > 0 && size[1] > 0 && size[2] > 0) {
      const real ps[3] = {p[0]/size[0], p[1]/size[1], p[2]/size[2]}, vs[3] = {v[0]/size[0], v[1]/size[1], v[2]/size[2]};
      if (ray_chord(ps, vs, 3, (real)1, tc, s)) { ray_take(tc + s, best); ray_take(tc - s, best); }
    }
  } else if (type == GEOM_CAPSULE || type == GEOM_CYLINDER) {
    const real r = size[0], h = size[1];
    if (ray_chord(p, v, 2, r*r, tc, s)) {                   // the side, between the end planes
      for (int k = 0; k < 2; k++) {
        const real t = k ? tc + s : tc - s, z = p[2] + t*v[2];
        if (z >= -h && z <= h) ray_take(t, best);
      }
    }
    for (int e = 0; e < 2; e++) {
      const real ze = e ? h : -h;
      if (type == GEOM_CYLINDER) {                          // a disc
        if (v[2] != 0) {
          const real t = (ze - p[2])/v[2];
          const real x = p[0] + t*v[0], y = p[1] + t*v[1];
          if (x*x + y*y <= r*r) ray_take(t, best);
        }
      } else {                                              // the outer half of the sphere around the cap centre
        const real pc[3] = {p[0], p[1], p[2] - ze};
        if (ray_chord(pc, v, 3, r*r, tc, s)) {
          for (int k = 0; k < 2; k++) {
            const real t = k ? tc + s : tc - s, z = pc[2] + t*v[2];
            if (e ? z >= 0 : z <= 0) ray_take(t, best);
          }
        }
      }
    }
  }
  return best;
}

// ---- terrain: the solid {|x| <= rx, |y| <= ry, -base <= z <= h(x, y)} in the terrain's frame (axis-aligned, at tpos)
// a real clamped into [0, hi] and made an index; NaN: 0
template <typename real> FBR int ray_index(real f, int hi) { return !(f >= 0) ? 0 : (f > (real)hi ? hi : (int)f); }

template <typename real>
struct RayCell { real x0, y0, h00, h01, h10, h11; };        // corner (row j, column i) of the cell and its four heights (hRC: row + R, column + C)

template <typename real>
FBR RayCell<real> ray_cell(const RayArgs<real>& A, const float* H, int i, int j, real dx, real dy) {
  RayCell<real> c;
  const size_t k = (size_t)j*A.ncol + i;
  c.x0 = -A.rx + dx*(real)i; c.y0 = -A.ry + dy*(real)j;
  c.h00 = A.elev*(real)H[k]; c.h01 = A.elev*(real)H[k + 1]; c.h10 = A.elev*(real)H[k + A.ncol]; c.h11 = A.elev*(real)H[k + A.ncol + 1];
  return c;
}

// the surface's height at (x, y), which lies in (or beside: clamped) the cell
template <typename real>
FBR real ray_cell_height(const RayCell<real>& c, real x, real y, real dx, real dy) {
  real fx = (x - c.x0)/dx, fy = (y - c.y0)/dy;
  fx = !(fx >= 0) ? 0 : (fx > 1 ? 1 : fx); fy = !(fy >= 0) ? 0 : (fy > 1 ? 1 : fy);
  return fy >= fx ? c.h00 + fx*(c.h11 - c.h10) + fy*(c.h10 - c.h00)       // triangle (v00, v11, v10)
                  : c.h00 + fx*(c.h01 - c.h00) + fy*(c.h11 - c.h01);      // triangle (v00, v11, v01)
}

// First crossing of the solid's boundary along ow + t d (d unit, world frame), `best` where there is none below it.
// The surface is found by SIGN, not by triangle tests: g(t) = z(t) - h(x(t), y(t)) is evaluated where the ray enters the box, where it
// crosses each grid line and where it crosses a cell's diagonal -- between two such points it runs over ONE triangle, so g is linear
// there -- and the hit is where "at or below the surface" flips, interpolated inside that piece.  Every piece starts from the value
// the piece before ended with, so the chain of signs has no gap a ray could slip through, whatever the rounding, and no plane is ever
// extrapolated beyond its triangle (triangle tests with inclusive edges do that inside their band: 3e-5 in FP32 at a cell of size 1).
template <typename real>
FBR real ray_terrain(const RayArgs<real>& A, int terrain, const real* ow, const real* d, real best) {
  const real o[3] = {ow[0] - A.tpos[0], ow[1] - A.tpos[1], ow[2] - A.tpos[2]};
  const real lo[3] = {-A.rx, -A.ry, -A.base}, hi[3] = {A.rx, A.ry, A.elev};
  // the ray inside the bounding box: [t0, t1]
  real t0 = 0, t1 = best;
  for (int k = 0; k < 3; k++) {
    if (d[k] != 0) {
      const real ta = (lo[k] - o[k])/d[k], tb = (hi[k] - o[k])/d[k];
      const real tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
      if (tn > t0) t0 = tn;
      if (tf < t1) t1 = tf;
    } else if (!(o[k] >= lo[k] && o[k] <= hi[k])) return best;
  }
  if (!(t0 <= t1)) return best;
  const float* H = A.hdata + (size_t)terrain*A.nrow*A.ncol;
  const real dx = 2*A.rx/(real)(A.ncol - 1), dy = 2*A.ry/(real)(A.nrow - 1);
  real xa = o[0] + t0*d[0], ya = o[1] + t0*d[1];
  int i = ray_index((xa + A.rx)/dx, A.ncol - 2), j = ray_index((ya + A.ry)/dy, A.nrow - 2);
  RayCell<real> c = ray_cell(A, H, i, j, dx, dy);
  real ta = t0, ga = o[2] + t0*d[2] - ray_cell_height(c, xa, ya, dx, dy);
  const bool inside = ga <= 0;
  if (inside && t0 > 0) return t0;                          // it enters the box through a wall or the bottom, below the surface
  const int si = d[0] > 0 ? 1 : -1, sj = d[1] > 0 ? 1 : -1;
  const int maxit = A.nrow + A.ncol + 2;
  for (int it = 0; it < maxit; it++) {
    // where the ray leaves the cell: the grid line it reaches first (none for a vertical ray), or the box
    const real tx = d[0] != 0 ? ((d[0] > 0 ? c.x0 + dx : c.x0) - o[0])/d[0] : (real)INFINITY;
    const real ty = d[1] != 0 ? ((d[1] > 0 ? c.y0 + dy : c.y0) - o[1])/d[1] : (real)INFINITY;
    const bool by_x = tx <= ty;
    real tb = by_x ? tx : ty;
    const bool last = !(tb <= t1);                          // (a NaN ends the walk as well)
    if (last) tb = t1;
    // the cell's diagonal fy = fx inside [ta, tb] splits the piece in two
    const real xb = o[0] + tb*d[0], yb = o[1] + tb*d[1];
    const real ea = (ya - c.y0)/dy - (xa - c.x0)/dx, eb = (yb - c.y0)/dy - (xb - c.x0)/dx;
    const bool split = (ea > 0) != (eb > 0) && ea != eb;
    const real tm = split ? ta + (tb - ta)*(ea/(ea - eb)) : tb;
    for (int seg = split ? 0 : 1; seg < 2; seg++) {
      const real te = seg ? tb : tm;
      const real xe = o[0] + te*d[0], ye = o[1] + te*d[1];
      const real ge = o[2] + te*d[2] - ray_cell_height(c, xe, ye, dx, dy);
      if ((ge <= 0) != (ga <= 0)) {                         // the surface is crossed inside [ta, te]
        const real den = ga - ge;
        real t = den != 0 ? ta + (te - ta)*(ga/den) : te;
        t = !(t >= ta) ? ta : (t > te ? te : t);
        return t < best ? t : best;
      }
      ta = te; ga = ge; xa = xe; ya = ye;
    }
    if (last) break;
    if (by_x) i += si; else j += sj;
    if (i < 0 || i > A.ncol - 2 || j < 0 || j > A.nrow - 2) break;
    c = ray_cell(A, H, i, j, dx, dy);
  }
  return inside ? t1 : best;                                // from inside the solid it leaves through a wall or the bottom
}

// quaternion (w, x, y, z) -> row-major rotation; a zero or non-finite one gives what it gives: the ray is then a miss by its own test
template <typename real>
FBR void ray_quat2mat(real* m, const real* q) {
  const real w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w*w + x*x - y*y - z*z; m[1] = 2*(x*y - w*z); m[2] = 2*(x*z + w*y);
  m[3] = 2*(x*y + w*z); m[4] = w*w - x*x + y*y - z*z; m[5] = 2*(y*z - w*x);
  m[6] = 2*(x*z - w*y); m[7] = 2*(y*z + w*x); m[8] = w*w - x*x - y*y + z*z;
}

// geoms vis[base .. base + cnt) of the frame into the workgroup's LDS records
template <typename real>
FBR void ray_stage(const RayArgs<real>& A, const real* row, RayGeom<real>* s_geom, int base, int cnt, int tid) {
  for (int k = tid; k < cnt; k += FB_RAY_THREADS) {
    const int g = A.vis[base + k];
    RayGeom<real>& G = s_geom[k];
    for (int c = 0; c < 3; c++) { G.pos[c] = row[A.o_gxpos + 3*g + c]; G.size[c] = A.geom_size[3*g + c]; }
    for (int c = 0; c < 9; c++) G.mat[c] = row[A.o_gxmat + 9*g + c];
    G.rbound = A.geom_rbound[g]; G.type = A.geom_type[g]; G.id = g;
  }
}

template <typename real>
__global__ void __launch_bounds__(FB_RAY_THREADS) k_raycast(RayArgs<real> A) {
  __shared__ RayGeom<real> s_geom[FB_RAY_CHUNK];
  const int tid = threadIdx.x;
  const int frame = (int)(blockIdx.x/(unsigned)A.tiles), tile = (int)(blockIdx.x%(unsigned)A.tiles);
  if (frame >= A.n_frames) return;                          // (never: the grid is n_frames x tiles)
  const real* row = A.rarena + (size_t)A.frame_env[frame]*A.nreal;
  const int terrain = A.frame_terrain ? A.frame_terrain[frame] : 0;
  // the frame of the rays: a body's pose, or the world
  real bm[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, bp[3] = {0, 0, 0};
  if (A.body >= 0) {
    const real q[4] = {row[A.o_xquat + 4*A.body], row[A.o_xquat + 4*A.body + 1], row[A.o_xquat + 4*A.body + 2], row[A.o_xquat + 4*A.body + 3]};
    ray_quat2mat(bm, q);
    for (int k = 0; k < 3; k++) bp[k] = row[A.o_xpos + 3*A.body + k];
  }
  const bool one_chunk = A.n_vis <= FB_RAY_CHUNK;           // (every compiled model: staged once for the workgroup's whole tile)
  if (one_chunk) { ray_stage(A, row, s_geom, 0, A.n_vis, tid); __syncthreads(); }
  // The lane's rays, one after the other, each wholly in registers.  Every lane runs every iteration up to the barriers of a chunked
  // model, so those are workgroup-uniform.
#pragma unroll 1
  for (int k = 0; k < FB_RAY_PER_LANE; k++) {
    const int r = tile*FB_RAY_TILE + k*FB_RAY_THREADS + tid;
    // origin, unit direction, 1 / |dir|; an invalid ray has inv = 0 and is never tested
    real o[3] = {0, 0, 0}, d[3] = {0, 0, 0}, inv = 0, best = (real)INFINITY; int bid = -1;
    if (r < A.n_ray) {
      const double* src = A.rays + ((size_t)(A.per_frame ? frame : 0)*A.n_ray + r)*6;
      real v[6];
      bool ok = true;
      for (int c = 0; c < 6; c++) { v[c] = (real)src[c]; ok = ok && ray_finite(v[c]); }
      for (int c = 0; c < 3; c++) {
        o[c] = bp[c] + bm[3*c]*v[0] + bm[3*c + 1]*v[1] + bm[3*c + 2]*v[2];
        d[c] = bm[3*c]*v[3] + bm[3*c + 1]*v[4] + bm[3*c + 2]*v[5];
        ok = ok && ray_finite(o[c]) && ray_finite(d[c]);
      }
      const real len = ray_sqrt(d[0]*d[0] + d[1]*d[1] + d[2]*d[2]);
      ok = ok && len > 0 && ray_finite(len);
      const real il = ok ? (real)1/len : (real)0;
      if (ok && il > 0 && ray_finite(il)) {
        inv = il;
        for (int c = 0; c < 3; c++) d[c] *= il;
        // (a head start for the culling; the exact test is on the result)
        if (A.cutoff < (real)INFINITY) best = A.cutoff*len*((real)1 + (sizeof(real) == 8 ? (real)1e-14 : (real)1e-5));
      }
    }
    for (int base = 0; base < A.n_vis; base += FB_RAY_CHUNK) {
      const int cnt = A.n_vis - base < FB_RAY_CHUNK ? A.n_vis - base : FB_RAY_CHUNK;
      if (!one_chunk) { __syncthreads(); ray_stage(A, row, s_geom, base, cnt, tid); __syncthreads(); }
      if (!(inv > 0)) continue;
#pragma unroll 1
      for (int e = 0; e < cnt; e++) {
        const RayGeom<real>& G = s_geom[e];
        const real c[3] = {o[0] - G.pos[0], o[1] - G.pos[1], o[2] - G.pos[2]};
        if (G.type != GEOM_PLANE && G.rbound > 0) {          // bounding sphere: the LINE's closest approach, and the sphere neither wholly behind nor beyond best
          const real b = -(c[0]*d[0] + c[1]*d[1] + c[2]*d[2]);
          const real q[3] = {c[0] + b*d[0], c[1] + b*d[1], c[2] + b*d[2]};
          const real q2 = q[0]*q[0] + q[1]*q[1] + q[2]*q[2], rb = G.rbound*(real)1.001;
          if (q2 > rb*rb || b + rb < 0 || b - rb > best) continue;
        }
        real p[3], v[3];
        for (int a = 0; a < 3; a++) {
          p[a] = G.mat[a]*c[0] + G.mat[3 + a]*c[1] + G.mat[6 + a]*c[2];
          v[a] = G.mat[a]*d[0] + G.mat[3 + a]*d[1] + G.mat[6 + a]*d[2];
        }
        const real t = ray_geom_local(G.type, G.size, p, v, best);
        if (t < best) { best = t; bid = G.id; }
      }
    }
    if (r >= A.n_ray) continue;
    // terrain, then the result: plain stores
    float out = -1.0f; int id = -1;
    if (inv > 0) {
      if (A.hdata) {
        const real t = ray_terrain(A, terrain, o, d, best);
        if (t < best) { best = t; bid = A.ngeom; }
      }
      const real x = best*inv;
      const float xf = (float)x;                            // (a distance beyond float32's range is a miss, not an inf)
      if (bid >= 0 && x >= 0 && ray_finite(xf) && !(x > A.cutoff)) { out = xf; id = bid; }
    }
    const size_t w = (size_t)frame*A.n_ray + r;
    A.dist[w] = out; A.geomid[w] = id;
  }
}
