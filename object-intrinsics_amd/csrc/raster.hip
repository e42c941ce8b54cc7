// A mesh rasteriser: the G-buffer of a triangle mesh in the arrays the surface shade reads (include/oi_raster.h; DESIGN section
// 4.33), gfx950.  Three stages, all memory-trivial next to an MLP pass:
//   setup    one thread per (view, triangle): project, snap to 24.8 fixed point, classify, compact the small and the large
//            triangles (wg_slot: one integer atomicAdd per workgroup and list)
//   fill     the visible triangle per pixel: exact int64 edge functions with the top-left rule, the depth of the pixel's own
//            make_ray ray against the triangle's plane, a 64-bit integer atomicMin on (float_as_uint(t) << 32) | f -- the
//            native global_atomic_umin_x2, no CAS loop, no float atomic.  Small triangles: a grid-stride loop of threads;
//            large ones: a grid-stride loop of waves, the lanes over 8 x 8 blocks of the box
//   resolve  one thread per (view, pixel): t recomputed by the function fill used, barycentrics, the vertex or texture
//            attributes, the ray state and the G-buffer
// No scratch, no LDS beyond the compaction's words; 64-bit indices; the view is blockIdx.y.  The ray is ray_common.h's, the
// compaction and the sample point trace_common.h's: nothing of them is restated.
#include "ray_common.h"
#include "trace_common.h"

#include "../../include/oi_raster.h"

namespace {

constexpr int RS_FIX = 256;                                     // 24.8 fixed point
constexpr long long RS_MAX_FIX = (long long)OI_RASTER_MAX_COORD * RS_FIX;   // 2^30
constexpr unsigned long long RS_NONE = ~0ull;
constexpr int RS_FILL_BLOCKS = 1024;                            // the most workgroups of one fill launch per view

struct Tri {
  float v[3][3];
};

// the three vertices of triangle f, or false when an index lies outside 0 .. V - 1
__device__ __forceinline__ bool load_tri(const float* __restrict__ pos, const int* __restrict__ triangles, long long V,
                                         long long f, Tri& T) {
  const int i0 = triangles[f * 3 + 0], i1 = triangles[f * 3 + 1], i2 = triangles[f * 3 + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return false;
  const int id[3] = {i0, i1, i2};
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int a = 0; a < 3; ++a) T.v[m][a] = pos[(long long)id[m] * 3 + a];
  return true;
}

// The raster coordinate of the box-frame point p in one view and its camera depth (include/oi_raster.h, GEOMETRY).
// Contraction off, as in the ray helpers: tests/helpers/raster_ref.py restates it.
__device__ __forceinline__ void project(const float* __restrict__ B /* b2c 4x4 */, const float* __restrict__ K, float offx,
                                        float offy, int R, const float* p, float& x, float& y, float& depth) {
#pragma clang fp contract(off)
  float pc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) pc[i] = B[i * 4 + 0] * p[0] + B[i * 4 + 1] * p[1] + B[i * 4 + 2] * p[2] + B[i * 4 + 3];
  const float qx = K[0] * pc[0] + K[1] * pc[1] + K[2] * pc[2];
  const float qy = K[3] * pc[0] + K[4] * pc[1] + K[5] * pc[2];
  const float scale = R > 1 ? (float)(R - 1) / (float)R : 1.f;
  x = (qx / pc[2] - offx) * scale;
  y = (qy / pc[2] - offy) * scale;
  depth = pc[2];
}

// rint(x * 256) as int32; false when x is not finite or beyond the limit
__device__ __forceinline__ bool snap(float x, int& out) {
  const float s = rintf(x * (float)RS_FIX);
  if (!finite_(s) || fabsf(s) > (float)RS_MAX_FIX) return false;
  out = (int)s;
  return true;
}

// (b - a) x (c - a) compared with 0 without leaving int64: each product is below 2^62 in magnitude
__device__ __forceinline__ int orientation(const int* a, const int* b, const int* c) {
  const long long l = ((long long)b[0] - a[0]) * ((long long)c[1] - a[1]);
  const long long r = ((long long)b[1] - a[1]) * ((long long)c[0] - a[0]);
  return l > r ? 1 : (l < r ? -1 : 0);
}

// Is the centre (PX, PY) (fixed point) on the inner side of the edge a -> b of a triangle of positive area?  The top-left rule.
__device__ __forceinline__ bool edge_in(const int* a, const int* b, long long PX, long long PY) {
  const long long dx = (long long)b[0] - a[0], dy = (long long)b[1] - a[1];
  const long long w = dx * (PY - a[1]) - dy * (PX - a[0]);
  return w > 0 || (w == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// c [3][2]: the snapped corners; orient: the sign of their area (never 0 here)
__device__ __forceinline__ bool covers(const int (*c)[2], int orient, int X, int Y) {
  const long long PX = (long long)X * RS_FIX, PY = (long long)Y * RS_FIX;
  const int* a = c[0];
  const int* b = orient > 0 ? c[1] : c[2];
  const int* d = orient > 0 ? c[2] : c[1];
  return edge_in(a, b, PX, PY) && edge_in(b, d, PX, PY) && edge_in(d, a, PX, PY);
}

// THE depth of a pixel on a triangle: the ray parameter of (o, d) on the plane of T, vertices in the order of `triangles`.
// fill and resolve both call it, so the key's t and the resolved t agree bit for bit.  Contraction off.
__device__ __forceinline__ float plane_t(const Tri& T, const RayOD& r, float* nrm) {
#pragma clang fp contract(off)
  float e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    e1[a] = T.v[1][a] - T.v[0][a];
    e2[a] = T.v[2][a] - T.v[0][a];
  }
  nrm[0] = e1[1] * e2[2] - e1[2] * e2[1];
  nrm[1] = e1[2] * e2[0] - e1[0] * e2[2];
  nrm[2] = e1[0] * e2[1] - e1[1] * e2[0];
  const float num = nrm[0] * (T.v[0][0] - r.o[0]) + nrm[1] * (T.v[0][1] - r.o[1]) + nrm[2] * (T.v[0][2] - r.o[2]);
  const float den = nrm[0] * r.d[0] + nrm[1] * r.d[1] + nrm[2] * r.d[2];
  return num / den;
}

__device__ __forceinline__ void view_offsets(const float* __restrict__ offs, long long e, float& ox, float& oy) {
  ox = offs ? offs[e * 2 + 0] : 0.f;
  oy = offs ? offs[e * 2 + 1] : 0.f;
}

__global__ void __launch_bounds__(TR_THREADS) raster_clear_kernel(int* __restrict__ counts, int n) {
  const int i = blockIdx.x * TR_THREADS + threadIdx.x;
  if (i < n) counts[i] = 0;
}

__global__ void __launch_bounds__(TR_THREADS) raster_setup_kernel(const float* __restrict__ b2c, const float* __restrict__ K,
                                                                  const float* __restrict__ offs, int R,
                                                                  const float* __restrict__ pos,
                                                                  const int* __restrict__ triangles, long long V, long long F,
                                                                  float near_, long long small_max, int* __restrict__ corners,
                                                                  int* __restrict__ bbox, uint8_t* __restrict__ cls,
                                                                  int* __restrict__ small_list, int* __restrict__ large_list,
                                                                  int* __restrict__ counts) {
  __shared__ unsigned lds_s[TR_WAVES + 1], lds_l[TR_WAVES + 1];
  const long long e = blockIdx.y;
  const long long f = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  int kind = -1;   // a thread past the last triangle
  if (f < F) {
    int c[3][2] = {{0, 0}, {0, 0}, {0, 0}}, box[4] = {0, 0, -1, -1};
    kind = OI_RASTER_DROPPED;
    Tri T;
    bool ok = load_tri(pos, triangles, V, f, T);
    if (ok) {
      float ox, oy;
      view_offsets(offs, e, ox, oy);
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        float x, y, depth;
        project(b2c + e * 16, K, ox, oy, R, T.v[m], x, y, depth);
        ok = ok && depth > near_ && snap(x, c[m][0]) && snap(y, c[m][1]);   // (a NaN depth fails the comparison)
      }
    }
    if (ok) {
      kind = OI_RASTER_EMPTY;
      const int lo_x = min(c[0][0], min(c[1][0], c[2][0])), hi_x = max(c[0][0], max(c[1][0], c[2][0]));
      const int lo_y = min(c[0][1], min(c[1][1], c[2][1])), hi_y = max(c[0][1], max(c[1][1], c[2][1]));
      // the centres 256 X inside [lo, hi]: ceil and floor of a division by 256 as arithmetic shifts
      const int x0 = max((lo_x + RS_FIX - 1) >> 8, 0), x1 = min(hi_x >> 8, R - 1);
      const int y0 = max((lo_y + RS_FIX - 1) >> 8, 0), y1 = min(hi_y >> 8, R - 1);
      if (orientation(c[0], c[1], c[2]) != 0 && x0 <= x1 && y0 <= y1) {
        box[0] = x0, box[1] = y0, box[2] = x1, box[3] = y1;
        kind = (long long)(x1 - x0 + 1) * (y1 - y0 + 1) <= small_max ? OI_RASTER_SMALL : OI_RASTER_LARGE;
      }
    } else {
#pragma unroll
      for (int m = 0; m < 3; ++m) c[m][0] = c[m][1] = 0;
    }
    const long long o = e * F + f;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      corners[o * 6 + m * 2 + 0] = c[m][0];
      corners[o * 6 + m * 2 + 1] = c[m][1];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) bbox[o * 4 + m] = box[m];
    cls[o] = (uint8_t)kind;
  }
  const long long ss = wg_slot(kind == OI_RASTER_SMALL, counts + e * 2 + 0, lds_s);
  const long long sl = wg_slot(kind == OI_RASTER_LARGE, counts + e * 2 + 1, lds_l);
  if (kind == OI_RASTER_SMALL) small_list[e * F + ss] = (int)f;   // (slot < F: at most F triangles are kept)
  if (kind == OI_RASTER_LARGE) large_list[e * F + sl] = (int)f;
}

// what fill needs of one listed triangle; false when the entry is not a valid triangle of this mesh with a box on the screen
struct FillTri {
  Tri T;
  int c[3][2], box[4], orient;
};
__device__ __forceinline__ bool load_fill(const float* __restrict__ pos, const int* __restrict__ triangles, long long V,
                                          long long F, const int* __restrict__ corners, const int* __restrict__ bbox, long long e,
                                          long long f, int R, FillTri& t) {
  if (f < 0 || f >= F || !load_tri(pos, triangles, V, f, t.T)) return false;
  const long long o = e * F + f;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    t.c[m][0] = corners[o * 6 + m * 2 + 0];
    t.c[m][1] = corners[o * 6 + m * 2 + 1];
    if (t.c[m][0] > RS_MAX_FIX || t.c[m][0] < -RS_MAX_FIX || t.c[m][1] > RS_MAX_FIX || t.c[m][1] < -RS_MAX_FIX) return false;
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) t.box[m] = bbox[o * 4 + m];
  t.orient = orientation(t.c[0], t.c[1], t.c[2]);
  return t.orient != 0 && t.box[0] >= 0 && t.box[1] >= 0 && t.box[2] < R && t.box[3] < R;   // (nothing is stored off the screen)
}

// one candidate: the centre (X, Y) of view e against triangle f
__device__ __forceinline__ void fill_pixel(const float* __restrict__ c2b, const float* __restrict__ kinv, float ox, float oy, int R,
                                           long long e, long long f, const FillTri& t, int X, int Y,
                                           unsigned long long* __restrict__ zbuf) {
  if (!covers(t.c, t.orient, X, Y)) return;
  const RayOD r = make_ray(c2b + e * 16, kinv, ox, oy, R, X, Y);
  float n[3];
  const float tt = plane_t(t.T, r, n);
  if (!finite_(tt) || !(tt > 0.f)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(tt) << 32) | (unsigned long long)(unsigned)f;
  atomicMin(zbuf + (e * R + Y) * (long long)R + X, key);
}

__global__ void __launch_bounds__(TR_THREADS) raster_fill_small_kernel(const float* __restrict__ c2b, const float* __restrict__ kinv,
                                                                       const float* __restrict__ offs, int R,
                                                                       const float* __restrict__ pos,
                                                                       const int* __restrict__ triangles, long long V, long long F,
                                                                       const int* __restrict__ corners, const int* __restrict__ bbox,
                                                                       const int* __restrict__ list, const int* __restrict__ counts,
                                                                       unsigned long long* __restrict__ zbuf) {
  const long long e = blockIdx.y;
  const long long n = min((long long)max(counts[e * 2 + 0], 0), F);
  float ox, oy;
  view_offsets(offs, e, ox, oy);
  for (long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * TR_THREADS) {
    const long long f = list[e * F + i];
    FillTri t;
    if (!load_fill(pos, triangles, V, F, corners, bbox, e, f, R, t)) continue;
    for (int Y = t.box[1]; Y <= t.box[3]; ++Y)
      for (int X = t.box[0]; X <= t.box[2]; ++X) fill_pixel(c2b, kinv, ox, oy, R, e, f, t, X, Y, zbuf);
  }
}

__global__ void __launch_bounds__(TR_THREADS) raster_fill_large_kernel(const float* __restrict__ c2b, const float* __restrict__ kinv,
                                                                       const float* __restrict__ offs, int R,
                                                                       const float* __restrict__ pos,
                                                                       const int* __restrict__ triangles, long long V, long long F,
                                                                       const int* __restrict__ corners, const int* __restrict__ bbox,
                                                                       const int* __restrict__ list, const int* __restrict__ counts,
                                                                       unsigned long long* __restrict__ zbuf) {
  const long long e = blockIdx.y;
  const long long n = min((long long)max(counts[e * 2 + 1], 0), F);
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * TR_WAVES + (threadIdx.x >> 6), waves = (long long)gridDim.x * TR_WAVES;
  float ox, oy;
  view_offsets(offs, e, ox, oy);
  for (long long i = wave; i < n; i += waves) {
    const long long f = __builtin_amdgcn_readfirstlane(list[e * F + i]);   // one triangle per wave: uniform loads
    FillTri t;
    if (!load_fill(pos, triangles, V, F, corners, bbox, e, f, R, t)) continue;
    for (int by = t.box[1]; by <= t.box[3]; by += 8)
      for (int bx = t.box[0]; bx <= t.box[2]; bx += 8) {
        const int X = bx + (lane & 7), Y = by + (lane >> 3);
        if (X <= t.box[2] && Y <= t.box[3]) fill_pixel(c2b, kinv, ox, oy, R, e, f, t, X, Y, zbuf);
      }
  }
}

struct ResolveArgs {
  const float *c2b, *kinv, *offs, *pos;
  const int* triangles;
  long long V, F;
  const unsigned long long* zbuf;
  int R, mode, W, H;
  const float *vnormal, *valbedo, *uv, *albedo_f32, *normal_f32;
  const unsigned char *albedo_u8, *normal_u8;
  float *rays_o, *rays_d, *t;
  uint8_t* status;
  int* hit_slot;
  float *hit_points, *grad, *rgb;
  int* triangle;
  float* barycentric;
};

// one tap of an atlas [H][W][3], byte or float; decode: v = byte * scale + bias
__device__ __forceinline__ void tap(const unsigned char* __restrict__ a8, const float* __restrict__ a32, int W, int x, int y,
                                    float scale, float bias, float w, float* acc) {
  const long long o = ((long long)y * W + x) * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float v = a8 ? __fmaf_rn((float)a8[o + a], scale, bias) : a32[o + a];
    acc[a] = __fmaf_rn(w, v, acc[a]);
  }
}

// the bilinear lookup of include/oi_raster.h at (u, v): row 0 on top, texel centres at + 0.5, clamp addressing
__device__ __forceinline__ void lookup(const unsigned char* __restrict__ a8, const float* __restrict__ a32, int W, int H, float u,
                                       float v, float scale, float bias, float* out) {
  const float x = __fmaf_rn(u, (float)W, -0.5f), y = __fmaf_rn(1.f - v, (float)H, -0.5f);
  const float xf = floorf(x), yf = floorf(y);
  const float fx = x - xf, fy = y - yf;
  // (a NaN or huge coordinate: the clamps below keep every tap inside the atlas)
  const int xi = (int)fminf(fmaxf(xf, -1.f), (float)W), yi = (int)fminf(fmaxf(yf, -1.f), (float)H);
  const int xa = min(max(xi, 0), W - 1), xb = min(max(xi + 1, 0), W - 1);
  const int ya = min(max(yi, 0), H - 1), yb = min(max(yi + 1, 0), H - 1);
  out[0] = out[1] = out[2] = 0.f;
  tap(a8, a32, W, xa, ya, scale, bias, (1.f - fx) * (1.f - fy), out);
  tap(a8, a32, W, xb, ya, scale, bias, fx * (1.f - fy), out);
  tap(a8, a32, W, xa, yb, scale, bias, (1.f - fx) * fy, out);
  tap(a8, a32, W, xb, yb, scale, bias, fx * fy, out);
}

__device__ __forceinline__ float sub_area(const float* n, const float* a, const float* b, const float* p) {
  const float ax = a[0] - p[0], ay = a[1] - p[1], az = a[2] - p[2];
  const float bx = b[0] - p[0], by = b[1] - p[1], bz = b[2] - p[2];
  return n[0] * (ay * bz - az * by) + n[1] * (az * bx - ax * bz) + n[2] * (ax * by - ay * bx);
}

__device__ __forceinline__ void store3(float* __restrict__ dst, long long i, float x, float y, float z) {
  if (dst) {
    dst[i * 3 + 0] = x;
    dst[i * 3 + 1] = y;
    dst[i * 3 + 2] = z;
  }
}

__global__ void __launch_bounds__(TR_THREADS) raster_resolve_kernel(const ResolveArgs A) {
  const long long N = (long long)A.R * A.R, e = blockIdx.y;
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= N) return;
  const long long g = e * N + q;
  const int Y = (int)(q / A.R), X = (int)(q - (long long)Y * A.R);
  float ox, oy;
  view_offsets(A.offs, e, ox, oy);
  const RayOD r = make_ray(A.c2b + e * 16, A.kinv, ox, oy, A.R, X, Y);
  store3(A.rays_o, g, r.o[0], r.o[1], r.o[2]);
  store3(A.rays_d, g, r.d[0], r.d[1], r.d[2]);
  if (A.hit_slot) A.hit_slot[g] = (int)q;

  const unsigned long long key = A.zbuf[g];
  const long long f = (long long)(key & 0xffffffffull);
  Tri T;
  float n[3] = {0.f, 0.f, 0.f}, tt = 0.f;
  bool hit = key != RS_NONE && f < A.F && load_tri(A.pos, A.triangles, A.V, f, T);
  if (hit) {
    tt = plane_t(T, r, n);
    hit = finite_(tt) && tt > 0.f;
  }
  if (!hit) {
    if (A.t) A.t[g] = 0.f;
    if (A.status) A.status[g] = OI_TRACE_MISS;
    store3(A.hit_points, g, 0.f, 0.f, 0.f);
    store3(A.grad, g, 0.f, 0.f, 0.f);
    store3(A.rgb, g, 0.f, 0.f, 0.f);
    store3(A.barycentric, g, 0.f, 0.f, 0.f);
    if (A.triangle) A.triangle[g] = -1;
    return;
  }
  float p[3];
  point_at(r.o, r.d, 0, tt, p);
  float b0 = fmaxf(sub_area(n, T.v[1], T.v[2], p), 0.f), b1 = fmaxf(sub_area(n, T.v[2], T.v[0], p), 0.f),
        b2 = fmaxf(sub_area(n, T.v[0], T.v[1], p), 0.f);   // (fmaxf drops a NaN)
  const float s = b0 + b1 + b2;
  if (s > 0.f && finite_(s)) {
    b0 /= s, b1 /= s, b2 /= s;
  } else {
    b0 = 1.f, b1 = 0.f, b2 = 0.f;
  }
  float nn[3], col[3];
  if (A.mode == OI_RASTER_VERTEX) {
    const int* tri = A.triangles + f * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      nn[a] = __fmaf_rn(b2, A.vnormal[(long long)tri[2] * 3 + a],
                        __fmaf_rn(b1, A.vnormal[(long long)tri[1] * 3 + a], b0 * A.vnormal[(long long)tri[0] * 3 + a]));
      col[a] = __fmaf_rn(b2, A.valbedo[(long long)tri[2] * 3 + a],
                         __fmaf_rn(b1, A.valbedo[(long long)tri[1] * 3 + a], b0 * A.valbedo[(long long)tri[0] * 3 + a]));
    }
  } else {
    const float* w = A.uv + f * 6;
    const float u = __fmaf_rn(b2, w[4], __fmaf_rn(b1, w[2], b0 * w[0]));
    const float v = __fmaf_rn(b2, w[5], __fmaf_rn(b1, w[3], b0 * w[1]));
    lookup(A.albedo_u8, A.albedo_f32, A.W, A.H, u, v, 1.f / 255.f, 0.f, col);
    lookup(A.normal_u8, A.normal_f32, A.W, A.H, u, v, 2.f / 255.f, -1.f, nn);
  }
  float ux, uy, uz;
  unit_normal(nn[0], nn[1], nn[2], ux, uy, uz);
  if (A.t) A.t[g] = tt;
  if (A.status) A.status[g] = OI_TRACE_HIT;
  store3(A.hit_points, g, p[0], p[1], p[2]);
  store3(A.grad, g, ux, uy, uz);
  store3(A.rgb, g, col[0], col[1], col[2]);
  store3(A.barycentric, g, b0, b1, b2);
  if (A.triangle) A.triangle[g] = (int)f;
}

// what the three entries check of the views and the mesh
int check_views(const char* what, int R, int E, long long V, long long F) {
  OI_REQUIRE(E >= 1 && E <= OI_RASTER_MAX_VIEWS, "%s: E=%d views (1 <= E <= %d)", what, E, OI_RASTER_MAX_VIEWS);
  OI_REQUIRE(R >= 1 && R <= OI_RASTER_MAX_RESOLUTION, "%s: resolution R=%d (1 <= R <= %d)", what, R, OI_RASTER_MAX_RESOLUTION);
  OI_REQUIRE((long long)E * R * R < (1ll << 31), "%s: E=%d views of %d x %d pixels (E * R * R < 2^31)", what, E, R, R);
  OI_REQUIRE(F >= 0 && F < (1ll << 31), "%s: F=%lld triangles (0 <= F < 2^31)", what, F);
  OI_REQUIRE(V >= 0 && V < (1ll << 31) && (F == 0 || V >= 1), "%s: V=%lld vertices for F=%lld triangles (1 <= V < 2^31)", what, V, F);
  return OI_OK;
}

}  // namespace

extern "C" {

int oi_raster_setup(const float* b2c, const float* K, const float* offs, int R, int E, const float* pos, const int* triangles,
                    long long V, long long F, float near_, long long small_max, int* corners, int* bbox, uint8_t* cls,
                    int* small_list, int* large_list, int* counts, oi_stream_t stream) {
  int rc = check_views("oi_raster_setup", R, E, V, F);
  if (rc != OI_OK) return rc;
  OI_REQUIRE(near_ > 0.f && near_ < INFINITY, "oi_raster_setup: near=%g (positive and finite)", (double)near_);
  OI_REQUIRE(small_max >= 0, "oi_raster_setup: small_max=%lld (>= 0)", small_max);
  if (F == 0) return OI_OK;
  OI_REQUIRE((long long)E * F < (1ll << 31), "oi_raster_setup: E=%d views of F=%lld triangles (E * F < 2^31)", E, F);
  OI_REQUIRE(b2c && K && pos && triangles && corners && bbox && cls && small_list && large_list && counts,
             "oi_raster_setup: null pointer");
  hipLaunchKernelGGL(raster_clear_kernel, dim3(n_blocks(2 * E)), dim3(TR_THREADS), 0, oi::as_stream(stream), counts, 2 * E);
  hipLaunchKernelGGL(raster_setup_kernel, dim3(n_blocks(F), E), dim3(TR_THREADS), 0, oi::as_stream(stream), b2c, K, offs, R, pos,
                     triangles, V, F, near_, small_max, corners, bbox, cls, small_list, large_list, counts);
  return oi::check_launch("oi_raster_setup");
}

int oi_raster_fill(const float* c2b, const float* kinv, const float* offs, int R, int E, const float* pos, const int* triangles,
                   long long V, long long F, const int* corners, const int* bbox, const int* small_list, const int* large_list,
                   const int* counts, unsigned long long* zbuf, oi_stream_t stream) {
  int rc = check_views("oi_raster_fill", R, E, V, F);
  if (rc != OI_OK) return rc;
  if (F == 0) return OI_OK;
  OI_REQUIRE((long long)E * F < (1ll << 31), "oi_raster_fill: E=%d views of F=%lld triangles (E * F < 2^31)", E, F);
  OI_REQUIRE(c2b && kinv && pos && triangles && corners && bbox && small_list && large_list && counts && zbuf,
             "oi_raster_fill: null pointer");
  // grid-stride loops over the lists, whose lengths only the device knows: F bounds both
  const unsigned bs = n_blocks(F) < (unsigned)RS_FILL_BLOCKS ? n_blocks(F) : (unsigned)RS_FILL_BLOCKS;
  const long long wl = (F + TR_WAVES - 1) / TR_WAVES;
  const unsigned bl = wl < RS_FILL_BLOCKS ? (unsigned)wl : (unsigned)RS_FILL_BLOCKS;
  hipLaunchKernelGGL(raster_fill_small_kernel, dim3(bs, E), dim3(TR_THREADS), 0, oi::as_stream(stream), c2b, kinv, offs, R, pos,
                     triangles, V, F, corners, bbox, small_list, counts, zbuf);
  hipLaunchKernelGGL(raster_fill_large_kernel, dim3(bl, E), dim3(TR_THREADS), 0, oi::as_stream(stream), c2b, kinv, offs, R, pos,
                     triangles, V, F, corners, bbox, large_list, counts, zbuf);
  return oi::check_launch("oi_raster_fill");
}

int oi_raster_resolve(const float* c2b, const float* kinv, const float* offs, int R, int E, const float* pos,
                      const int* triangles, long long V, long long F, const unsigned long long* zbuf, int mode,
                      const float* vnormal, const float* valbedo, const float* uv, int W, int H,
                      const unsigned char* albedo_u8, const float* albedo_f32, const unsigned char* normal_u8,
                      const float* normal_f32, float* rays_o, float* rays_d, float* t, uint8_t* status, int* hit_slot,
                      float* hit_points, float* grad, float* rgb, int* triangle, float* barycentric, oi_stream_t stream) {
  int rc = check_views("oi_raster_resolve", R, E, V, F);
  if (rc != OI_OK) return rc;
  OI_REQUIRE(mode == OI_RASTER_VERTEX || mode == OI_RASTER_TEXTURE, "oi_raster_resolve: mode=%d (OI_RASTER_VERTEX or OI_RASTER_TEXTURE)",
             mode);
  OI_REQUIRE(c2b && kinv && zbuf && (F == 0 || (pos && triangles)), "oi_raster_resolve: null pointer");
  if (F > 0 && mode == OI_RASTER_VERTEX) {
    OI_REQUIRE(vnormal && valbedo, "oi_raster_resolve: mode OI_RASTER_VERTEX needs vnormal and valbedo");
  } else if (F > 0) {
    OI_REQUIRE(uv, "oi_raster_resolve: mode OI_RASTER_TEXTURE needs uv");
    OI_REQUIRE(W >= 1 && W <= OI_TEX_MAX_SIZE && H >= 1 && H <= OI_TEX_MAX_SIZE, "oi_raster_resolve: atlas of %d x %d texels (1 .. %d)",
               W, H, OI_TEX_MAX_SIZE);
    OI_REQUIRE((albedo_u8 != nullptr) != (albedo_f32 != nullptr), "oi_raster_resolve: exactly one of albedo_u8 and albedo_f32");
    OI_REQUIRE((normal_u8 != nullptr) != (normal_f32 != nullptr), "oi_raster_resolve: exactly one of normal_u8 and normal_f32");
  }
  if (!(rays_o || rays_d || t || status || hit_slot || hit_points || grad || rgb || triangle || barycentric)) return OI_OK;
  ResolveArgs A;
  A.c2b = c2b, A.kinv = kinv, A.offs = offs, A.pos = pos, A.triangles = triangles, A.V = V, A.F = F, A.zbuf = zbuf;
  A.R = R, A.mode = mode, A.W = W, A.H = H;
  A.vnormal = vnormal, A.valbedo = valbedo, A.uv = uv, A.albedo_f32 = albedo_f32, A.normal_f32 = normal_f32;
  A.albedo_u8 = albedo_u8, A.normal_u8 = normal_u8;
  A.rays_o = rays_o, A.rays_d = rays_d, A.t = t, A.status = status, A.hit_slot = hit_slot, A.hit_points = hit_points;
  A.grad = grad, A.rgb = rgb, A.triangle = triangle, A.barycentric = barycentric;
  hipLaunchKernelGGL(raster_resolve_kernel, dim3(n_blocks((long long)R * R), E), dim3(TR_THREADS), 0, oi::as_stream(stream), A);
  return oi::check_launch("oi_raster_resolve");
}

}  // extern "C"
