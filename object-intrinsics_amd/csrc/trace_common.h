// What trace.hip, occlusion.hip, trace_batch.hip, envlight.hip, envgloss.hip, scene.hip, scene_light.hip and envbounce.hip share
// (include/oi_trace.h, include/oi_occlusion.h, include/oi_trace_batch.h, include/oi_envlight.h, include/oi_scene.h,
// include/oi_scene_light.h, include/oi_envbounce.h; DESIGN sections 4.13, 4.16 - 4.22): the workgroup compaction, the state of
// a ray that starts (write_ray) and the compaction of the started rays (enter_rays): every begin kernel's, the ray state
// machine (the full one and its any-hit form, one template), the offset origin, the sample numbers and directions of the
// secondary rays (occlusion.hip, envgloss.hip), the lit share of a pixel's rays, the SH basis and the closed-form transfer of a
// normal, the shadow ray of a surface point, the per-pixel shading, and the argument checks the C entries repeat (check_*).
// (The environment shade's pixel is env_shade_common.h's; the unit normal, the view vector, the light's direction and the
// Phong geometry are shade_common.h's, shared with the compositing kernels.)  Local lights (local_light.hip,
// include/oi_local_light.h) add the shadow sample aimed at a sphere and the Phong pixel under them.
// Everything here has internal linkage; each source file instantiates what it exports.
#ifndef OI_TRACE_COMMON_H_
#define OI_TRACE_COMMON_H_

#include "shade_common.h"
#include "../../include/oi_occlusion.h"
#include "../../include/oi_trace_batch.h"
#include "../../include/oi_local_light.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int N_HIT_WORD = OI_TRACE_COUNT_WORDS - 1;
static_assert(OI_TRACE_COUNT_WORDS == OI_TRACE_MAX_STEPS + 2, "counts[0 .. MAX_STEPS] and the hit count");

__device__ __forceinline__ bool finite_(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the sample point of ray (o, d) at t: the one expression every kernel here uses, so a hit's position is bit-equal to the
// point the MLP was given
__device__ __forceinline__ void point_at(const float* __restrict__ o, const float* __restrict__ d, long long r, float t,
                                         float* __restrict__ dst) {
  dst[0] = __fmaf_rn(t, d[r * 3 + 0], o[r * 3 + 0]);
  dst[1] = __fmaf_rn(t, d[r * 3 + 1], o[r * 3 + 1]);
  dst[2] = __fmaf_rn(t, d[r * 3 + 2], o[r * 3 + 2]);
}

// p + bias n: the origin of a secondary ray, off the surface along the normal (the owner's frame or the world's)
__device__ __forceinline__ void offset_origin(const float* __restrict__ p, float bias, float nx, float ny, float nz, float& ox, float& oy,
                                              float& oz) {
  ox = __fmaf_rn(bias, nx, p[0]);
  oy = __fmaf_rn(bias, ny, p[1]);
  oz = __fmaf_rn(bias, nz, p[2]);
}

// Dense output slot of this thread (meaningful where `keep`), the workgroup's kept threads in thread order behind
// `*counter`'s previous value.  Every thread of the workgroup calls it.  lds: TR_WAVES + 1 words.
// live (the batched trace, include/oi_trace_batch.h): a word that follows the maximum of several counters.  The counter's
// value after this workgroup's add goes into it with one integer atomicMax; the workgroup that adds last holds the final
// count, so when the launch has ended the word is the largest of the final counts.
__device__ __forceinline__ long long wg_slot(bool keep, int* counter, unsigned* lds, int* live = nullptr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  const unsigned pre = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) lds[wave] = (unsigned)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned tot = 0;
    for (int w = 0; w < TR_WAVES; ++w) {
      const unsigned c = lds[w];
      lds[w] = tot;
      tot += c;
    }
    lds[TR_WAVES] = tot ? (unsigned)atomicAdd(counter, (int)tot) : 0u;
    if (live != nullptr && tot) atomicMax(live, (int)(lds[TR_WAVES] + tot));
  }
  __syncthreads();
  return (long long)lds[TR_WAVES] + lds[wave] + pre;
}

// element e's segment of every array of the batched state
__device__ __forceinline__ oi_trace_state element_view(const oi_trace_state& s, long long e) {
  const long long o = e * s.N;
  oi_trace_state v;
  v.N = s.N;
  v.rays_o = s.rays_o + o * 3;
  v.rays_d = s.rays_d + o * 3;
  v.near_ = s.near_ + o;
  v.far_ = s.far_ + o;
  v.t = s.t + o;
  v.status = s.status + o;
  v.steps = s.steps + o;
  v.bracket = s.bracket + o * 4;
  v.side = s.side + o;
  v.active = s.active + o * 2;
  v.points = s.points + o * 3;
  v.counts = s.counts + e * OI_TRACE_COUNT_WORDS;
  return v;
}

__device__ __forceinline__ void clear_counts(int* counts, int first) {
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < OI_TRACE_COUNT_WORDS; i += TR_THREADS) counts[i] = i == 0 ? first : 0;
}

__global__ void __launch_bounds__(TR_THREADS) trace_clear_counts_kernel(int* counts) { clear_counts(counts, 0); }

// ray r of v starts at near_: what every begin kernel writes besides the ray itself
__device__ __forceinline__ void restart_ray(const oi_trace_state& v, long long r, float near_, unsigned status) {
  v.t[r] = near_;
  v.status[r] = (uint8_t)status;
  v.steps[r] = 0;
  v.side[r] = 0;
  v.bracket[r * 4 + 0] = near_;
  v.bracket[r * 4 + 1] = 0.f;
  v.bracket[r * 4 + 2] = near_;
  v.bracket[r * 4 + 3] = 0.f;
}

// ray r of v, whole: (o, d) on near_ .. far_, started (MARCH) or ended before its first sample (0 .. 0 and a final status)
__device__ __forceinline__ void write_ray(const oi_trace_state& v, long long r, const float* o, const float* d, float near_,
                                          float far_, unsigned status) {
  v.rays_o[r * 3 + 0] = o[0], v.rays_o[r * 3 + 1] = o[1], v.rays_o[r * 3 + 2] = o[2];  // (each triple on its own: one 12-byte store)
  v.rays_d[r * 3 + 0] = d[0], v.rays_d[r * 3 + 1] = d[1], v.rays_d[r * 3 + 2] = d[2];
  v.near_[r] = near_;
  v.far_[r] = far_;
  restart_ray(v, r, near_, status);
}

// The started rays of this workgroup, compacted behind v's counter: the active list and the first sample points.  Every
// thread of the workgroup calls it; live: wg_slot's.  (px, py, pz): ray r's point at near_, values the caller holds in
// registers -- the origin itself where near_ is 0 (o + 0 d would lose the sign of a zero and turn a non-finite d into NaN),
// point_at's fmaf of the values it has just written otherwise.
__device__ __forceinline__ void enter_rays(const oi_trace_state& v, long long r, bool entered, float px, float py, float pz,
                                           unsigned* lds, int* live = nullptr) {
  const long long slot = wg_slot(entered, v.counts, lds, live);
  if (entered) {
    v.active[slot] = (int)r;
    v.points[slot * 3 + 0] = px, v.points[slot * 3 + 1] = py, v.points[slot * 3 + 2] = pz;
  }
}

// One step of the ray state machine on the sdf of the last MLP pass, and the compaction of the rays still in flight.
// ANYHIT = false: oi_trace_step (march, bracket, Illinois regula falsi).  ANYHIT = true: oi_occlusion_step, whose MARCH
// phase is the same and whose first later negative sample ends the ray as a HIT at that sample: there is no REFINE state.
// s: the state of the rays this workgroup serves (a whole trace, or one element's view of a batched one: element_view);
// live: wg_slot's, nullptr for a single trace.  Every thread of the workgroup calls it.
template <bool ANYHIT>
__device__ __forceinline__ void trace_step_rays(const oi_trace_state& s, const float* __restrict__ sdf, long long bound, int k,
                                                float tol, float omega, unsigned* lds, int* live = nullptr) {
  long long cnt = s.counts[k];
  cnt = cnt < bound ? cnt : bound;
  const long long j0 = (long long)blockIdx.x * TR_THREADS;
  if (j0 >= cnt) return;  // the whole workgroup: slots at or above the count hold rays that ended earlier
  const long long j = j0 + threadIdx.x;
  const int* __restrict__ act_in = s.active + (long long)(k & 1) * s.N;
  int* __restrict__ act_out = s.active + (long long)((k + 1) & 1) * s.N;
  bool alive = false;
  long long r = 0;
  float tn = 0.f;
  if (j < cnt) {
    r = act_in[j];
    const float v = sdf[j];
    float t = s.t[r];
    const unsigned n_eval = (unsigned)s.steps[r] + 1u;
    s.steps[r] = (uint16_t)n_eval;
    unsigned st = s.status[r];
    if (!finite_(v)) {
      st = OI_TRACE_NONFINITE;
    } else if (fabsf(v) <= tol) {
      st = OI_TRACE_HIT;
    } else if (st == OI_TRACE_MARCH && v > 0.f) {
      if (!ANYHIT) {  // the bracket's low end: only a refinement reads it
        s.bracket[r * 4 + 0] = t;
        s.bracket[r * 4 + 1] = v;
      }
      t += fmaxf(omega * v, tol);
      if (t > s.far_[r]) st = OI_TRACE_MISS;
      else alive = true;
    } else if (st == OI_TRACE_MARCH && n_eval == 1u) {
      st = OI_TRACE_START_INSIDE;
    } else if (ANYHIT) {
      st = OI_TRACE_HIT;  // an occluder: nobody reads the root
    } else {
      float t_lo = s.bracket[r * 4 + 0], s_lo = s.bracket[r * 4 + 1], t_hi, s_hi;
      unsigned side = 0;
      if (st == OI_TRACE_MARCH) {  // the first negative sample closes the bracket
        t_hi = t;
        s_hi = v;
        st = OI_TRACE_REFINE;
      } else {
        t_hi = s.bracket[r * 4 + 2];
        s_hi = s.bracket[r * 4 + 3];
        side = s.side[r];
        if (v > 0.f) {
          if (side == 1u) s_hi *= 0.5f;
          t_lo = t;
          s_lo = v;
          side = 1u;
        } else {
          if (side == 2u) s_lo *= 0.5f;
          t_hi = t;
          s_hi = v;
          side = 2u;
        }
      }
      t = __fmaf_rn(t_hi - t_lo, s_lo / (s_lo - s_hi), t_lo);
      if (!(t > t_lo && t < t_hi)) t = 0.5f * (t_lo + t_hi);
      if (!(t > t_lo && t < t_hi)) {  // the ends are adjacent numbers: nothing left to split
        t = t_hi;
        st = OI_TRACE_HIT;
      } else {
        alive = true;
        s.bracket[r * 4 + 0] = t_lo;
        s.bracket[r * 4 + 1] = s_lo;
        s.bracket[r * 4 + 2] = t_hi;
        s.bracket[r * 4 + 3] = s_hi;
        s.side[r] = (uint8_t)side;
      }
    }
    s.t[r] = t;
    s.status[r] = (uint8_t)st;
    tn = t;
  }
  const long long slot = wg_slot(alive, s.counts + k + 1, lds, live);
  if (alive) {
    act_out[slot] = (int)r;
    point_at(s.rays_o, s.rays_d, r, tn, s.points + slot * 3);
  }
}

template <bool ANYHIT>
__global__ void __launch_bounds__(TR_THREADS) trace_step_kernel(const oi_trace_state s, const float* __restrict__ sdf,
                                                                long long bound, int k, float tol, float omega) {
  __shared__ unsigned lds[TR_WAVES + 1];
  trace_step_rays<ANYHIT>(s, sdf, bound, k, tol, omega, lds);
}

// oi_trace_begin's work for ray blockIdx.x * TR_THREADS + threadIdx.x of s, and the counters of s.
__device__ __forceinline__ void trace_begin_rays(const oi_trace_state& s) {
  clear_counts(s.counts, (int)s.N);
  const long long r = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (r >= s.N) return;
  const float t = s.near_[r];  // (the caller's rays: nothing but restart_ray's part of write_ray is stored, and nothing is compacted)
  restart_ray(s, r, t, OI_TRACE_MARCH);
  s.active[r] = (int)r;
  point_at(s.rays_o, s.rays_d, r, t, s.points + r * 3);
}

// oi_trace_finish's work: rays in flight -> LIMIT, the hits listed densely (hit_index, hit_slot; POINTS: hit_points too).
// Every thread of the workgroup calls it; live: wg_slot's.
template <bool POINTS>
__device__ __forceinline__ void trace_finish_rays(const oi_trace_state& s, int* __restrict__ hit_index,
                                                  float* __restrict__ hit_points, int* __restrict__ hit_slot, unsigned* lds,
                                                  int* live = nullptr) {
  const long long r = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool hit = false;
  if (r < s.N) {
    unsigned st = s.status[r];
    if (st >= OI_TRACE_MARCH) {
      st = OI_TRACE_LIMIT;
      s.status[r] = (uint8_t)st;
    }
    hit = st == OI_TRACE_HIT;
  }
  const long long slot = wg_slot(hit, s.counts + N_HIT_WORD, lds, live);
  if (r < s.N) hit_slot[r] = hit ? (int)slot : -1;
  if (hit) {
    hit_index[slot] = (int)r;
    if (POINTS) point_at(s.rays_o, s.rays_d, r, s.t[r], hit_points + slot * 3);
  }
}

// The exit of the unit sphere along (o, d), |o + t d| = 1: 0 when the origin is outside and the ray leaves it.
__device__ __forceinline__ float unit_sphere_exit(float ox, float oy, float oz, float dx, float dy, float dz) {
  const float b = ox * dx + oy * dy + oz * dz, c = ox * ox + oy * oy + oz * oz - 1.0f;
  const float disc = b * b - c;
  return disc > 0.f ? fmaxf(sqrtf(disc) - b, 0.f) : 0.f;
}

// include/oi_occlusion.h's sample numbers: a 32-bit mix of (pixel, seed), one stratum per sample, a 24-bit rotation
__device__ __forceinline__ void sample_numbers(unsigned pix, unsigned seed, unsigned j, int S, float& u1, float& u2) {
  unsigned x = pix * 0x9E3779B9u + seed;
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  u1 = ((float)j + 0.5f) / (float)S;
  u2 = (float)((j * 2654435769u + x) >> 8) * 0x1p-24f;
}

// d = sa cos(phi) t1 + sa sin(phi) t2 + ca a in include/oi_occlusion.h's frame of the unit axis a; sa == 0 returns a itself
__device__ __forceinline__ void direction_about(float ax, float ay, float az, float sa, float ca, float u2, float& dx, float& dy,
                                                float& dz) {
  const float sg = copysignf(1.0f, az);
  const float A = -1.0f / (sg + az), B = ax * ay * A;
  const float t1x = 1.0f + sg * ax * ax * A, t1y = sg * B, t1z = -sg * ax;
  const float t2x = B, t2y = sg + ay * ay * A, t2z = -ay;
  float sp, cp;
  sincospif(2.0f * u2, &sp, &cp);  // phi = 2 pi u2
  const float e1 = sa * cp, e2 = sa * sp;
  dx = e1 * t1x + e2 * t2x + ca * ax;
  dy = e1 * t1y + e2 * t2y + ca * ay;
  dz = e1 * t1z + e2 * t2z + ca * az;
  if (sa == 0.f) dx = ax, dy = ay, dz = az;  // (the sums above give a up to the sign of a zero)
}

constexpr float HALF_PI = 1.57079632679489662f;

// Sample j of S at the pixel `pix` of a point with the unit normal n (include/oi_occlusion.h): AMBIENT = false: uniform in
// solid angle over the cap of angular radius radius[l] (clamped) about light lt's direction in the frame w2b; AMBIENT =
// true: cosine-weighted over the hemisphere about n (lt, radius, w2b are not read).  -> the direction; traced: n . d > 0.
// occlusion.hip's begin kernel and scene_light.hip's draw their directions here.
template <bool AMBIENT>
__device__ __forceinline__ bool occlusion_direction(float nx, float ny, float nz, unsigned pix, unsigned seed, unsigned j, int S,
                                                    const float* __restrict__ lt, const float* __restrict__ radius, long long l,
                                                    const float* __restrict__ w2b, float& dx, float& dy, float& dz) {
  float u1, u2;
  sample_numbers(pix, seed, j, S, u1, u2);
  float ax, ay, az, sa, ca;
  if (AMBIENT) {
    ax = nx, ay = ny, az = nz;
    ca = sqrtf(1.0f - u1);
    sa = sqrtf(u1);
  } else {
    light_dir(lt, w2b, ax, ay, az);
    const float rad = fminf(fmaxf(radius[l], 0.f), HALF_PI);  // (fmaxf drops a NaN)
    const float m = u1 * (1.0f - cosf(rad));
    ca = 1.0f - m;
    sa = sqrtf(fmaxf(m * (2.0f - m), 0.f));  // sqrt(1 - ca^2) without the cancellation
  }
  direction_about(ax, ay, az, sa, ca, u2, dx, dy, dz);
  return nx * dx + ny * dy + nz * dz > 0.f;
}

// Sample j of S at the pixel `pix` of the reflection lobe about the unit axis a (include/oi_envgloss.h): the polar angle has
// density proportional to cos^s(alpha), cos(alpha) = u1^(1 / (s + 1)) evaluated as expf(logf(u1) inv_s1) with inv_s1 = 1 / (s + 1),
// sin(alpha) = sqrt(-expm1f(2 logf(u1) inv_s1)) (1 - cos^2 without the cancellation).  -> the direction; traced: n . d > 0.
// envgloss.hip's begin kernel and the scene's lobe rays (scene_gloss.hip) draw their directions here.
__device__ __forceinline__ bool lobe_direction(const float* n, const float* a, unsigned pix, unsigned seed, unsigned j, int S,
                                               float inv_s1, float& dx, float& dy, float& dz) {
  float u1, u2;
  sample_numbers(pix, seed, j, S, u1, u2);
  const float e = logf(u1) * inv_s1;  // log(cos alpha)
  const float ca = expf(e), sa = sqrtf(fmaxf(-expm1f(2.0f * e), 0.f));
  direction_about(a[0], a[1], a[2], sa, ca, u2, dx, dy, dz);
  return n[0] * dx + n[1] * dy + n[2] * dz > 0.f;
}

// include/oi_envlight.h's basis of a unit vector
__device__ __forceinline__ void sh9(float x, float y, float z, float* __restrict__ o) {
  o[0] = 0.28209479177387814f;
  o[1] = 0.4886025119029199f * y;
  o[2] = 0.4886025119029199f * z;
  o[3] = 0.4886025119029199f * x;
  o[4] = 1.0925484305920792f * (x * y);
  o[5] = 1.0925484305920792f * (y * z);
  o[6] = 0.31539156525252005f * (3.0f * (z * z) - 1.0f);
  o[7] = 1.0925484305920792f * (x * z);
  o[8] = 0.5462742152960396f * (x * x - y * y);
}

// v = w2b[:3,:3]^T d: a box-frame direction in the world (scene_light.hip's rotate_t is this with contraction off)
__device__ __forceinline__ void to_world(const float* __restrict__ Wb, float dx, float dy, float dz, float& x, float& y, float& z) {
  x = Wb[0] * dx + Wb[4] * dy + Wb[8] * dz;
  y = Wb[1] * dx + Wb[5] * dy + Wb[9] * dz;
  z = Wb[2] * dx + Wb[6] * dy + Wb[10] * dz;
}

// the unit normal of gradient row k
__device__ __forceinline__ void unit_normal(const float* __restrict__ grad, long long k, float& nx, float& ny, float& nz) {
  unit_normal(grad[k * 3 + 0], grad[k * 3 + 1], grad[k * 3 + 2], nx, ny, nz);
}

// n = the unit normal of hit k, v = its unit view vector from `eye`, r = 2 ((n . v) n) - v
__device__ __forceinline__ void reflect_view(const float* __restrict__ grad, const float* __restrict__ hit_points, long long k,
                                             const float* __restrict__ eye, float* n, float* r) {
  unit_normal(grad, k, n[0], n[1], n[2]);
  float vx, vy, vz;
  unit_view(eye[0], eye[1], eye[2], hit_points[k * 3 + 0], hit_points[k * 3 + 1], hit_points[k * 3 + 2], vx, vy, vz);
  const float ndv = n[0] * vx + n[1] * vy + n[2] * vz;
  r[0] = 2.0f * (ndv * n[0]) - vx, r[1] = 2.0f * (ndv * n[1]) - vy, r[2] = 2.0f * (ndv * n[2]) - vz;
}

// The unshadowed transfer of a point with the unit normal n in the frame w2b (include/oi_envlight.h's closed form):
// t[c] = A_band y_c(world normal), the clamped cosine's A = 1, 2/3, 1/4 for the bands 0, 1, 2
__device__ __forceinline__ void normal_transfer(const float* __restrict__ Wb, float nx, float ny, float nz, float* __restrict__ t) {
  float x, y, z;
  to_world(Wb, nx, ny, nz, x, y, z);
  sh9(x, y, z, t);
#pragma unroll
  for (int c = 1; c < 4; ++c) t[c] *= 2.0f / 3.0f;
#pragma unroll
  for (int c = 4; c < 9; ++c) t[c] *= 0.25f;
}

// oi_trace_shadow_begin's ray of hit i under the light lt: n = the unit normal, l = the light's direction in the object
// frame; origin = point + bias n, direction = l, far = the exit of the unit sphere; traced: n . l > 0.
struct ShadowRay {
  float o[3], l[3], far_;
  bool traced;
};
__device__ __forceinline__ ShadowRay shadow_ray(const float* __restrict__ hit_points, const float* __restrict__ grad, long long i,
                                                const float* __restrict__ lt, const float* __restrict__ w2b, float bias) {
  ShadowRay r;
  light_dir(lt, w2b, r.l[0], r.l[1], r.l[2]);
  float nx, ny, nz;
  unit_normal(grad, i, nx, ny, nz);
  r.traced = nx * r.l[0] + ny * r.l[1] + nz * r.l[2] > 0.f;
  offset_origin(hit_points + i * 3, bias, nx, ny, nz, r.o[0], r.o[1], r.o[2]);
  r.far_ = unit_sphere_exit(r.o[0], r.o[1], r.o[2], r.l[0], r.l[1], r.l[2]);
  return r;
}

// Value i of the (L, N) map of oi_occlusion_resolve: the share of pixel i % N's S rays under light i / N that ended MISS, 1
// off the surface.  oi_trace_visibility's map is this at S = 1.
__device__ __forceinline__ void lit_share(const uint8_t* __restrict__ status, const int* __restrict__ hit_slot, long long N,
                                          long long n_hit, int L, int S, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= N * L) return;
  const long long l = i / N, px = i - l * N;
  const int slot = hit_slot[px];
  if (slot < 0) {
    out[i] = 1.0f;
    return;
  }
  const uint8_t* __restrict__ st = status + l * S * n_hit + slot;
  int lit = 0;
  for (int j = 0; j < S; ++j) lit += st[(long long)j * n_hit] == OI_TRACE_MISS ? 1 : 0;
  out[i] = (float)lit / (float)S;
}

// One pixel of the G-buffer and of the Phong image.  P: oi_surface_params or a struct with the same fields; ao: ambient occlusion
// per output pixel (read at q) or nullptr (the ambient term as it is).  The inputs are read at ray r of p (only where `hit`), the outputs
// written at pixel q of planes of M pixels (p.visibility is read there too): r == q and M == p.N for a single view; a scene
// (scene.hip) reads the owner's ray and writes the scene's pixel.
template <class P>
__device__ __forceinline__ void surface_shade_at(const P& p, const float* __restrict__ ao, long long r, bool hit, long long q,
                                                 long long M) {
  const float b3[3] = {p.bg ? p.bg[0] : 0.f, p.bg ? p.bg[1] : 0.f, p.bg ? p.bg[2] : 0.f};
  float pos[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f}, nw[3] = {0.f, 0.f, 0.f}, alb[3] = {0.f, 0.f, 0.f};
  float vx = 0.f, vy = 0.f, vz = 0.f;
  const float* Wb = p.w2b;
  if (hit) {
    const long long k = p.hit_slot[r];
    unit_normal(p.grad, k, n[0], n[1], n[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[a] = p.hit_points[k * 3 + a], alb[a] = p.rgb[k * 3 + a];
    to_world(Wb, n[0], n[1], n[2], nw[0], nw[1], nw[2]);
    unit_view(p.rays_o[r * 3 + 0], p.rays_o[r * 3 + 1], p.rays_o[r * 3 + 2], pos[0], pos[1], pos[2], vx, vy, vz);
  }
  if (p.depth) p.depth[q] = hit ? p.t[r] : __uint_as_float(0x7fc00000u);
  if (p.mask) p.mask[q] = hit ? 1.0f : 0.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (p.position) p.position[q * 3 + a] = pos[a];
    if (p.normal) p.normal[q * 3 + a] = n[a];
    if (p.normal_world) p.normal_world[q * 3 + a] = nw[a];
    if (p.albedo) p.albedo[q * 3 + a] = alb[a];
  }
  if (!p.image) return;
  const bool occluded = ao != nullptr;
  const float aov = occluded && hit ? ao[q] : 1.0f;
  for (int l = 0; l < p.L; ++l) {
    float* img = p.image + (long long)l * 3 * M + q;
    if (!hit) {
      img[0] = b3[0], img[M] = b3[1], img[2 * M] = b3[2];
      continue;
    }
    const float* lt = p.lights + (long long)l * OI_RELIGHT_LIGHT_FLOATS;
    float lx, ly, lz;
    light_dir(lt, Wb, lx, ly, lz);
    const PhongGeometry ph = phong_geometry(n[0], n[1], n[2], lx, ly, lz, vx, vy, vz);
    const float rl = fmaxf(ph.ndl, 0.f);
    const float pw = powf(ph.al, lt[15]);
    const bool shadowed = p.visibility != nullptr;
    const float vis = shadowed ? p.visibility[(long long)l * M + q] : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float diff = lt[8 + c] * rl, spec = lt[12 + c] * pw;
      if (shadowed) diff *= vis, spec *= vis;
      // (a product rounded on its own: the sum below contracts with the diffuse term whether or not ao is given)
      const float amb = occluded ? __fmul_rn(aov, lt[4 + c]) : lt[4 + c];
      const float shade = amb + diff;
      img[c * M] = shade * alb[c] + spec;
    }
  }
}

template <class P>
__device__ __forceinline__ void surface_shade_pixel(const P& p, const float* __restrict__ ao) {
  const long long r = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (r >= p.N) return;
  surface_shade_at(p, ao, r, p.status[r] == OI_TRACE_HIT, r, p.N);
}

// ---- local lights (include/oi_local_light.h) ----

// q = w2b (position, 1): local light lt in the box frame Wb, and its radius R (NaN / negative -> 0: fmaxf drops a NaN)
__device__ __forceinline__ void local_light_position(const float* __restrict__ lt, const float* __restrict__ Wb, float* q, float& R) {
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = Wb[a * 4 + 0] * lt[0] + Wb[a * 4 + 1] * lt[1] + Wb[a * 4 + 2] * lt[2] + Wb[a * 4 + 3];
  R = fmaxf(lt[3], 0.f);
}

// Shadow sample j of S from the origin o (normal n, key pix) towards the sphere of radius R about q, all in one frame
// (include/oi_local_light.h): uniform in solid angle over the cone the sphere subtends at o.  -> kind; AIMED_TRACED: the unit
// direction d and t_light, where the ray meets the sphere (R == 0: d = (q - o) / |q - o| bit for bit, t_light = |q - o|).
// AIMED_BACKFACING holds d too; AIMED_INSIDE (|q - o| <= R) leaves d at three zeros.
enum AimedKind { AIMED_TRACED, AIMED_INSIDE, AIMED_BACKFACING };
struct AimedSample {
  float d[3], t_light;
  AimedKind kind;
};
__device__ __forceinline__ AimedSample aimed_sample(const float* o, const float* n, const float* q, float R, unsigned pix,
                                                    unsigned seed, unsigned j, int S) {
  AimedSample a;
  a.d[0] = a.d[1] = a.d[2] = 0.f;
  a.t_light = 0.f;
  const float wx = q[0] - o[0], wy = q[1] - o[1], wz = q[2] - o[2];
  const float dc = sqrtf(wx * wx + wy * wy + wz * wz);
  if (dc <= R) {
    a.kind = AIMED_INSIDE;
    return a;
  }
  const float ax = wx / dc, ay = wy / dc, az = wz / dc;
  const float sin_max = R / dc, cos_max = sqrtf((1.0f - sin_max) * (1.0f + sin_max));
  float u1, u2;
  sample_numbers(pix, seed, j, S, u1, u2);
  const float m = u1 * (1.0f - cos_max);
  const float ca = 1.0f - m, sa = sqrtf(fmaxf(m * (2.0f - m), 0.f));
  direction_about(ax, ay, az, sa, ca, u2, a.d[0], a.d[1], a.d[2]);
  const float ds = dc * sa;
  a.t_light = dc * ca - sqrtf(fmaxf(R * R - ds * ds, 0.f));
  a.kind = n[0] * a.d[0] + n[1] * a.d[1] + n[2] * a.d[2] > 0.f ? AIMED_TRACED : AIMED_BACKFACING;
  return a;
}

// Local light lt seen from the point pos in the box frame Wb (include/oi_local_light.h's shading): -> att spot, and the unit
// direction l = u / max(|u|, 1e-6) towards the light (the view vector's clamped quotient).  local_shade_at's and the ground
// plane's (ground.hip, with the identity for Wb: the world frame).
__device__ __forceinline__ float local_light_factor(const float* __restrict__ lt, const float* __restrict__ Wb, const float* pos,
                                                    float& lx, float& ly, float& lz) {
  float lq[3], R;
  local_light_position(lt, Wb, lq, R);
  const float ux = lq[0] - pos[0], uy = lq[1] - pos[1], uz = lq[2] - pos[2];
  const float dist2 = ux * ux + uy * uy + uz * uz;
  unit_view(lq[0], lq[1], lq[2], pos[0], pos[1], pos[2], lx, ly, lz);
  const float rmin = fmaxf(R, OI_LOCAL_LIGHT_MIN_DISTANCE);
  float k = lt[7] * lt[7] / fmaxf(dist2, rmin * rmin);
  float spot = 1.0f;
  if (lt[11] > -1.0f) {
    const float a0 = lt[16], a1 = lt[17], a2 = lt[18];
    const float an = sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
    const float cx = Wb[0] * (a0 / an) + Wb[1] * (a1 / an) + Wb[2] * (a2 / an);
    const float cy = Wb[4] * (a0 / an) + Wb[5] * (a1 / an) + Wb[6] * (a2 / an);
    const float cz = Wb[8] * (a0 / an) + Wb[9] * (a1 / an) + Wb[10] * (a2 / an);
    const float c = -(lx * cx + ly * cy + lz * cz);
    const float tt = fminf(fmaxf((c - lt[11]) / (lt[19] - lt[11]), 0.f), 1.0f);
    spot = tt * tt * (3.0f - 2.0f * tt);
  }
  k *= spot;
  return k;
}

// One pixel of the Phong image under local lights (include/oi_local_light.h's shading), surface_shade_at's arguments with
// p.lights pointing at local records.  The G-buffer is not written here: the caller runs surface_shade_at without an image
// for it, so those outputs are oi_surface_shade's bytes.
template <class P>
__device__ __forceinline__ void local_shade_at(const P& p, const float* __restrict__ ao, long long r, bool hit, long long q,
                                               long long M) {
  if (!p.image) return;
  const float b3[3] = {p.bg ? p.bg[0] : 0.f, p.bg ? p.bg[1] : 0.f, p.bg ? p.bg[2] : 0.f};
  float pos[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f}, alb[3] = {0.f, 0.f, 0.f};
  float vx = 0.f, vy = 0.f, vz = 0.f;
  const float* Wb = p.w2b;
  if (hit) {
    const long long k = p.hit_slot[r];
    unit_normal(p.grad, k, n[0], n[1], n[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) pos[a] = p.hit_points[k * 3 + a], alb[a] = p.rgb[k * 3 + a];
    unit_view(p.rays_o[r * 3 + 0], p.rays_o[r * 3 + 1], p.rays_o[r * 3 + 2], pos[0], pos[1], pos[2], vx, vy, vz);
  }
  const bool occluded = ao != nullptr;
  const float aov = occluded && hit ? ao[q] : 1.0f;
  for (int l = 0; l < p.L; ++l) {
    float* img = p.image + (long long)l * 3 * M + q;
    if (!hit) {
      img[0] = b3[0], img[M] = b3[1], img[2 * M] = b3[2];
      continue;
    }
    const float* lt = p.lights + (long long)l * OI_LOCAL_LIGHT_FLOATS;
    float lx, ly, lz;
    float k = local_light_factor(lt, Wb, pos, lx, ly, lz);
    if (p.visibility != nullptr) k *= p.visibility[(long long)l * M + q];
    const PhongGeometry ph = phong_geometry(n[0], n[1], n[2], lx, ly, lz, vx, vy, vz);
    const float rl = fmaxf(ph.ndl, 0.f) * k;
    const float pw = powf(ph.al, lt[15]) * k;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float diff = lt[8 + c] * rl, spec = lt[12 + c] * pw;
      const float amb = occluded ? __fmul_rn(aov, lt[4 + c]) : lt[4 + c];
      const float shade = amb + diff;
      img[c * M] = shade * alb[c] + spec;
    }
  }
}

// surface_shade_at with local lights: its G-buffer (the same body, run without an image) and local_shade_at's image
template <class P>
__device__ __forceinline__ void surface_shade_local_at(const P& p, const float* __restrict__ ao, long long r, bool hit, long long q,
                                                       long long M) {
  P g = p;
  g.image = nullptr;
  surface_shade_at(g, nullptr, r, hit, q, M);
  local_shade_at(p, ao, r, hit, q, M);
}

// The secondary ray of hit i (pixel key hit_index[i]) under light l, sample j of S: what the begin kernels of trace.hip,
// occlusion.hip, local_light.hip and occlusion_batch.hip write with write_ray and enter with enter_rays.  One function per kind,
// NOT inlined: it is compiled on its own, so the single-view kernels and the batched kernels (include/oi_occlusion_batch.h)
// run the same instructions and a ray is the same bits whichever of them writes it -- inlined, the compiler contracts and packs
// these sums differently from kernel to kernel.  Everything is returned in registers: no memory.
enum BeginKind { BEGIN_SHADOW = 0, BEGIN_CAP = 1, BEGIN_HEMISPHERE = 2, BEGIN_LOCAL = 3 };
struct BeginRay {
  float o[3], d[3], far_;
  unsigned status;
  bool entered;
};
template <int KIND>
__device__ __noinline__ BeginRay begin_ray(const float* __restrict__ hit_points, const float* __restrict__ grad,
                                           const int* __restrict__ hit_index, long long i, long long l, unsigned j, int S,
                                           const float* __restrict__ lights, const float* __restrict__ radius,
                                           const float* __restrict__ w2b, float bias, float distance, unsigned seed) {
  BeginRay r;
  if constexpr (KIND == BEGIN_SHADOW) {
    const ShadowRay ry = shadow_ray(hit_points, grad, i, lights + l * OI_RELIGHT_LIGHT_FLOATS, w2b, bias);
#pragma unroll
    for (int a = 0; a < 3; ++a) r.o[a] = ry.o[a], r.d[a] = ry.l[a];
    r.far_ = ry.far_;
    r.entered = ry.traced;
    r.status = ry.traced ? OI_TRACE_MARCH : OI_TRACE_BACKFACING;
  } else if constexpr (KIND == BEGIN_LOCAL) {
    float n[3], lq[3], R;
    unit_normal(grad, i, n[0], n[1], n[2]);
    offset_origin(hit_points + i * 3, bias, n[0], n[1], n[2], r.o[0], r.o[1], r.o[2]);
    local_light_position(lights + l * OI_LOCAL_LIGHT_FLOATS, w2b, lq, R);
    const AimedSample a = aimed_sample(r.o, n, lq, R, (unsigned)hit_index[i], seed, j, S);
    r.entered = a.kind == AIMED_TRACED;
    r.d[0] = a.d[0], r.d[1] = a.d[1], r.d[2] = a.d[2];
    r.far_ = r.entered ? fminf(a.t_light, unit_sphere_exit(r.o[0], r.o[1], r.o[2], a.d[0], a.d[1], a.d[2])) : 0.f;
    r.status = r.entered ? OI_TRACE_MARCH : a.kind == AIMED_INSIDE ? OI_TRACE_MISS : OI_TRACE_BACKFACING;
  } else {
    constexpr bool AMBIENT = KIND == BEGIN_HEMISPHERE;
    float nx, ny, nz;
    unit_normal(grad, i, nx, ny, nz);
    r.entered = occlusion_direction<AMBIENT>(nx, ny, nz, (unsigned)hit_index[i], seed, j, S, lights + l * OI_RELIGHT_LIGHT_FLOATS, radius,
                                             l, w2b, r.d[0], r.d[1], r.d[2]);
    offset_origin(hit_points + i * 3, bias, nx, ny, nz, r.o[0], r.o[1], r.o[2]);
    r.far_ = unit_sphere_exit(r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2]);
    if (AMBIENT) r.far_ = fminf(r.far_, distance);
    r.status = r.entered ? OI_TRACE_MARCH : OI_TRACE_BACKFACING;
  }
  return r;
}

inline unsigned n_blocks(long long n) { return (unsigned)((n + TR_THREADS - 1) / TR_THREADS); }

// a check's refusal is the entry's
#define OI_TRY(call)                  \
  do {                                \
    const int rc_ = (call);           \
    if (rc_ != OI_OK) return rc_;     \
  } while (0)

// The conditions several entries refuse in the same words; `what` is the entry's name.
inline int check_lights(const char* what, int L) {
  OI_REQUIRE(L >= 1 && L <= OI_RELIGHT_MAX_LIGHTS, "%s: L=%d (1 .. %d lights)", what, L, OI_RELIGHT_MAX_LIGHTS);
  return OI_OK;
}
inline int check_samples(const char* what, int S) {
  OI_REQUIRE(S >= 1 && S <= OI_OCCLUSION_MAX_SAMPLES, "%s: S=%d (1 .. %d samples)", what, S, OI_OCCLUSION_MAX_SAMPLES);
  return OI_OK;
}
inline int check_bias(const char* what, float bias) {
  OI_REQUIRE(bias >= 0.f && bias < INFINITY, "%s: bias %g (>= 0, finite)", what, (double)bias);
  return OI_OK;
}
inline int check_pixels(const char* what, long long N, long long n_hit) {
  OI_REQUIRE(N >= 1 && N < (1ll << 31) && n_hit >= 0 && n_hit <= N, "%s: N=%lld, n_hit=%lld", what, N, n_hit);
  return OI_OK;
}
inline int check_elements(const char* what, int E) {
  OI_REQUIRE(E >= 1 && E <= OI_TRACE_BATCH_MAX_ELEMS, "%s: E=%d elements (1 .. %d)", what, E, OI_TRACE_BATCH_MAX_ELEMS);
  return OI_OK;
}
// a scene's elements and rays per element as plain numbers
inline int check_scene_rays(const char* what, int E, long long N) {
  OI_TRY(check_elements(what, E));
  OI_REQUIRE(N >= 1 && E * N < (1ll << 31), "%s: E=%d x N=%lld rays (N >= 1, E * N < 2^31)", what, E, N);
  return OI_OK;
}

inline int check_state(const oi_trace_state* s, const char* what) {
  OI_REQUIRE(s != nullptr, "%s: null state", what);
  OI_REQUIRE(s->N >= 1 && s->N < (1ll << 31), "%s: N=%lld rays (1 <= N < 2^31)", what, s->N);
  OI_REQUIRE(s->rays_o && s->rays_d && s->near_ && s->far_ && s->t && s->status && s->steps && s->bracket && s->side &&
                 s->active && s->points && s->counts,
             "%s: null pointer in the state", what);
  return OI_OK;
}

inline int check_batch(const oi_trace_batch* b, const char* what) {
  OI_REQUIRE(b != nullptr, "%s: null batch", what);
  OI_TRY(check_elements(what, b->E));
  OI_TRY(check_state(&b->s, what));
  OI_REQUIRE((long long)b->E * b->s.N < (1ll << 31), "%s: E=%d x N=%lld rays (E * N < 2^31)", what, b->E, b->s.N);
  OI_REQUIRE(b->live != nullptr, "%s: null live", what);
  return OI_OK;
}

// Arguments of oi_trace_step and oi_occlusion_step, then the launch.
template <bool ANYHIT>
inline int launch_step(const char* what, const oi_trace_state* s, const float* sdf, long long bound, int k, float tol,
                       float omega, oi_stream_t stream) {
  OI_TRY(check_state(s, what));
  OI_REQUIRE(k >= 0 && k < OI_TRACE_MAX_STEPS, "%s: step k=%d (0 <= k < %d)", what, k, OI_TRACE_MAX_STEPS);
  OI_REQUIRE(bound >= 0 && bound <= s->N, "%s: bound=%lld (0 <= bound <= N=%lld)", what, bound, s->N);
  OI_REQUIRE(tol > 0.f && omega > 0.f && tol < INFINITY && omega < INFINITY, "%s: tol %g, omega %g (both > 0, finite)", what,
             (double)tol, (double)omega);
  if (bound == 0) return OI_OK;
  OI_REQUIRE(sdf != nullptr, "%s: null sdf", what);
  hipLaunchKernelGGL(trace_step_kernel<ANYHIT>, dim3(n_blocks(bound)), dim3(TR_THREADS), 0, oi::as_stream(stream), *s, sdf, bound,
                     k, tol, omega);
  return oi::check_launch(what);
}

// The counters cleared, then a begin kernel on one thread per ray of s: the two launches of every single-view secondary begin.
template <class K, class... A>
inline int launch_begin(const char* what, const oi_trace_state* s, oi_stream_t stream, K kernel, A... args) {
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(trace_clear_counts_kernel, dim3(1), dim3(TR_THREADS), 0, st, s->counts);
  hipLaunchKernelGGL(kernel, dim3(n_blocks(s->N)), dim3(TR_THREADS), 0, st, *s, args...);
  return oi::check_launch(what);
}

// Arguments of oi_surface_shade and oi_surface_shade_ao (P: oi_surface_params or a struct with the same fields).
template <class P>
inline int check_surface(const char* what, const P* p) {
  OI_REQUIRE(p != nullptr, "%s: null params", what);
  OI_TRY(check_pixels(what, p->N, p->n_hit));
  OI_REQUIRE(p->image ? (p->L >= 1 && p->L <= OI_RELIGHT_MAX_LIGHTS && p->lights) : p->L >= 0,
             "%s: L=%d (1 .. %d lights with an image)", what, p->L, OI_RELIGHT_MAX_LIGHTS);
  OI_REQUIRE(p->rays_o && p->rays_d && p->t && p->status && p->hit_slot && p->w2b, "%s: null input pointer", what);
  OI_REQUIRE(p->n_hit == 0 || (p->hit_points && p->grad && p->rgb), "%s: null hit arrays with n_hit=%lld", what, p->n_hit);
  return OI_OK;
}

}  // namespace

#endif  // OI_TRACE_COMMON_H_
