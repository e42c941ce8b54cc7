// What scene.hip, scene_light.hip, scene_gloss.hip and scene_bounce.hip share (include/oi_scene.h, include/oi_scene_light.h,
// include/oi_scene_gloss.h, include/oi_scene_bounce.h; DESIGN sections 4.19, 4.21, 4.25 and 4.26): the unit sphere's chord, the
// rigid transform and its rotation, the begin of a sampled ray against every instance (one body for the cap, the hemisphere and
// the lobe), "missed every instance", the clearing of the hit words before a compaction into them, the per-pixel shading on the
// owner's slices and the checks of its arguments and of the resolves'; for local_light.hip (include/oi_local_light.h; DESIGN
// section 4.27) the begin of a ray aimed at a local light against every instance.  (What a begin kernel stores and the
// compaction of the entered rays are trace_common.h's write_ray and enter_rays.)  Internal linkage, as trace_common.h.
#ifndef OI_SCENE_COMMON_H_
#define OI_SCENE_COMMON_H_

#include "trace_common.h"

#include "../../include/oi_scene.h"
#include "../../include/oi_scene_light.h"

namespace {

// The unit sphere's chord on the ray (o, d): false when the ray passes at 1 or more from the centre or the sphere lies wholly
// behind the origin; otherwise near_ = max(mid - h, 0), far_ = mid + h.  Contraction off: tests/helpers/scene_ref.py restates
// these expressions.
__device__ __forceinline__ bool unit_sphere_chord(const float* o, const float* d, float& near_, float& far_) {
#pragma clang fp contract(off)
  const float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  const float od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2];
  const float mid = -od / dd;
  const float cx = o[0] + mid * d[0], cy = o[1] + mid * d[1], cz = o[2] + mid * d[2];
  const float c2 = cx * cx + cy * cy + cz * cz;
  if (!(c2 < 1.0f)) return false;
  const float h = sqrtf((1.0f - c2) / dd);
  far_ = mid + h;
  near_ = fmaxf(mid - h, 0.f);
  return far_ > 0.f;
}

// M (4x4, rigid) applied to the point v: three products and three sums per component, contraction off
__device__ __forceinline__ void transform_point(const float* __restrict__ M, const float* v, float* out) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 3; ++a) out[a] = M[a * 4 + 0] * v[0] + M[a * 4 + 1] * v[1] + M[a * 4 + 2] * v[2] + M[a * 4 + 3];
}

// every counter of every element and of live, and points = the coordinate origin: the slots behind an element's entered rays
// are input of the first MLP passes (the bound is the largest count of any element)
__global__ void __launch_bounds__(TR_THREADS) scene_clear_kernel(const oi_trace_state s, int* __restrict__ live) {
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int i = threadIdx.x; i < OI_TRACE_COUNT_WORDS; i += TR_THREADS) live[i] = 0;
  const oi_trace_state v = element_view(s, blockIdx.y);
  clear_counts(v.counts, 0);
  const long long r = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (r < s.N) v.points[r * 3 + 0] = v.points[r * 3 + 1] = v.points[r * 3 + 2] = 0.f;
}

// the hit words of every element and of live to 0, before a compaction into them (oi_scene_visible, oi_scene_bounce_visible):
// the body of a one-dimensional launch over the elements
__device__ __forceinline__ void clear_hit_words(int* __restrict__ counts, int* __restrict__ live, int E) {
  const int e = blockIdx.x * TR_THREADS + threadIdx.x;
  if (e < E) counts[(long long)e * OI_TRACE_COUNT_WORDS + N_HIT_WORD] = 0;
  if (e == 0) live[N_HIT_WORD] = 0;
}

// R (the rotation of the rigid 4 x 4 M) applied to v, contraction off: tests/helpers/scene_light_ref.py restates it
__device__ __forceinline__ void rotate(const float* __restrict__ M, const float* v, float* out) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 3; ++a) out[a] = M[a * 4 + 0] * v[0] + M[a * 4 + 1] * v[1] + M[a * 4 + 2] * v[2];
}

// ... and its transpose: w2b[:3,:3]^T v, a box-frame direction in the world.  trace_common.h's to_world is the same sum
// under the default contraction (fused multiply-adds); this one rounds every product, as scene_light_ref.py does, so the two
// stay apart.
__device__ __forceinline__ void rotate_t(const float* __restrict__ M, const float* v, float* out) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 3; ++a) out[a] = M[0 + a] * v[0] + M[4 + a] * v[1] + M[8 + a] * v[2];
}

// How a scene's sampled rays are drawn in the owner's frame: uniform over the cap about a light, cosine-weighted over the
// hemisphere about the normal (with a distance limit), or as cos^s about the reflected view vector (the hemisphere's cases
// without a limit).
enum class SceneSampler { CAP, HEMISPHERE, LOBE };

// what the LOBE sampler reads beside oi_scene_occlusion_params (oi_scene_lobe_begin's own arguments, include/oi_scene_gloss.h)
struct SceneLobe {
  const float* rays_o;   // [E][N][3] the primary batch's origins
  const int* vis_index;  // [E][N]
  long long N;
  float inv_s1;          // 1 / (shininess + 1)
};

// One ray of oi_scene_occlusion_begin (CAP, HEMISPHERE: scene_light.hip) and oi_scene_lobe_begin (LOBE: scene_gloss.hip): ray
// blockIdx.x * TR_THREADS + threadIdx.x of occluder element blockIdx.y.  The direction is drawn once in the owner's frame;
// the owner's ray starts at the biased point, any other instance's is moved into its box frame and culled against its unit
// sphere.  Every thread of the workgroup calls it; lds: TR_WAVES + 1 words.  g: read for LOBE only.
template <SceneSampler X>
__device__ __forceinline__ void scene_sampled_begin(const oi_trace_state& s, int* __restrict__ live,
                                                    const oi_scene_occlusion_params& p, const SceneLobe& g, unsigned* lds) {
  constexpr bool LIMITED = X == SceneSampler::HEMISPHERE;  // far and the cull honour p.distance
  const int eo = blockIdx.y;  // the occluder
  const oi_trace_state v = element_view(s, eo);
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool entered = false;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (q < s.N) {
    const long long lj = q / p.n_vis, gi = q - lj * p.n_vis;
    const long long l = lj / p.Sc;
    const unsigned j = (unsigned)p.j0 + (unsigned)(lj - l * p.Sc);
    const int e = p.elem[gi];  // the point's owner
    const long long slot = gi - p.offset[e], k = (long long)e * p.n_pad + slot;
    const float* We = p.w2b + (long long)e * 16;
    float n[3], d[3], o[3];
    bool traced;
    if constexpr (X == SceneSampler::LOBE) {
      float r[3];
      reflect_view(p.grad, p.hit_points, k, g.rays_o + ((long long)e * g.N + g.vis_index[(long long)e * g.N + slot]) * 3, n, r);
      traced = lobe_direction(n, r, (unsigned)p.pixel[gi], p.seed, j, p.S, g.inv_s1, d[0], d[1], d[2]);
    } else {
      unit_normal(p.grad, k, n[0], n[1], n[2]);
      traced = occlusion_direction<X == SceneSampler::HEMISPHERE>(n[0], n[1], n[2], (unsigned)p.pixel[gi], p.seed, j, p.S,
                                                                  p.lights + l * OI_RELIGHT_LIGHT_FLOATS, p.radius, l, We, d[0],
                                                                  d[1], d[2]);
    }
    offset_origin(p.hit_points + k * 3, p.bias, n[0], n[1], n[2], o[0], o[1], o[2]);
    float near_ = 0.f, far_ = 0.f;
    unsigned status = OI_TRACE_BACKFACING;
    if (traced && e == eo) {
      far_ = unit_sphere_exit(o[0], o[1], o[2], d[0], d[1], d[2]);
      if (LIMITED) far_ = fminf(far_, p.distance);
      entered = true;
      status = OI_TRACE_MARCH;
    } else if (traced) {
      const float* Wb = p.w2b + (long long)eo * 16;
      float ow[3], dw[3], dd[3];
      offset_origin(p.position + gi * 3, p.bias, p.normal[gi * 3 + 0], p.normal[gi * 3 + 1], p.normal[gi * 3 + 2], ow[0], ow[1], ow[2]);
      transform_point(Wb, ow, o);
      rotate_t(We, d, dw);
      rotate(Wb, dw, dd);
      d[0] = dd[0], d[1] = dd[1], d[2] = dd[2];
      entered = unit_sphere_chord(o, d, near_, far_);
      if (LIMITED) {
        entered = entered && near_ < p.distance;
        far_ = fminf(far_, p.distance);
      }
      status = entered ? OI_TRACE_MARCH : OI_TRACE_MISS;
    }
    if (!entered) near_ = far_ = 0.f;
    write_ray(v, q, o, d, near_, far_, status);
    px = __fmaf_rn(near_, d[0], o[0]), py = __fmaf_rn(near_, d[1], o[1]), pz = __fmaf_rn(near_, d[2], o[2]);
  }
  enter_rays(v, q, entered, px, py, pz, lds, live);
}

// One ray of oi_scene_local_light_begin (local_light.hip; include/oi_local_light.h): scene_sampled_begin's layout with the
// direction aimed at a local light (trace_common.h's aimed_sample, drawn once in the owner's frame, where the light's world
// position is moved) and every ray clipped to the light: the owner's far = min(t_light, the sphere's exit); another
// instance's chord is cut at t_light, the rule `distance` has for the hemisphere.
__device__ __forceinline__ void scene_local_begin(const oi_trace_state& s, int* __restrict__ live,
                                                  const oi_scene_occlusion_params& p, unsigned* lds) {
  const int eo = blockIdx.y;  // the occluder
  const oi_trace_state v = element_view(s, eo);
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool entered = false;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (q < s.N) {
    const long long lj = q / p.n_vis, gi = q - lj * p.n_vis;
    const long long l = lj / p.Sc;
    const unsigned j = (unsigned)p.j0 + (unsigned)(lj - l * p.Sc);
    const int e = p.elem[gi];  // the point's owner
    const long long slot = gi - p.offset[e], k = (long long)e * p.n_pad + slot;
    const float* We = p.w2b + (long long)e * 16;
    float n[3], o[3], lq[3], R;
    unit_normal(p.grad, k, n[0], n[1], n[2]);
    offset_origin(p.hit_points + k * 3, p.bias, n[0], n[1], n[2], o[0], o[1], o[2]);
    local_light_position(p.lights + l * OI_LOCAL_LIGHT_FLOATS, We, lq, R);
    const AimedSample a = aimed_sample(o, n, lq, R, (unsigned)p.pixel[gi], p.seed, j, p.S);
    float d[3] = {a.d[0], a.d[1], a.d[2]};
    float near_ = 0.f, far_ = 0.f;
    unsigned status = a.kind == AIMED_INSIDE ? OI_TRACE_MISS : OI_TRACE_BACKFACING;
    if (a.kind == AIMED_TRACED && e == eo) {
      far_ = fminf(a.t_light, unit_sphere_exit(o[0], o[1], o[2], d[0], d[1], d[2]));
      entered = true;
      status = OI_TRACE_MARCH;
    } else if (a.kind == AIMED_TRACED) {
      const float* Wb = p.w2b + (long long)eo * 16;
      float ow[3], dw[3], dd[3];
      offset_origin(p.position + gi * 3, p.bias, p.normal[gi * 3 + 0], p.normal[gi * 3 + 1], p.normal[gi * 3 + 2], ow[0], ow[1], ow[2]);
      transform_point(Wb, ow, o);
      rotate_t(We, d, dw);
      rotate(Wb, dw, dd);
      d[0] = dd[0], d[1] = dd[1], d[2] = dd[2];
      entered = unit_sphere_chord(o, d, near_, far_) && near_ < a.t_light;
      far_ = fminf(far_, a.t_light);
      status = entered ? OI_TRACE_MARCH : OI_TRACE_MISS;
    }
    if (!entered) near_ = far_ = 0.f;
    write_ray(v, q, o, d, near_, far_, status);
    px = __fmaf_rn(near_, d[0], o[0]), py = __fmaf_rn(near_, d[1], o[1]), pz = __fmaf_rn(near_, d[2], o[2]);
  }
  enter_rays(v, q, entered, px, py, pz, lds, live);
}

// did ray `ray` (of `rays` per element) end OI_TRACE_MISS in every element?  A fixed-order loop, no early exit.
__device__ __forceinline__ bool escaped_everywhere(const uint8_t* __restrict__ status, int E, long long rays, long long ray) {
  bool free_ = true;
  for (int eo = 0; eo < E; ++eo)
    if (status[(long long)eo * rays + ray] != OI_TRACE_MISS) free_ = false;
  return free_;
}

// oi_surface_params' fields for one element of the scene (surface_shade_at's P)
struct ElementSurface {
  int L;
  const float *rays_o, *rays_d, *t;
  const int* hit_slot;
  const float *hit_points, *grad, *rgb, *w2b, *lights, *bg, *visibility;
  float *depth, *position, *normal, *normal_world, *albedo, *mask, *image;
};

// One scene pixel of oi_scene_shade / oi_scene_shade_ao: trace_common.h's shading on the owner's slices.  ao: [S * S] or nullptr.
// LOCAL (oi_scene_shade_local): p.lights are local records, shaded by trace_common.h's surface_shade_local_at.
template <bool LOCAL = false>
__device__ __forceinline__ void scene_shade_pixel(const oi_scene_shade_params& p, const float* __restrict__ ao) {
  const long long M = (long long)p.S * p.S, N = (long long)p.W * p.W;
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= M) return;
  const int e = p.owner[q];
  const bool hit = e >= 0 && e < p.E && p.n_pad > 0;
  const long long eo = hit ? e : 0, r = hit ? p.owner_ray[q] : 0;
  ElementSurface v;
  v.L = p.L;
  v.rays_o = p.rays_o + eo * N * 3, v.rays_d = p.rays_d + eo * N * 3, v.t = p.t + eo * N;
  v.hit_slot = p.vis_slot + eo * N;
  v.hit_points = p.hit_points + eo * p.n_pad * 3, v.grad = p.grad + eo * p.n_pad * 3, v.rgb = p.rgb + eo * p.n_pad * 3;
  v.w2b = p.w2b + eo * 16, v.lights = p.lights, v.bg = p.bg, v.visibility = p.visibility;
  v.depth = p.depth, v.position = nullptr, v.normal = p.normal, v.normal_world = p.normal_world, v.albedo = p.albedo;
  v.mask = p.mask, v.image = p.image;
  if (p.instance) p.instance[q] = hit ? e : -1;
  if (p.position) {
    float w[3] = {0.f, 0.f, 0.f};
    if (hit) transform_point(p.b2w + eo * 16, v.hit_points + (long long)v.hit_slot[r] * 3, w);
    p.position[q * 3 + 0] = w[0], p.position[q * 3 + 1] = w[1], p.position[q * 3 + 2] = w[2];
  }
  if constexpr (LOCAL) surface_shade_local_at(v, ao, r, hit, q, M);
  else surface_shade_at(v, ao, r, hit, q, M);
}

// the scene's resolution; name: how the entry's message calls it ("S", or "scene S" where S counts samples)
inline int check_resolution(const char* what, const char* name, int S) {
  OI_REQUIRE(S >= 1 && S <= OI_SCENE_MAX_RESOLUTION, "%s: %s=%d (1 .. %d)", what, name, S, OI_SCENE_MAX_RESOLUTION);
  return OI_OK;
}

// the strata and the chunk of a sampled trace
inline int check_chunk(const char* what, int L, int S, int j0, int Sc) {
  OI_TRY(check_lights(what, L));
  OI_TRY(check_samples(what, S));
  OI_REQUIRE(j0 >= 0 && Sc >= 1 && j0 <= S - Sc, "%s: j0=%d, Sc=%d, S=%d (the chunk [j0, j0 + Sc) within [0, S), Sc >= 1)", what,
             j0, Sc, S);
  return OI_OK;
}

// what the resolves share: the scene's shape and the size of the chunk's trace
inline int check_resolve(const char* what, int E, long long N, int L, int Sc, long long n_vis, int scene_S) {
  OI_TRY(check_scene_rays(what, E, N));
  OI_TRY(check_resolution(what, "scene S", scene_S));
  OI_REQUIRE(n_vis >= 1 && n_vis <= E * N && (long long)E * L * Sc * n_vis < (1ll << 31),
             "%s: n_vis=%lld (1 <= n_vis <= E * N, E * L * Sc * n_vis < 2^31)", what, n_vis);
  return OI_OK;
}

// the layout of a sampled begin's rays (sb: a checked batch) and its bias
inline int check_sampled_rays(const char* what, const oi_trace_batch* sb, const oi_scene_occlusion_params* p) {
  OI_REQUIRE(p->n_pad >= 1 && p->n_vis >= 1 && p->n_vis <= sb->E * p->n_pad,
             "%s: n_pad=%lld, n_vis=%lld (n_pad >= 1, 1 <= n_vis <= E * n_pad)", what, p->n_pad, p->n_vis);
  OI_REQUIRE((long long)p->L * p->Sc * p->n_vis == sb->s.N, "%s: L=%d, Sc=%d, n_vis=%lld, N=%lld (N must be L * Sc * n_vis)", what,
             p->L, p->Sc, p->n_vis, sb->s.N);
  OI_TRY(check_bias(what, p->bias));
  return OI_OK;
}

// Arguments of oi_scene_shade and oi_scene_shade_ao.
inline int check_scene_shade(const oi_scene_shade_params* p, const char* what) {
  OI_REQUIRE(p != nullptr, "%s: null params", what);
  OI_TRY(check_elements(what, p->E));
  OI_REQUIRE(p->W >= 1 && (long long)p->E * p->W * p->W < (1ll << 31), "%s: E=%d, W=%d (W >= 1, E * W * W < 2^31)", what, p->E,
             p->W);
  OI_TRY(check_resolution(what, "S", p->S));
  OI_REQUIRE(p->n_pad >= 0 && p->n_pad <= (long long)p->W * p->W, "%s: n_pad=%lld (0 <= n_pad <= W * W = %lld)", what, p->n_pad,
             (long long)p->W * p->W);
  OI_REQUIRE(p->image ? (p->L >= 1 && p->L <= OI_RELIGHT_MAX_LIGHTS && p->lights) : p->L >= 0,
             "%s: L=%d (1 .. %d lights with an image)", what, p->L, OI_RELIGHT_MAX_LIGHTS);
  OI_REQUIRE(p->owner && p->owner_ray, "%s: null owner map", what);
  OI_REQUIRE(p->n_pad == 0 || (p->rays_o && p->rays_d && p->t && p->vis_slot && p->hit_points && p->grad && p->rgb &&
                               p->w2b && p->b2w),
             "%s: null input pointer with n_pad=%lld", what, p->n_pad);
  return OI_OK;
}

}  // namespace

#endif  // OI_SCENE_COMMON_H_
