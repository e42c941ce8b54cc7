// A ground plane in the world of a scene for gfx950 (include/oi_ground.h): a shadow catcher.  Small
// memory-bound kernels around the batched any-hit march, which is unchanged and dominates:
//   begin        one thread per scene pixel: the world ray (ray_common.h's make_ray on c2w), t_g, the classification against
//                the owner map, the ground pixels compacted (wg_slot: one integer atomicAdd per workgroup)
//   rays_begin   per occluder instance the secondary rays of the ground points: the direction drawn once in the WORLD frame
//                (trace_common.h's occlusion_direction / aimed_sample with the identity for the frame), moved into every
//                instance's box frame by scene_common.h's "e' != e" expressions, culled and clipped, stored through write_ray
//                and compacted through enter_rays
//   resolve      per (light, ground point) the samples that missed every instance (escaped_everywhere), as integers
//   shade        one thread per ground point: the Lambertian ground into the scene's maps, the mask and the shadow matte
//   occlude      one thread per ray of a finished chunk of the instances' rays: MISS -> HIT where the owner's ray meets the plane
// ground_point is the one place the point p = o + t_g d is formed.  No LDS beyond the compaction's counter words, no scratch.
#include "ray_common.h"
#include "scene_common.h"

#include "../../include/oi_ground.h"

namespace {

// the ground points of a scene as the kernels take them (include/oi_ground.h's shared arguments)
struct GroundPoints {
  int S;                    // the scene's resolution
  long long n_g;            // ground points
  const float *c2w, *kinv;  // [16], [9]
  const float* ground;      // [OI_GROUND_FLOATS]
  const float* ground_t;    // [S * S]
  const int* ground_index;  // [n_g]
};

// oi_ground_shade's arguments
struct GroundShade {
  GroundPoints g;
  int L;
  const float *lights, *visibility, *ambient_occlusion;
  float *image, *depth, *position, *normal_world, *albedo, *mask;
  int* instance;
  float *ground_mask, *shadow_matte;
};

// the frame of directions drawn in the world: light_dir and local_light_position with it return the world's own vectors
__device__ __forceinline__ void identity16(float* I) {
#pragma unroll
  for (int i = 0; i < 16; ++i) I[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

// the world ray of scene pixel q: what oi_scene_begin builds with c2b_e = w2b_e c2w
__device__ __forceinline__ RayOD ground_ray(const float* __restrict__ c2w, const float* __restrict__ kinv, int S, long long q) {
  const int Y = (int)(q / S), X = (int)(q - (long long)Y * S);
  return make_ray(c2w, kinv, 0.f, 0.f, S, X, Y);
}

// p = o + t d on the world ray of scene pixel q: the ground point, formed here and nowhere else
__device__ __forceinline__ void ground_point(const float* __restrict__ c2w, const float* __restrict__ kinv, int S, long long q,
                                             float t, float* p) {
  const RayOD r = ground_ray(c2w, kinv, S, q);
  p[0] = __fmaf_rn(t, r.d[0], r.o[0]);
  p[1] = __fmaf_rn(t, r.d[1], r.o[1]);
  p[2] = __fmaf_rn(t, r.d[2], r.o[2]);
}

// |p - c| <= R_g; contraction off: tests/helpers/ground_ref.py restates it
__device__ __forceinline__ bool within_extent(const float* __restrict__ gr, const float* p) {
#pragma clang fp contract(off)
  const float ux = p[0] - gr[8], uy = p[1] - gr[9], uz = p[2] - gr[10];
  return sqrtf(ux * ux + uy * uy + uz * uz) <= gr[7];
}

__global__ void __launch_bounds__(TR_THREADS) ground_clear_kernel(int* __restrict__ count) {
  if (threadIdx.x == 0) count[0] = 0;
}

__global__ void __launch_bounds__(TR_THREADS) ground_begin_kernel(const float* __restrict__ c2w, const float* __restrict__ kinv,
                                                                  int S, const float* __restrict__ gr,
                                                                  const int* __restrict__ owner,
                                                                  const int* __restrict__ owner_ray,
                                                                  const float* __restrict__ t, long long N, int E,
                                                                  float* __restrict__ ground_t, int* __restrict__ ground_index,
                                                                  int* __restrict__ count) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const long long M = (long long)S * S;
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool ground = false;
  float tg = 0.f;
  if (q < M) {
    const RayOD r = ground_ray(c2w, kinv, S, q);
    float nd, no;
    {
#pragma clang fp contract(off)
      nd = gr[0] * r.d[0] + gr[1] * r.d[1] + gr[2] * r.d[2];
      no = gr[0] * r.o[0] + gr[1] * r.o[1] + gr[2] * r.o[2];
      tg = (gr[3] - no) / nd;
    }
    if (nd < -1e-6f && tg > 0.f) {
      float p[3];
      ground_point(c2w, kinv, S, q, tg, p);
      ground = within_extent(gr, p);
      if (ground && owner != nullptr) {
        const int e = owner[q];
        const long long ray = owner_ray[q];
        if (e >= 0 && e < E && ray >= 0 && ray < N) ground = tg < t[(long long)e * N + ray];  // an equal depth: the instance's
      }
    }
    ground_t[q] = ground ? tg : __uint_as_float(0x7fc00000u);
  }
  const long long slot = wg_slot(ground, count, lds);
  if (ground) ground_index[slot] = (int)q;  // (slot < M: at most M pixels are kept)
}

// what a begin needs of one ground point's sample, drawn once in the world frame
struct GroundSample {
  float o[3], d[3], limit;  // origin p + bias n, unit direction, the far clip (INFINITY: none)
  unsigned status;          // OI_TRACE_MARCH: traced; otherwise the final status in every element
};

template <int MODE>
__device__ __forceinline__ GroundSample ground_sample(const GroundPoints& g, const oi_scene_occlusion_params& p, long long gi,
                                                      long long l, unsigned j) {
  GroundSample s;
  const float* gr = g.ground;
  const int pix = g.ground_index[gi];
  const float n[3] = {gr[0], gr[1], gr[2]};
  float pt[3], I[16];
  identity16(I);
  const bool inside = pix >= 0 && pix < (long long)g.S * g.S;  // (a list that is not this scene's: nothing is read outside)
  ground_point(g.c2w, g.kinv, g.S, inside ? pix : 0, g.ground_t[inside ? pix : 0], pt);
  offset_origin(pt, p.bias, n[0], n[1], n[2], s.o[0], s.o[1], s.o[2]);
  s.limit = INFINITY;
  s.d[0] = s.d[1] = s.d[2] = 0.f;
  bool traced;
  if constexpr (MODE == OI_GROUND_RAYS_LOCAL) {
    float lq[3], R;
    local_light_position(p.lights + l * OI_LOCAL_LIGHT_FLOATS, I, lq, R);
    const AimedSample a = aimed_sample(s.o, n, lq, R, (unsigned)pix, p.seed, j, p.S);
    s.d[0] = a.d[0], s.d[1] = a.d[1], s.d[2] = a.d[2];
    s.limit = a.t_light;
    traced = a.kind == AIMED_TRACED;
    s.status = traced ? OI_TRACE_MARCH : a.kind == AIMED_INSIDE ? OI_TRACE_MISS : OI_TRACE_BACKFACING;
  } else {
    traced = occlusion_direction<MODE == OI_GROUND_RAYS_HEMISPHERE>(n[0], n[1], n[2], (unsigned)pix, p.seed, j, p.S,
                                                                    p.lights + l * OI_RELIGHT_LIGHT_FLOATS, p.radius, l, I, s.d[0],
                                                                    s.d[1], s.d[2]);
    if (MODE == OI_GROUND_RAYS_HEMISPHERE) s.limit = p.distance;
    s.status = traced ? OI_TRACE_MARCH : OI_TRACE_BACKFACING;
  }
  return s;
}

template <int MODE>
__global__ void __launch_bounds__(TR_THREADS) ground_rays_begin_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                       const GroundPoints g, const oi_scene_occlusion_params p) {
  __shared__ unsigned lds[TR_WAVES + 1];
  constexpr bool LIMITED = MODE != OI_GROUND_RAYS_CAP;  // far and the cull honour the sample's limit
  const int eo = blockIdx.y;  // the occluder
  const oi_trace_state v = element_view(s, eo);
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool entered = false;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (q < s.N) {
    const long long lj = q / g.n_g, gi = q - lj * g.n_g;
    const long long l = lj / p.Sc;
    const unsigned j = (unsigned)p.j0 + (unsigned)(lj - l * p.Sc);
    const GroundSample a = ground_sample<MODE>(g, p, gi, l, j);
    const float* Wb = p.w2b + (long long)eo * 16;
    float o[3], d[3], near_ = 0.f, far_ = 0.f;
    transform_point(Wb, a.o, o);
    rotate(Wb, a.d, d);
    unsigned status = a.status;
    if (status == OI_TRACE_MARCH) {
      entered = unit_sphere_chord(o, d, near_, far_);
      if (LIMITED) {
        entered = entered && near_ < a.limit;
        far_ = fminf(far_, a.limit);
      }
      status = entered ? OI_TRACE_MARCH : OI_TRACE_MISS;
    }
    if (!entered) near_ = far_ = 0.f;
    write_ray(v, q, o, d, near_, far_, status);
    px = __fmaf_rn(near_, d[0], o[0]), py = __fmaf_rn(near_, d[1], o[1]), pz = __fmaf_rn(near_, d[2], o[2]);
  }
  enter_rays(v, q, entered, px, py, pz, lds, live);
}

__global__ void __launch_bounds__(TR_THREADS) ground_resolve_kernel(const uint8_t* __restrict__ status, int E, long long n_g, int L,
                                                                    int S, int j0, int Sc, int last, int* __restrict__ count,
                                                                    float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= n_g * L) return;
  const long long l = i / n_g, g = i - l * n_g;
  int c = j0 > 0 ? count[i] : 0;
  for (int jj = 0; jj < Sc; ++jj) c += escaped_everywhere(status, E, (long long)L * Sc * n_g, (l * Sc + jj) * n_g + g) ? 1 : 0;
  count[i] = c;
  if (last) out[i] = (float)c / (float)S;
}

template <bool LOCAL>
__global__ void __launch_bounds__(TR_THREADS) ground_shade_kernel(const GroundShade p) {
  const long long gi = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (gi >= p.g.n_g) return;
  const long long M = (long long)p.g.S * p.g.S;
  const long long q = p.g.ground_index[gi];
  if (q < 0 || q >= M) return;  // (a list that is not this scene's: nothing is written outside the maps)
  const float* gr = p.g.ground;
  const float tg = p.g.ground_t[q];
  const float n[3] = {gr[0], gr[1], gr[2]}, alb[3] = {gr[4], gr[5], gr[6]};
  float pt[3], I[16];
  identity16(I);
  ground_point(p.g.c2w, p.g.kinv, p.g.S, q, tg, pt);
  if (p.depth) p.depth[q] = tg;
  if (p.mask) p.mask[q] = 0.0f;
  if (p.instance) p.instance[q] = -1;
  if (p.ground_mask) p.ground_mask[q] = 1.0f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (p.position) p.position[q * 3 + a] = pt[a];
    if (p.normal_world) p.normal_world[q * 3 + a] = n[a];
    if (p.albedo) p.albedo[q * 3 + a] = alb[a];
  }
  if (!p.image && !p.shadow_matte) return;
  const float ao = p.ambient_occlusion ? p.ambient_occlusion[gi] : 1.0f;
  for (int l = 0; l < p.L; ++l) {
    const float* lt = p.lights + (long long)l * (LOCAL ? OI_LOCAL_LIGHT_FLOATS : OI_RELIGHT_LIGHT_FLOATS);
    float lx, ly, lz, k0 = 1.0f;
    if (LOCAL) k0 = local_light_factor(lt, I, pt, lx, ly, lz);
    else light_dir(lt, I, lx, ly, lz);
    const float vis = p.visibility ? p.visibility[(long long)l * p.g.n_g + gi] : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // every product and sum rounded on its own: tests/helpers/ground_ref.py's bar counts them
#pragma clang fp contract(off)
      const float rl = fmaxf(n[0] * lx + n[1] * ly + n[2] * lz, 0.f);
      const float dk = lt[8 + c] * rl * k0;
      const float value = (lt[4 + c] * ao + dk * vis) * alb[c];
      const float full = (lt[4 + c] + dk) * alb[c];
      if (p.image) p.image[((long long)l * 3 + c) * M + q] = value;
      if (p.shadow_matte) p.shadow_matte[((long long)l * 3 + c) * M + q] = full == 0.f ? 1.0f : value / full;
    }
  }
}

__global__ void __launch_bounds__(TR_THREADS) ground_occlude_kernel(const oi_trace_state s, int E, const float* __restrict__ gr,
                                                                    const int* __restrict__ elem, const float* __restrict__ b2w,
                                                                    long long n_vis, float limit) {
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= s.N) return;
  const int e = elem[q % n_vis];
  if (e < 0 || e >= E) return;  // (a list that is not this batch's: nothing is touched outside it)
  const long long r = (long long)e * s.N + q;
  if (s.status[r] != OI_TRACE_MISS) return;
  const float* Bw = b2w + (long long)e * 16;
  const float ob[3] = {s.rays_o[r * 3 + 0], s.rays_o[r * 3 + 1], s.rays_o[r * 3 + 2]};
  const float db[3] = {s.rays_d[r * 3 + 0], s.rays_d[r * 3 + 1], s.rays_d[r * 3 + 2]};
  float o[3], d[3];
  transform_point(Bw, ob, o);
  rotate(Bw, db, d);
  bool hit;
  {
#pragma clang fp contract(off)
    const float nd = gr[0] * d[0] + gr[1] * d[1] + gr[2] * d[2];
    const float no = gr[0] * o[0] + gr[1] * o[1] + gr[2] * o[2];
    const float t = (gr[3] - no) / nd;  // (nd == 0: inf or NaN, no hit)
    const float p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
    hit = t > 0.f && t < limit && within_extent(gr, p);
  }
  if (hit) s.status[r] = (uint8_t)OI_TRACE_HIT;
}

// the ground points' description: sizes and pointers
inline int check_ground(const char* what, const GroundPoints* g) {
  OI_TRY(check_resolution(what, "scene S", g->S));
  OI_REQUIRE(g->n_g >= 1 && g->n_g <= (long long)g->S * g->S, "%s: n_g=%lld ground points (1 .. S * S = %lld)", what, g->n_g,
             (long long)g->S * g->S);
  OI_REQUIRE(g->c2w && g->kinv && g->ground && g->ground_t && g->ground_index, "%s: null pointer among the ground's arguments", what);
  return OI_OK;
}

}  // namespace

extern "C" {

int oi_ground_begin(const float* c2w, const float* kinv, int S, const float* ground, const int* owner, const int* owner_ray,
                    const float* t, const int* window, int W, int E, float* ground_t, int* ground_index, int* count,
                    oi_stream_t stream) {
  const char* what = "oi_ground_begin";
  OI_TRY(check_resolution(what, "S", S));
  OI_TRY(check_elements(what, E));
  OI_REQUIRE(W >= 1 && (long long)E * W * W < (1ll << 31), "%s: E=%d, W=%d (W >= 1, E * W * W < 2^31)", what, E, W);
  OI_REQUIRE(c2w && kinv && ground && ground_t && ground_index && count, "%s: null pointer", what);
  OI_REQUIRE(owner == nullptr || (owner_ray && t && window), "%s: null owner_ray, t or window with an owner map", what);
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(ground_clear_kernel, dim3(1), dim3(TR_THREADS), 0, st, count);
  hipLaunchKernelGGL(ground_begin_kernel, dim3(n_blocks((long long)S * S)), dim3(TR_THREADS), 0, st, c2w, kinv, S, ground, owner,
                     owner_ray, t, (long long)W * W, E, ground_t, ground_index, count);
  return oi::check_launch(what);
}

int oi_ground_rays_begin(const oi_trace_batch* sb, const oi_scene_occlusion_params* p, int mode, const float* c2w,
                         const float* kinv, int scene_S, const float* ground, const float* ground_t, oi_stream_t stream) {
  const char* what = "oi_ground_rays_begin";
  OI_TRY(check_batch(sb, what));
  OI_REQUIRE(p != nullptr, "%s: null params", what);
  const GroundPoints g{scene_S, p->n_vis, c2w, kinv, ground, ground_t, p->pixel};
  OI_TRY(check_ground(what, &g));
  OI_TRY(check_chunk(what, p->L, p->S, p->j0, p->Sc));
  OI_REQUIRE(mode == OI_GROUND_RAYS_CAP || mode == OI_GROUND_RAYS_HEMISPHERE || mode == OI_GROUND_RAYS_LOCAL,
             "%s: mode=%d (0: caps, 1: the hemisphere, 2: local lights)", what, mode);
  const bool hemi = mode == OI_GROUND_RAYS_HEMISPHERE;
  OI_REQUIRE(hemi == (p->ambient != 0), "%s: ambient=%d with mode=%d (ambient != 0 exactly for the hemisphere)", what, p->ambient, mode);
  OI_REQUIRE(!hemi || p->L == 1, "%s: L=%d with the hemisphere (one set of rays: L must be 1)", what, p->L);
  OI_REQUIRE((long long)p->L * p->Sc * g.n_g == sb->s.N, "%s: L=%d, Sc=%d, n_g=%lld, N=%lld (N must be L * Sc * n_g)", what, p->L,
             p->Sc, g.n_g, sb->s.N);
  OI_TRY(check_bias(what, p->bias));
  OI_REQUIRE(!hemi || p->distance > 0.f, "%s: distance %g (> 0; INFINITY is allowed)", what, (double)p->distance);
  OI_REQUIRE(p->w2b && (hemi || p->lights) && (mode != OI_GROUND_RAYS_CAP || p->radius), "%s: null input pointer", what);
  const hipStream_t st = oi::as_stream(stream);
  const dim3 grid(n_blocks(sb->s.N), sb->E);
  hipLaunchKernelGGL(scene_clear_kernel, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live);
  if (hemi)
    hipLaunchKernelGGL(ground_rays_begin_kernel<OI_GROUND_RAYS_HEMISPHERE>, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, g, *p);
  else if (mode == OI_GROUND_RAYS_LOCAL)
    hipLaunchKernelGGL(ground_rays_begin_kernel<OI_GROUND_RAYS_LOCAL>, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, g, *p);
  else
    hipLaunchKernelGGL(ground_rays_begin_kernel<OI_GROUND_RAYS_CAP>, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, g, *p);
  return oi::check_launch(what);
}

int oi_ground_resolve(const uint8_t* status, int E, long long n_g, int L, int S, int j0, int Sc, int last, int* count,
                      float* out, oi_stream_t stream) {
  const char* what = "oi_ground_resolve";
  OI_TRY(check_elements(what, E));
  OI_TRY(check_chunk(what, L, S, j0, Sc));
  OI_REQUIRE(n_g >= 1 && (long long)E * L * Sc * n_g < (1ll << 31), "%s: n_g=%lld (n_g >= 1, E * L * Sc * n_g < 2^31)", what, n_g);
  OI_REQUIRE(status && count && (out || !last), "%s: null pointer", what);
  hipLaunchKernelGGL(ground_resolve_kernel, dim3(n_blocks(n_g * L)), dim3(TR_THREADS), 0, oi::as_stream(stream), status, E, n_g, L,
                     S, j0, Sc, last, count, out);
  return oi::check_launch(what);
}

int oi_ground_shade(const float* c2w, const float* kinv, int S, const float* ground, const float* ground_t,
                    const int* ground_index, long long n_g, const float* lights, int L, int local, const float* visibility,
                    const float* ambient_occlusion, float* image, float* depth, float* position, float* normal_world,
                    float* albedo, float* mask, int* instance, float* ground_mask, float* shadow_matte, oi_stream_t stream) {
  const char* what = "oi_ground_shade";
  GroundShade p;
  p.g = GroundPoints{S, n_g, c2w, kinv, ground, ground_t, ground_index};
  OI_TRY(check_ground(what, &p.g));
  if (image || shadow_matte) {
    OI_TRY(check_lights(what, L));
    OI_REQUIRE(lights != nullptr, "%s: null lights with an image or a shadow matte", what);
  }
  p.L = L, p.lights = lights, p.visibility = visibility, p.ambient_occlusion = ambient_occlusion;
  p.image = image, p.depth = depth, p.position = position, p.normal_world = normal_world, p.albedo = albedo, p.mask = mask;
  p.instance = instance, p.ground_mask = ground_mask, p.shadow_matte = shadow_matte;
  const dim3 grid(n_blocks(n_g));
  if (local) hipLaunchKernelGGL(ground_shade_kernel<true>, grid, dim3(TR_THREADS), 0, oi::as_stream(stream), p);
  else hipLaunchKernelGGL(ground_shade_kernel<false>, grid, dim3(TR_THREADS), 0, oi::as_stream(stream), p);
  return oi::check_launch(what);
}

int oi_ground_occlude(const oi_trace_batch* sb, const float* ground, const int* elem, const float* b2w, long long n_vis,
                      float limit, oi_stream_t stream) {
  const char* what = "oi_ground_occlude";
  OI_TRY(check_batch(sb, what));
  OI_REQUIRE(n_vis >= 1 && n_vis <= sb->s.N && sb->s.N % n_vis == 0, "%s: n_vis=%lld, N=%lld (N must be a multiple of n_vis >= 1)",
             what, n_vis, sb->s.N);
  OI_REQUIRE(limit > 0.f, "%s: limit %g (> 0; INFINITY is allowed)", what, (double)limit);
  OI_REQUIRE(ground && elem && b2w, "%s: null pointer", what);
  hipLaunchKernelGGL(ground_occlude_kernel, dim3(n_blocks(sb->s.N)), dim3(TR_THREADS), 0, oi::as_stream(stream), sb->s, sb->E,
                     ground, elem, b2w, n_vis, limit);
  return oi::check_launch(what);
}

}  // extern "C"
