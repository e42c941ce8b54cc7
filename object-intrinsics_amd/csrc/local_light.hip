// Local lights for the sphere-traced renderer and for scenes (include/oi_local_light.h), gfx950: point,
// spot and sphere lights that stand in the world, with shadow rays that end at the light.  Small memory-bound kernels, one
// thread per ray or pixel, around the library's own sdf-only MLP passes and the any-hit step, which are unchanged:
//   local_light_begin        S rays per (light, visible point) aimed at the light's sphere (trace_common.h's aimed_sample),
//                            far = min(where the ray meets the light, the exit of the unit sphere); compacted like a step
//   scene_local_light_begin  the same ray against every instance of a scene (scene_common.h's scene_local_begin): drawn once
//                            in the owner's frame, moved into every other instance's box frame, culled and cut at the light
//   surface_shade_local      oi_surface_shade's G-buffer (the same body) and the Phong image with the per-pixel direction,
//                            the inverse-square falloff and the cone (trace_common.h's local_shade_at)
//   scene_shade_local        the same pixel on the owner's slices of a scene
// The state a begin kernel writes and its compaction are trace_common.h's write_ray and enter_rays, as every begin kernel's.
// No float atomics, no scratch; the only atomics are the compaction's integer counters.
#include "scene_common.h"

#include "../../include/oi_local_light.h"

namespace {

__global__ void __launch_bounds__(TR_THREADS) local_light_begin_kernel(const oi_trace_state s, const float* __restrict__ hit_points,
                                                                       const float* __restrict__ grad,
                                                                       const int* __restrict__ hit_index, long long n_hit,
                                                                       const float* __restrict__ lights, int S,
                                                                       const float* __restrict__ w2b, float bias, unsigned seed) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  BeginRay ry = {};
  if (q < s.N) {
    const long long lj = q / n_hit, i = q - lj * n_hit;
    const long long l = lj / S;
    const unsigned j = (unsigned)(lj - l * S);
    ry = begin_ray<BEGIN_LOCAL>(hit_points, grad, hit_index, i, l, j, S, lights, nullptr, w2b, bias, 0.f, seed);
    write_ray(s, q, ry.o, ry.d, 0.f, ry.far_, ry.status);
  }
  enter_rays(s, q, ry.entered, ry.o[0], ry.o[1], ry.o[2], lds);
}

__global__ void __launch_bounds__(TR_THREADS) scene_local_light_begin_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                             const oi_scene_occlusion_params p) {
  __shared__ unsigned lds[TR_WAVES + 1];
  scene_local_begin(s, live, p, lds);
}

__global__ void __launch_bounds__(TR_THREADS) surface_shade_local_kernel(const oi_surface_ao_params p) {
  const long long r = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (r >= p.N) return;
  surface_shade_local_at(p, p.ambient_occlusion, r, p.status[r] == OI_TRACE_HIT, r, p.N);
}

__global__ void __launch_bounds__(TR_THREADS) scene_shade_local_kernel(const oi_scene_shade_ao_params p) {
  scene_shade_pixel<true>(p.s, p.ambient_occlusion);
}

}  // namespace

extern "C" {

int oi_local_light_begin(const oi_trace_state* s, const float* hit_points, const float* grad, const int* hit_index,
                         long long n_hit, const float* lights, int L, int S, const float* w2b, float bias, unsigned seed,
                         oi_stream_t stream) {
  const char* what = "oi_local_light_begin";
  OI_TRY(check_state(s, what));
  OI_TRY(check_lights(what, L));
  OI_TRY(check_samples(what, S));
  OI_REQUIRE(n_hit >= 1 && n_hit < (1ll << 31) && n_hit * L * S == s->N,
             "%s: n_hit=%lld, L=%d, S=%d, N=%lld (N must be L * S * n_hit, below 2^31)", what, n_hit, L, S, s->N);
  OI_TRY(check_bias(what, bias));
  OI_REQUIRE(hit_points && grad && hit_index && lights && w2b, "%s: null input pointer", what);
  return launch_begin(what, s, stream, local_light_begin_kernel, hit_points, grad, hit_index, n_hit, lights, S, w2b, bias, seed);
}

int oi_surface_shade_local(const oi_surface_ao_params* p, oi_stream_t stream) {
  OI_TRY(check_surface("oi_surface_shade_local", p));
  hipLaunchKernelGGL(surface_shade_local_kernel, dim3(n_blocks(p->N)), dim3(TR_THREADS), 0, oi::as_stream(stream), *p);
  return oi::check_launch("oi_surface_shade_local");
}

int oi_scene_local_light_begin(const oi_trace_batch* sb, const oi_scene_occlusion_params* p, oi_stream_t stream) {
  const char* what = "oi_scene_local_light_begin";
  OI_TRY(check_batch(sb, what));
  OI_REQUIRE(p != nullptr, "%s: null params", what);
  OI_TRY(check_chunk(what, p->L, p->S, p->j0, p->Sc));
  OI_REQUIRE(!p->ambient, "%s: ambient=%d (local lights have no ambient form: must be 0)", what, p->ambient);
  OI_TRY(check_sampled_rays(what, sb, p));
  OI_REQUIRE(p->hit_points && p->grad && p->offset && p->elem && p->pixel && p->position && p->normal && p->w2b && p->lights,
             "%s: null input pointer", what);
  const hipStream_t st = oi::as_stream(stream);
  const dim3 grid(n_blocks(sb->s.N), sb->E);
  hipLaunchKernelGGL(scene_clear_kernel, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live);
  hipLaunchKernelGGL(scene_local_light_begin_kernel, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, *p);
  return oi::check_launch(what);
}

int oi_scene_shade_local(const oi_scene_shade_ao_params* p, oi_stream_t stream) {
  const char* what = "oi_scene_shade_local";
  OI_REQUIRE(p != nullptr, "%s: null params", what);
  OI_TRY(check_scene_shade(&p->s, what));
  hipLaunchKernelGGL(scene_shade_local_kernel, dim3(n_blocks((long long)p->s.S * p->s.S)), dim3(TR_THREADS), 0, oi::as_stream(stream),
                     *p);
  return oi::check_launch("oi_scene_shade_local");
}

}  // extern "C"
