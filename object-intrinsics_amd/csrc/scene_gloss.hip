// Glossy environment lighting in a scene of many instances for gfx950 (include/oi_scene_gloss.h):
// envgloss.hip's reflection lobe with scene_light.hip's "every sampled ray against every instance".  Small memory-bound
// kernels, one thread per ray or pixel:
//   scene_lobe_begin      per occluder instance Sc lobe rays per visible point: scene_common.h's scene_sampled_begin with the
//                         LOBE sampler (trace_common.h's reflect_view and lobe_direction, envgloss.hip's own); the march, the
//                         finish and the resolve are scene_light.hip's and trace_batch.hip's
//   scene_reflect         per scene pixel the reflected view vector of its owner's point, in the world
//   env_shade_glossy_dirs env_shade_common.h's pixel with the GLOSSY_DIRS term: the lookup direction read from that plane
// The only atomics are the compaction's integer counters (wg_slot).  No LDS beyond the compaction's counter words, no scratch.
#include "env_shade_common.h"
#include "scene_common.h"

#include "../../include/oi_scene_gloss.h"

namespace {

__global__ void __launch_bounds__(TR_THREADS) scene_lobe_begin_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                      const oi_scene_occlusion_params p, const SceneLobe g) {
  __shared__ unsigned lds[TR_WAVES + 1];
  scene_sampled_begin<SceneSampler::LOBE>(s, live, p, g, lds);
}

__global__ void __launch_bounds__(TR_THREADS) scene_reflect_kernel(const float* __restrict__ rays_o,
                                                                   const float* __restrict__ hit_points,
                                                                   const float* __restrict__ grad, long long n_pad,
                                                                   const int* __restrict__ owner,
                                                                   const int* __restrict__ owner_ray,
                                                                   const int* __restrict__ vis_slot,
                                                                   const float* __restrict__ w2b, long long N, long long M,
                                                                   float* __restrict__ reflect) {
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= M) return;
  const int e = owner[q];
  float w[3] = {0.f, 0.f, 0.f};
  if (e >= 0) {
    const long long ray = (long long)e * N + owner_ray[q];
    float n[3], r[3];
    reflect_view(grad, hit_points, (long long)e * n_pad + vis_slot[ray], rays_o + ray * 3, n, r);
    to_world(w2b + (long long)e * 16, r[0], r[1], r[2], w[0], w[1], w[2]);
  }
  reflect[q * 3 + 0] = w[0], reflect[q * 3 + 1] = w[1], reflect[q * 3 + 2] = w[2];
}

__global__ void __launch_bounds__(ES_THREADS) env_shade_glossy_dirs_kernel(const oi_env_shade_params p, const GlossArgs g,
                                                                           const MapIndex mi) {
  env_shade_pixel<EnvTerm::GLOSSY_DIRS>(p, g, mi);
}

}  // namespace

extern "C" {

int oi_scene_lobe_begin(const oi_trace_batch* sb, const oi_scene_occlusion_params* op, const float* rays_o, const int* vis_index,
                        long long N, float shininess, oi_stream_t stream) {
  const char* what = "oi_scene_lobe_begin";
  OI_TRY(check_batch(sb, what));
  OI_REQUIRE(op != nullptr, "%s: null params", what);
  const oi_scene_occlusion_params& o = *op;
  OI_TRY(check_chunk(what, o.L, o.S, o.j0, o.Sc));
  OI_REQUIRE(o.L == 1, "%s: L=%d (the lobe is one set of rays: L must be 1)", what, o.L);
  OI_TRY(check_sampled_rays(what, sb, &o));
  OI_REQUIRE(shininess_ok(shininess), "%s: shininess %g (%d .. %d, finite)", what, (double)shininess, OI_ENVGLOSS_MIN_SHININESS,
             OI_ENVGLOSS_MAX_SHININESS);
  OI_TRY(check_scene_rays(what, sb->E, N));
  OI_REQUIRE(o.n_pad <= N, "%s: n_pad=%lld (1 <= n_pad <= N=%lld)", what, o.n_pad, N);
  OI_REQUIRE(o.hit_points && o.grad && o.offset && o.elem && o.pixel && o.position && o.normal && o.w2b && rays_o && vis_index,
             "%s: null input pointer", what);
  const SceneLobe g = {rays_o, vis_index, N, 1.0f / (shininess + 1.0f)};
  const hipStream_t st = oi::as_stream(stream);
  const dim3 grid(n_blocks(sb->s.N), sb->E);
  hipLaunchKernelGGL(scene_clear_kernel, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live);
  hipLaunchKernelGGL(scene_lobe_begin_kernel, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, o, g);
  return oi::check_launch(what);
}

int oi_scene_reflect(const float* rays_o, const float* hit_points, const float* grad, long long n_pad, const int* owner,
                     const int* owner_ray, const int* vis_slot, const float* w2b, int E, long long N, int scene_S,
                     float* reflect, oi_stream_t stream) {
  const char* what = "oi_scene_reflect";
  OI_TRY(check_scene_rays(what, E, N));
  OI_REQUIRE(n_pad >= 1 && n_pad <= N, "%s: n_pad=%lld (1 <= n_pad <= N=%lld)", what, n_pad, N);
  OI_TRY(check_resolution(what, "scene S", scene_S));
  OI_REQUIRE(rays_o && hit_points && grad && owner && owner_ray && vis_slot && w2b && reflect, "%s: null pointer", what);
  const long long M = (long long)scene_S * scene_S;
  hipLaunchKernelGGL(scene_reflect_kernel, dim3(n_blocks(M)), dim3(TR_THREADS), 0, oi::as_stream(stream), rays_o, hit_points, grad,
                     n_pad, owner, owner_ray, vis_slot, w2b, N, M, reflect);
  return oi::check_launch(what);
}

int oi_env_shade_glossy_dirs(const oi_env_shade_params* p, const float* dirs, const float* spec_vis, const float* glossy, int M,
                             int Hp, int Wp, const int* map_index, const float* rot, const float* k_s, float* specular,
                             oi_stream_t stream) {
  const char* what = "oi_env_shade_glossy_dirs";
  OI_TRY(check_env_shade(what, p, p && (p->shading || p->image || specular), "shading, image and specular are all null"));
  OI_TRY(check_gloss_maps(what, M, Hp, Wp));
  OI_REQUIRE(glossy && map_index && rot && k_s, "%s: null glossy input pointer", what);
  OI_REQUIRE(p->n_hit == 0 || dirs, "%s: null dirs with n_hit=%lld", what, p->n_hit);
  MapIndex mi = {};
  OI_TRY(pack_map_index(what, p->F, M, map_index, mi));
  const GlossArgs g = {nullptr, nullptr, nullptr, nullptr, spec_vis, glossy, rot, k_s, specular, Hp, Wp, dirs};
  hipLaunchKernelGGL(env_shade_glossy_dirs_kernel, dim3((unsigned)((p->N + ES_THREADS - 1) / ES_THREADS)), dim3(ES_THREADS), 0,
                     oi::as_stream(stream), *p, g, mi);
  return oi::check_launch(what);
}

}  // extern "C"
