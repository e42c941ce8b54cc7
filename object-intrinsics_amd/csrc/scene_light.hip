// Soft shadows, ambient occlusion and environment lighting between the instances of a scene for gfx950
// (include/oi_scene_light.h): scene.hip's "every ray against every instance" layout with occlusion.hip's
// sampled rays.  Small memory-bound kernels, one thread per ray or scene pixel:
//   point_pixels        the scene pixel of every visible point: the key of its sample sequence
//   occlusion_begin     per occluder instance Sc sampled rays per (light, visible point): the direction drawn once in the
//                       owner's frame (trace_common.h's occlusion_direction, occlusion.hip's own), the owner's ray by
//                       occlusion.hip's expressions, any other instance's moved into its box frame and culled against its
//                       unit sphere (and against `distance` when ambient): scene_common.h's scene_sampled_begin, the one
//                       body of the scene's three samplers (the lobe's entry is scene_gloss.hip's)
//   step_anyhit         trace_common.h's state machine in its any-hit form on an element's view of the batched state
//   occlusion_resolve   per scene pixel the number of samples that missed every instance (scene_common.h's
//                       escaped_everywhere), accumulated across chunks as integers
//   transfer_resolve    per scene pixel the sum of sh9(world direction) over those samples, in sample order, the running sums
//                       kept in the output between chunks
//   transfer_normal     the unshadowed closed form on the owner's slices
//   shade_ao            scene.hip's shading with an occlusion factor on the ambient term
// The only atomics are the compaction's integer counters (wg_slot); the resolves loop over samples and elements in a fixed
// order.  No LDS beyond the compaction's counter words, no scratch.
#include "scene_common.h"

#include "../../include/oi_scene_light.h"

namespace {

constexpr int NC = OI_ENV_COEFFS;

__global__ void __launch_bounds__(TR_THREADS) scene_point_pixels_kernel(const int* __restrict__ counts, long long N,
                                                                        const int* __restrict__ vis_index,
                                                                        const int* __restrict__ window, int W, int S,
                                                                        const int* __restrict__ offset, long long n_vis,
                                                                        int* __restrict__ pixel) {
  const int e = blockIdx.y;
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= N || i >= counts[(long long)e * OI_TRACE_COUNT_WORDS + N_HIT_WORD]) return;
  const long long g = (long long)offset[e] + i;
  if (g < 0 || g >= n_vis) return;  // (offsets that do not belong to these counts: nothing is written outside the list)
  const int r = vis_index[(long long)e * N + i];
  const int j = r / W, c = r - j * W;
  const long long X = (long long)window[e * 2 + 0] + c, Y = (long long)window[e * 2 + 1] + j;
  pixel[g] = (int)(Y * S + X);
}

template <SceneSampler X>
__global__ void __launch_bounds__(TR_THREADS) scene_occlusion_begin_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                           const oi_scene_occlusion_params p) {
  __shared__ unsigned lds[TR_WAVES + 1];
  scene_sampled_begin<X>(s, live, p, SceneLobe{}, lds);
}

__global__ void __launch_bounds__(TR_THREADS) trace_batch_step_anyhit_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                             const float* __restrict__ sdf, long long bound,
                                                                             int k, float tol, float omega) {
  __shared__ unsigned lds[TR_WAVES + 1];
  trace_step_rays<true>(element_view(s, blockIdx.y), sdf + (long long)blockIdx.y * s.N, bound, k, tol, omega, lds, live + k + 1);
}

__global__ void __launch_bounds__(TR_THREADS) scene_occlusion_resolve_kernel(const uint8_t* __restrict__ status,
                                                                             const int* __restrict__ owner,
                                                                             const int* __restrict__ owner_ray,
                                                                             const int* __restrict__ vis_slot,
                                                                             const int* __restrict__ offset, int E, long long N,
                                                                             int L, int S, int j0, int Sc, long long n_vis,
                                                                             long long M, int last, int* __restrict__ count,
                                                                             float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= M * L) return;
  const long long l = i / M, q = i - l * M;
  const int e = owner[q];
  int c = 0;
  if (e >= 0) {
    const long long g = (long long)offset[e] + vis_slot[(long long)e * N + owner_ray[q]];
    if (j0 > 0) c = count[i];
    for (int jj = 0; jj < Sc; ++jj) c += escaped_everywhere(status, E, (long long)L * Sc * n_vis, (l * Sc + jj) * n_vis + g) ? 1 : 0;
  }
  count[i] = c;
  if (last) out[i] = e >= 0 ? (float)c / (float)S : 1.0f;
}

__global__ void __launch_bounds__(TR_THREADS) scene_transfer_resolve_kernel(const uint8_t* __restrict__ status,
                                                                            const float* __restrict__ rays_d,
                                                                            const int* __restrict__ owner,
                                                                            const int* __restrict__ owner_ray,
                                                                            const int* __restrict__ vis_slot,
                                                                            const int* __restrict__ offset,
                                                                            const float* __restrict__ w2b, int E, long long N,
                                                                            int S, int j0, int Sc, long long n_vis, long long M,
                                                                            int last, float* __restrict__ transfer) {
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= M) return;
  const int e = owner[q];
  float acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.f;
  if (e >= 0) {
    if (j0 > 0) {
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] = transfer[c * M + q];
    }
    const long long g = (long long)offset[e] + vis_slot[(long long)e * N + owner_ray[q]], rays = (long long)Sc * n_vis;
    const float* Wb = w2b + (long long)e * 16;
    for (int jj = 0; jj < Sc; ++jj) {
      const long long ray = (long long)jj * n_vis + g;
      if (!escaped_everywhere(status, E, rays, ray)) continue;
      const long long r = (long long)e * rays + ray;  // the owner's element holds the direction in the owner's frame
      float x, y, z;
      to_world(Wb, rays_d[r * 3 + 0], rays_d[r * 3 + 1], rays_d[r * 3 + 2], x, y, z);
      normalize3(x, y, z, 1e-6f);
      float sh[NC];
      sh9(x, y, z, sh);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] += sh[c];
    }
    if (last) {
      const float s = (float)S;
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] /= s;
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) transfer[c * M + q] = acc[c];
}

__global__ void __launch_bounds__(TR_THREADS) scene_transfer_normal_kernel(const float* __restrict__ grad, long long n_pad,
                                                                           const int* __restrict__ owner,
                                                                           const int* __restrict__ owner_ray,
                                                                           const int* __restrict__ vis_slot,
                                                                           const float* __restrict__ w2b, long long N,
                                                                           long long M, float* __restrict__ transfer) {
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= M) return;
  const int e = owner[q];
  float t[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) t[c] = 0.f;
  if (e >= 0) {
    const long long k = (long long)e * n_pad + vis_slot[(long long)e * N + owner_ray[q]];
    float nx, ny, nz;
    unit_normal(grad, k, nx, ny, nz);
    normal_transfer(w2b + (long long)e * 16, nx, ny, nz, t);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) transfer[c * M + q] = t[c];
}

__global__ void __launch_bounds__(TR_THREADS) scene_shade_ao_kernel(const oi_scene_shade_ao_params p) {
  scene_shade_pixel(p.s, p.ambient_occlusion);
}

}  // namespace

extern "C" {

int oi_scene_point_pixels(const oi_trace_batch* b, const int* vis_index, const int* window, int W, int S, const int* offset,
                          long long n_vis, int* pixel, oi_stream_t stream) {
  const char* what = "oi_scene_point_pixels";
  OI_TRY(check_batch(b, what));
  OI_REQUIRE(W >= 1 && (long long)W * W == b->s.N, "%s: W=%d, N=%lld rays per element (N must be W * W)", what, W, b->s.N);
  OI_TRY(check_resolution(what, "S", S));
  OI_REQUIRE(n_vis >= 1 && n_vis <= b->E * b->s.N, "%s: n_vis=%lld (1 <= n_vis <= E * N = %lld)", what, n_vis, b->E * b->s.N);
  OI_REQUIRE(vis_index && window && offset && pixel, "%s: null pointer", what);
  hipLaunchKernelGGL(scene_point_pixels_kernel, dim3(n_blocks(b->s.N), b->E), dim3(TR_THREADS), 0, oi::as_stream(stream),
                     b->s.counts, b->s.N, vis_index, window, W, S, offset, n_vis, pixel);
  return oi::check_launch(what);
}

int oi_scene_occlusion_begin(const oi_trace_batch* sb, const oi_scene_occlusion_params* p, oi_stream_t stream) {
  const char* what = "oi_scene_occlusion_begin";
  OI_TRY(check_batch(sb, what));
  OI_REQUIRE(p != nullptr, "%s: null params", what);
  OI_TRY(check_chunk(what, p->L, p->S, p->j0, p->Sc));
  OI_REQUIRE(!p->ambient || p->L == 1, "%s: L=%d with ambient (the hemisphere is one set of rays: L must be 1)", what, p->L);
  OI_TRY(check_sampled_rays(what, sb, p));
  OI_REQUIRE(!p->ambient || p->distance > 0.f, "%s: distance %g (> 0; INFINITY is allowed)", what, (double)p->distance);
  OI_REQUIRE(p->hit_points && p->grad && p->offset && p->elem && p->pixel && p->position && p->normal && p->w2b &&
                 (p->ambient || (p->lights && p->radius)),
             "%s: null input pointer", what);
  const hipStream_t st = oi::as_stream(stream);
  const dim3 grid(n_blocks(sb->s.N), sb->E);
  hipLaunchKernelGGL(scene_clear_kernel, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live);
  if (p->ambient)
    hipLaunchKernelGGL(scene_occlusion_begin_kernel<SceneSampler::HEMISPHERE>, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, *p);
  else
    hipLaunchKernelGGL(scene_occlusion_begin_kernel<SceneSampler::CAP>, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, *p);
  return oi::check_launch(what);
}

int oi_trace_batch_step_anyhit(const oi_trace_batch* b, const float* sdf, long long bound, int k, float tol, float omega,
                               oi_stream_t stream) {
  const char* what = "oi_trace_batch_step_anyhit";
  OI_TRY(check_batch(b, what));
  OI_REQUIRE(k >= 0 && k < OI_TRACE_MAX_STEPS, "%s: step k=%d (0 <= k < %d)", what, k, OI_TRACE_MAX_STEPS);
  OI_REQUIRE(bound >= 0 && bound <= b->s.N, "%s: bound=%lld (0 <= bound <= N=%lld)", what, bound, b->s.N);
  OI_REQUIRE(tol > 0.f && omega > 0.f && tol < INFINITY && omega < INFINITY, "%s: tol %g, omega %g (both > 0, finite)", what,
             (double)tol, (double)omega);
  if (bound == 0) return OI_OK;
  OI_REQUIRE(sdf != nullptr, "%s: null sdf", what);
  hipLaunchKernelGGL(trace_batch_step_anyhit_kernel, dim3(n_blocks(bound), b->E), dim3(TR_THREADS), 0, oi::as_stream(stream), b->s,
                     b->live, sdf, bound, k, tol, omega);
  return oi::check_launch(what);
}

int oi_scene_occlusion_resolve(const uint8_t* status, const int* owner, const int* owner_ray, const int* vis_slot,
                               const int* offset, int E, long long N, int L, int S, int j0, int Sc, long long n_vis,
                               int scene_S, int last, int* count, float* out, oi_stream_t stream) {
  const char* what = "oi_scene_occlusion_resolve";
  OI_TRY(check_chunk(what, L, S, j0, Sc));
  OI_TRY(check_resolve(what, E, N, L, Sc, n_vis, scene_S));
  OI_REQUIRE(status && owner && owner_ray && vis_slot && offset && count && (out || !last), "%s: null pointer", what);
  const long long M = (long long)scene_S * scene_S;
  hipLaunchKernelGGL(scene_occlusion_resolve_kernel, dim3(n_blocks(M * L)), dim3(TR_THREADS), 0, oi::as_stream(stream), status, owner,
                     owner_ray, vis_slot, offset, E, N, L, S, j0, Sc, n_vis, M, last, count, out);
  return oi::check_launch(what);
}

int oi_scene_transfer_resolve(const uint8_t* status, const float* rays_d, const int* owner, const int* owner_ray,
                              const int* vis_slot, const int* offset, const float* w2b, int E, long long N, int S, int j0,
                              int Sc, long long n_vis, int scene_S, int last, float* transfer, oi_stream_t stream) {
  const char* what = "oi_scene_transfer_resolve";
  OI_TRY(check_chunk(what, 1, S, j0, Sc));
  OI_TRY(check_resolve(what, E, N, 1, Sc, n_vis, scene_S));
  OI_REQUIRE(status && rays_d && owner && owner_ray && vis_slot && offset && w2b && transfer, "%s: null pointer", what);
  const long long M = (long long)scene_S * scene_S;
  hipLaunchKernelGGL(scene_transfer_resolve_kernel, dim3(n_blocks(M)), dim3(TR_THREADS), 0, oi::as_stream(stream), status, rays_d,
                     owner, owner_ray, vis_slot, offset, w2b, E, N, S, j0, Sc, n_vis, M, last, transfer);
  return oi::check_launch(what);
}

int oi_scene_transfer_normal(const float* grad, long long n_pad, const int* owner, const int* owner_ray, const int* vis_slot,
                             const float* w2b, int E, long long N, int scene_S, float* transfer, oi_stream_t stream) {
  const char* what = "oi_scene_transfer_normal";
  OI_TRY(check_scene_rays(what, E, N));
  OI_REQUIRE(n_pad >= 1 && n_pad <= N, "%s: n_pad=%lld (1 <= n_pad <= N=%lld)", what, n_pad, N);
  OI_TRY(check_resolution(what, "scene S", scene_S));
  OI_REQUIRE(grad && owner && owner_ray && vis_slot && w2b && transfer, "%s: null pointer", what);
  const long long M = (long long)scene_S * scene_S;
  hipLaunchKernelGGL(scene_transfer_normal_kernel, dim3(n_blocks(M)), dim3(TR_THREADS), 0, oi::as_stream(stream), grad, n_pad, owner,
                     owner_ray, vis_slot, w2b, N, M, transfer);
  return oi::check_launch(what);
}

int oi_scene_shade_ao(const oi_scene_shade_ao_params* p, oi_stream_t stream) {
  const char* what = "oi_scene_shade_ao";
  OI_REQUIRE(p != nullptr, "%s: null params", what);
  OI_TRY(check_scene_shade(&p->s, what));
  hipLaunchKernelGGL(scene_shade_ao_kernel, dim3(n_blocks((long long)p->s.S * p->s.S)), dim3(TR_THREADS), 0, oi::as_stream(stream),
                     *p);
  return oi::check_launch(what);
}

}  // extern "C"
