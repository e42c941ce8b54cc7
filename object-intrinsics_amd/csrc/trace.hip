// Sphere-traced surface rendering for gfx950 (include/oi_trace.h): small memory-bound kernels around
// the library's own MLP passes (oi_sdf_mlp_fwd, called by the host between them), one thread per ray or pixel:
//   begin          t = near, first sample points, identity active list, the per-step counters
//   step           the ray state machine on the sdf of the last MLP pass (march, bracket, Illinois regula falsi) and the
//                  compaction of the rays still in flight: next active list + next sample points, densely
//   finish         rays still in flight -> LIMIT; the hits gathered densely (index, point) and the pixel -> hit map
//   shadow_begin   one shadow ray per (light, hit) facing the light, offset along the normal, compacted like a step
//   visibility     shadow-ray states -> the (L, N) visibility map
//   shade          G-buffer (depth, position, normals, albedo, mask) and the Phong image under L lights
// The per-ray work of begin, step and finish, the compaction, the state a begin kernel writes (write_ray, enter_rays), the
// lit share that visibility is at S = 1, the shading and the shared argument checks live in trace_common.h, which
// occlusion.hip, trace_batch.hip, envgloss.hip and the scene sources share.
// Compaction inside a workgroup: one 64-bit ballot per wave (popcount on the lower lanes) and an LDS scan over the waves,
// as mesh.hip; across workgroups one integer atomicAdd per workgroup on the step's counter.  No float atomics, no scratch.
#include "trace_common.h"

namespace {

__global__ void __launch_bounds__(TR_THREADS) trace_begin_kernel(const oi_trace_state s) { trace_begin_rays(s); }

__global__ void __launch_bounds__(TR_THREADS) trace_finish_kernel(const oi_trace_state s, int* __restrict__ hit_index,
                                                                  float* __restrict__ hit_points,
                                                                  int* __restrict__ hit_slot) {
  __shared__ unsigned lds[TR_WAVES + 1];
  trace_finish_rays<true>(s, hit_index, hit_points, hit_slot, lds);
}

__global__ void __launch_bounds__(TR_THREADS) trace_shadow_begin_kernel(const oi_trace_state s,
                                                                        const float* __restrict__ hit_points,
                                                                        const float* __restrict__ grad, long long n_hit,
                                                                        const float* __restrict__ lights,
                                                                        const float* __restrict__ w2b, float bias) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  BeginRay ry = {};
  if (q < s.N) {
    const long long l = q / n_hit, i = q - l * n_hit;
    ry = begin_ray<BEGIN_SHADOW>(hit_points, grad, nullptr, i, l, 0u, 1, lights, nullptr, w2b, bias, 0.f, 0u);
    write_ray(s, q, ry.o, ry.d, 0.f, ry.far_, ry.status);
  }
  enter_rays(s, q, ry.entered, ry.o[0], ry.o[1], ry.o[2], lds);
}

__global__ void __launch_bounds__(TR_THREADS) trace_visibility_kernel(const uint8_t* __restrict__ status,
                                                                      const int* __restrict__ hit_slot, long long N,
                                                                      long long n_hit, int L, float* __restrict__ vis) {
  lit_share(status, hit_slot, N, n_hit, L, 1, vis);
}

__global__ void __launch_bounds__(TR_THREADS) surface_shade_kernel(const oi_surface_params p) { surface_shade_pixel(p, nullptr); }

}  // namespace

extern "C" {

int oi_trace_begin(const oi_trace_state* s, oi_stream_t stream) {
  OI_TRY(check_state(s, "oi_trace_begin"));
  hipLaunchKernelGGL(trace_begin_kernel, dim3(n_blocks(s->N)), dim3(TR_THREADS), 0, oi::as_stream(stream), *s);
  return oi::check_launch("oi_trace_begin");
}

int oi_trace_step(const oi_trace_state* s, const float* sdf, long long bound, int k, float tol, float omega,
                  oi_stream_t stream) {
  return launch_step<false>("oi_trace_step", s, sdf, bound, k, tol, omega, stream);
}

int oi_trace_finish(const oi_trace_state* s, int* hit_index, float* hit_points, int* hit_slot, oi_stream_t stream) {
  OI_TRY(check_state(s, "oi_trace_finish"));
  OI_REQUIRE(hit_index && hit_points && hit_slot, "oi_trace_finish: null output pointer");
  hipLaunchKernelGGL(trace_finish_kernel, dim3(n_blocks(s->N)), dim3(TR_THREADS), 0, oi::as_stream(stream), *s, hit_index,
                     hit_points, hit_slot);
  return oi::check_launch("oi_trace_finish");
}

int oi_trace_shadow_begin(const oi_trace_state* s, const float* hit_points, const float* grad, long long n_hit,
                          const float* lights, int L, const float* w2b, float bias, oi_stream_t stream) {
  const char* what = "oi_trace_shadow_begin";
  OI_TRY(check_state(s, what));
  OI_TRY(check_lights(what, L));
  OI_REQUIRE(n_hit >= 1 && n_hit * L == s->N, "%s: n_hit=%lld, L=%d, N=%lld (N must be L * n_hit)", what, n_hit, L, s->N);
  OI_TRY(check_bias(what, bias));
  OI_REQUIRE(hit_points && grad && lights && w2b, "%s: null input pointer", what);
  return launch_begin(what, s, stream, trace_shadow_begin_kernel, hit_points, grad, n_hit, lights, w2b, bias);
}

int oi_trace_visibility(const uint8_t* shadow_status, const int* hit_slot, long long N, long long n_hit, int L,
                        float* visibility, oi_stream_t stream) {
  OI_TRY(check_pixels("oi_trace_visibility", N, n_hit));
  OI_TRY(check_lights("oi_trace_visibility", L));
  OI_REQUIRE(hit_slot && visibility && (shadow_status || n_hit == 0), "oi_trace_visibility: null pointer");
  hipLaunchKernelGGL(trace_visibility_kernel, dim3(n_blocks(N * L)), dim3(TR_THREADS), 0, oi::as_stream(stream), shadow_status,
                     hit_slot, N, n_hit, L, visibility);
  return oi::check_launch("oi_trace_visibility");
}

int oi_surface_shade(const oi_surface_params* p, oi_stream_t stream) {
  OI_TRY(check_surface("oi_surface_shade", p));
  hipLaunchKernelGGL(surface_shade_kernel, dim3(n_blocks(p->N)), dim3(TR_THREADS), 0, oi::as_stream(stream), *p);
  return oi::check_launch("oi_surface_shade");
}

}  // extern "C"
