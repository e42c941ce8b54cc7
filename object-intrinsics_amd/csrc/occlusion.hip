// Soft shadows and ambient occlusion for the sphere-traced renderer (include/oi_occlusion.h), gfx950.
// One thread per secondary ray or pixel, around the library's own sdf-only MLP passes:
//   light_begin / ambient_begin   S sample directions per (light, visible point): a cap about the light's direction, uniform
//                                 in solid angle, or the cosine-weighted hemisphere about the normal; offset along the
//                                 normal, compacted like a step
//   step                          trace_common.h's state machine in its any-hit form: the first occluder ends the ray
//   resolve                       S ray states per light and pixel -> the share that ended MISS (trace_common.h's lit_share)
//   shade_ao                      trace_common.h's shading with an occlusion factor on the ambient term
// The state a begin kernel writes and its compaction are trace_common.h's write_ray and enter_rays, as every begin kernel's.
// No float atomics, no scratch; the only atomics are the compaction's integer counters (one add per workgroup).
#include "trace_common.h"

namespace {

// AMBIENT = false: rays to L lights of angular radius radius[l].  AMBIENT = true: L = 1, the hemisphere about the normal.
template <bool AMBIENT>
__global__ void __launch_bounds__(TR_THREADS) occlusion_begin_kernel(const oi_trace_state s,
                                                                     const float* __restrict__ hit_points,
                                                                     const float* __restrict__ grad,
                                                                     const int* __restrict__ hit_index, long long n_hit,
                                                                     const float* __restrict__ lights,
                                                                     const float* __restrict__ radius, int S,
                                                                     const float* __restrict__ w2b, float bias, float distance,
                                                                     unsigned seed) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  BeginRay ry = {};
  if (q < s.N) {
    const long long lj = q / n_hit, i = q - lj * n_hit;
    const long long l = lj / S;
    const unsigned j = (unsigned)(lj - l * S);
    ry = begin_ray<AMBIENT ? BEGIN_HEMISPHERE : BEGIN_CAP>(hit_points, grad, hit_index, i, l, j, S, lights, radius, w2b, bias, distance, seed);
    write_ray(s, q, ry.o, ry.d, 0.f, ry.far_, ry.status);
  }
  enter_rays(s, q, ry.entered, ry.o[0], ry.o[1], ry.o[2], lds);
}

__global__ void __launch_bounds__(TR_THREADS) occlusion_resolve_kernel(const uint8_t* __restrict__ status,
                                                                       const int* __restrict__ hit_slot, long long N,
                                                                       long long n_hit, int L, int S, float* __restrict__ out) {
  lit_share(status, hit_slot, N, n_hit, L, S, out);
}

__global__ void __launch_bounds__(TR_THREADS) surface_shade_ao_kernel(const oi_surface_ao_params p) {
  surface_shade_pixel(p, p.ambient_occlusion);
}

// what the two begin entries share: the state, the counts and the ray layout
int check_begin(const char* what, const oi_trace_state* s, long long n_hit, int L, int S, float bias) {
  OI_TRY(check_state(s, what));
  OI_TRY(check_lights(what, L));
  OI_TRY(check_samples(what, S));
  OI_REQUIRE(n_hit >= 1 && n_hit < (1ll << 31) && n_hit * L * S == s->N,
             "%s: n_hit=%lld, L=%d, S=%d, N=%lld (N must be L * S * n_hit, below 2^31)", what, n_hit, L, S, s->N);
  return check_bias(what, bias);
}

}  // namespace

extern "C" {

int oi_occlusion_light_begin(const oi_trace_state* s, const float* hit_points, const float* grad, const int* hit_index,
                             long long n_hit, const float* lights, const float* radius, int L, int S, const float* w2b,
                             float bias, unsigned seed, oi_stream_t stream) {
  OI_TRY(check_begin("oi_occlusion_light_begin", s, n_hit, L, S, bias));
  OI_REQUIRE(radius != nullptr, "oi_occlusion_light_begin: null radius (one angular radius per light, device memory)");
  OI_REQUIRE(hit_points && grad && hit_index && lights && w2b, "oi_occlusion_light_begin: null input pointer");
  return launch_begin("oi_occlusion_light_begin", s, stream, occlusion_begin_kernel<false>, hit_points, grad, hit_index, n_hit, lights,
                      radius, S, w2b, bias, 0.f, seed);
}

int oi_occlusion_ambient_begin(const oi_trace_state* s, const float* hit_points, const float* grad, const int* hit_index,
                               long long n_hit, int S, float bias, float distance, unsigned seed, oi_stream_t stream) {
  OI_TRY(check_begin("oi_occlusion_ambient_begin", s, n_hit, 1, S, bias));
  OI_REQUIRE(distance > 0.f && distance < INFINITY, "oi_occlusion_ambient_begin: distance %g (> 0, finite)", (double)distance);
  OI_REQUIRE(hit_points && grad && hit_index, "oi_occlusion_ambient_begin: null input pointer");
  const float* const none = nullptr;  // lights, radius, w2b: not read
  return launch_begin("oi_occlusion_ambient_begin", s, stream, occlusion_begin_kernel<true>, hit_points, grad, hit_index, n_hit, none,
                      none, S, none, bias, distance, seed);
}

int oi_occlusion_step(const oi_trace_state* s, const float* sdf, long long bound, int k, float tol, float omega,
                      oi_stream_t stream) {
  return launch_step<true>("oi_occlusion_step", s, sdf, bound, k, tol, omega, stream);
}

int oi_occlusion_resolve(const uint8_t* status, const int* hit_slot, long long N, long long n_hit, int L, int S, float* out,
                         oi_stream_t stream) {
  OI_TRY(check_pixels("oi_occlusion_resolve", N, n_hit));
  OI_TRY(check_lights("oi_occlusion_resolve", L));
  OI_TRY(check_samples("oi_occlusion_resolve", S));
  OI_REQUIRE(n_hit * L * S < (1ll << 31), "oi_occlusion_resolve: L * S * n_hit = %lld rays (below 2^31)", n_hit * L * S);
  OI_REQUIRE(hit_slot && out && (status || n_hit == 0), "oi_occlusion_resolve: null pointer");
  hipLaunchKernelGGL(occlusion_resolve_kernel, dim3(n_blocks(N * L)), dim3(TR_THREADS), 0, oi::as_stream(stream), status, hit_slot,
                     N, n_hit, L, S, out);
  return oi::check_launch("oi_occlusion_resolve");
}

int oi_surface_shade_ao(const oi_surface_ao_params* p, oi_stream_t stream) {
  OI_TRY(check_surface("oi_surface_shade_ao", p));
  hipLaunchKernelGGL(surface_shade_ao_kernel, dim3(n_blocks(p->N)), dim3(TR_THREADS), 0, oi::as_stream(stream), *p);
  return oi::check_launch("oi_surface_shade_ao");
}

}  // extern "C"
