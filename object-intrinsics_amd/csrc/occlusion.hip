// Soft shadows and ambient occlusion for the sphere-traced renderer (include/oi_occlusion.h), gfx950.
// One thread per secondary ray or pixel, around the library's own sdf-only MLP passes:
//   light_begin / ambient_begin   S sample directions per (light, visible point): a cap about the light's direction, uniform
//                                 in solid angle, or the cosine-weighted hemisphere about the normal; offset along the
//                                 normal, compacted like a step
//   step                          trace_common.h's state machine in its any-hit form: the first occluder ends the ray
//   resolve                       S ray states per light and pixel -> the share that ended MISS
//   shade_ao                      trace_common.h's shading with an occlusion factor on the ambient term
// No float atomics, no scratch; the only atomics are the compaction's integer counters (one add per workgroup).
#include "trace_common.h"
#include "../../include/oi_occlusion.h"

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
  bool traced = false;
  float ox = 0.f, oy = 0.f, oz = 0.f;
  if (q < s.N) {
    const long long lj = q / n_hit, i = q - lj * n_hit;
    const long long l = lj / S;
    const unsigned j = (unsigned)(lj - l * S);
    float nx, ny, nz, dx, dy, dz;
    unit_normal(grad, i, nx, ny, nz);
    traced = occlusion_direction<AMBIENT>(nx, ny, nz, (unsigned)hit_index[i], seed, j, S, lights + l * OI_RELIGHT_LIGHT_FLOATS, radius,
                                          l, w2b, dx, dy, dz);
    ox = __fmaf_rn(bias, nx, hit_points[i * 3 + 0]);
    oy = __fmaf_rn(bias, ny, hit_points[i * 3 + 1]);
    oz = __fmaf_rn(bias, nz, hit_points[i * 3 + 2]);
    float far = unit_sphere_exit(ox, oy, oz, dx, dy, dz);
    if (AMBIENT) far = fminf(far, distance);
    s.rays_o[q * 3 + 0] = ox, s.rays_o[q * 3 + 1] = oy, s.rays_o[q * 3 + 2] = oz;
    s.rays_d[q * 3 + 0] = dx, s.rays_d[q * 3 + 1] = dy, s.rays_d[q * 3 + 2] = dz;
    s.near_[q] = 0.f;
    s.far_[q] = far;
    s.t[q] = 0.f;
    s.status[q] = traced ? OI_TRACE_MARCH : OI_TRACE_BACKFACING;
    s.steps[q] = 0;
    s.side[q] = 0;
    s.bracket[q * 4 + 0] = s.bracket[q * 4 + 1] = s.bracket[q * 4 + 2] = s.bracket[q * 4 + 3] = 0.f;
  }
  const long long slot = wg_slot(traced, s.counts, lds);
  if (traced) {
    s.active[slot] = (int)q;
    s.points[slot * 3 + 0] = ox, s.points[slot * 3 + 1] = oy, s.points[slot * 3 + 2] = oz;  // o + 0 d
  }
}

__global__ void __launch_bounds__(TR_THREADS) occlusion_resolve_kernel(const uint8_t* __restrict__ status,
                                                                       const int* __restrict__ hit_slot, long long N,
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

__global__ void __launch_bounds__(TR_THREADS) surface_shade_ao_kernel(const oi_surface_ao_params p) {
  surface_shade_pixel(p, p.ambient_occlusion);
}

// what the two begin entries share: the state, the counts and the ray layout
int check_begin(const char* what, const oi_trace_state* s, long long n_hit, int L, int S, float bias) {
  int rc = check_state(s, what);
  if (rc != OI_OK) return rc;
  OI_REQUIRE(L >= 1 && L <= OI_RELIGHT_MAX_LIGHTS, "%s: L=%d (1 .. %d lights)", what, L, OI_RELIGHT_MAX_LIGHTS);
  OI_REQUIRE(S >= 1 && S <= OI_OCCLUSION_MAX_SAMPLES, "%s: S=%d (1 .. %d samples)", what, S, OI_OCCLUSION_MAX_SAMPLES);
  OI_REQUIRE(n_hit >= 1 && n_hit < (1ll << 31) && n_hit * L * S == s->N,
             "%s: n_hit=%lld, L=%d, S=%d, N=%lld (N must be L * S * n_hit, below 2^31)", what, n_hit, L, S, s->N);
  OI_REQUIRE(bias >= 0.f && bias < INFINITY, "%s: bias %g (>= 0, finite)", what, (double)bias);
  return OI_OK;
}

}  // namespace

extern "C" {

int oi_occlusion_light_begin(const oi_trace_state* s, const float* hit_points, const float* grad, const int* hit_index,
                             long long n_hit, const float* lights, const float* radius, int L, int S, const float* w2b,
                             float bias, unsigned seed, oi_stream_t stream) {
  int rc = check_begin("oi_occlusion_light_begin", s, n_hit, L, S, bias);
  if (rc != OI_OK) return rc;
  OI_REQUIRE(radius != nullptr, "oi_occlusion_light_begin: null radius (one angular radius per light, device memory)");
  OI_REQUIRE(hit_points && grad && hit_index && lights && w2b, "oi_occlusion_light_begin: null input pointer");
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(trace_clear_counts_kernel, dim3(1), dim3(TR_THREADS), 0, st, s->counts);
  hipLaunchKernelGGL(occlusion_begin_kernel<false>, dim3(n_blocks(s->N)), dim3(TR_THREADS), 0, st, *s, hit_points, grad, hit_index,
                     n_hit, lights, radius, S, w2b, bias, 0.f, seed);
  return oi::check_launch("oi_occlusion_light_begin");
}

int oi_occlusion_ambient_begin(const oi_trace_state* s, const float* hit_points, const float* grad, const int* hit_index,
                               long long n_hit, int S, float bias, float distance, unsigned seed, oi_stream_t stream) {
  int rc = check_begin("oi_occlusion_ambient_begin", s, n_hit, 1, S, bias);
  if (rc != OI_OK) return rc;
  OI_REQUIRE(distance > 0.f && distance < INFINITY, "oi_occlusion_ambient_begin: distance %g (> 0, finite)", (double)distance);
  OI_REQUIRE(hit_points && grad && hit_index, "oi_occlusion_ambient_begin: null input pointer");
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(trace_clear_counts_kernel, dim3(1), dim3(TR_THREADS), 0, st, s->counts);
  hipLaunchKernelGGL(occlusion_begin_kernel<true>, dim3(n_blocks(s->N)), dim3(TR_THREADS), 0, st, *s, hit_points, grad, hit_index,
                     n_hit, (const float*)nullptr, (const float*)nullptr, S, (const float*)nullptr, bias, distance, seed);
  return oi::check_launch("oi_occlusion_ambient_begin");
}

int oi_occlusion_step(const oi_trace_state* s, const float* sdf, long long bound, int k, float tol, float omega,
                      oi_stream_t stream) {
  return launch_step<true>("oi_occlusion_step", s, sdf, bound, k, tol, omega, stream);
}

int oi_occlusion_resolve(const uint8_t* status, const int* hit_slot, long long N, long long n_hit, int L, int S, float* out,
                         oi_stream_t stream) {
  OI_REQUIRE(N >= 1 && N < (1ll << 31) && n_hit >= 0 && n_hit <= N, "oi_occlusion_resolve: N=%lld, n_hit=%lld", N, n_hit);
  OI_REQUIRE(L >= 1 && L <= OI_RELIGHT_MAX_LIGHTS, "oi_occlusion_resolve: L=%d (1 .. %d lights)", L, OI_RELIGHT_MAX_LIGHTS);
  OI_REQUIRE(S >= 1 && S <= OI_OCCLUSION_MAX_SAMPLES, "oi_occlusion_resolve: S=%d (1 .. %d samples)", S, OI_OCCLUSION_MAX_SAMPLES);
  OI_REQUIRE(n_hit * L * S < (1ll << 31), "oi_occlusion_resolve: L * S * n_hit = %lld rays (below 2^31)", n_hit * L * S);
  OI_REQUIRE(hit_slot && out && (status || n_hit == 0), "oi_occlusion_resolve: null pointer");
  hipLaunchKernelGGL(occlusion_resolve_kernel, dim3(n_blocks(N * L)), dim3(TR_THREADS), 0, oi::as_stream(stream), status, hit_slot,
                     N, n_hit, L, S, out);
  return oi::check_launch("oi_occlusion_resolve");
}

int oi_surface_shade_ao(const oi_surface_ao_params* p, oi_stream_t stream) {
  int rc = check_surface("oi_surface_shade_ao", p);
  if (rc != OI_OK) return rc;
  hipLaunchKernelGGL(surface_shade_ao_kernel, dim3(n_blocks(p->N)), dim3(TR_THREADS), 0, oi::as_stream(stream), *p);
  return oi::check_launch("oi_surface_shade_ao");
}

}  // extern "C"
