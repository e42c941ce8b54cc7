// Soft shadows, ambient occlusion and environment lighting between the instances of a scene for gfx950
// (include/oi_scene_light.h): scene.hip's "every ray against every instance" layout with occlusion.hip's
// sampled rays.  Small memory-bound kernels, one thread per ray or scene pixel:
//   point_pixels        the scene pixel of every visible point: the key of its sample sequence
//   occlusion_begin     per occluder instance Sc sampled rays per (light, visible point): the direction drawn once in the
//                       owner's frame (trace_common.h's occlusion_direction, occlusion.hip's own), the owner's ray by
//                       occlusion.hip's expressions, any other instance's moved into its box frame and culled against its
//                       unit sphere (and against `distance` when ambient); both origins are trace_common.h's
//                       offset_origin, the stores and the compaction its write_ray and enter_rays
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

template <bool AMBIENT>
__global__ void __launch_bounds__(TR_THREADS) scene_occlusion_begin_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                           const oi_scene_occlusion_params p) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const int eo = blockIdx.y;  // the occluder
  const oi_trace_state v = element_view(s, eo);
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool entered = false;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (q < s.N) {
    const long long lj = q / p.n_vis, g = q - lj * p.n_vis;
    const long long l = lj / p.Sc;
    const unsigned j = (unsigned)p.j0 + (unsigned)(lj - l * p.Sc);
    const int e = p.elem[g];  // the point's owner
    const long long k = (long long)e * p.n_pad + (g - p.offset[e]);
    const float* We = p.w2b + (long long)e * 16;
    float nx, ny, nz, d[3], o[3];
    unit_normal(p.grad, k, nx, ny, nz);
    const bool traced = occlusion_direction<AMBIENT>(nx, ny, nz, (unsigned)p.pixel[g], p.seed, j, p.S,
                                                     p.lights + l * OI_RELIGHT_LIGHT_FLOATS, p.radius, l, We, d[0], d[1], d[2]);
    offset_origin(p.hit_points + k * 3, p.bias, nx, ny, nz, o[0], o[1], o[2]);
    float near_ = 0.f, far_ = 0.f;
    unsigned status = OI_TRACE_BACKFACING;
    if (traced && e == eo) {
      far_ = unit_sphere_exit(o[0], o[1], o[2], d[0], d[1], d[2]);
      if (AMBIENT) far_ = fminf(far_, p.distance);
      entered = true;
      status = OI_TRACE_MARCH;
    } else if (traced) {
      const float* Wb = p.w2b + (long long)eo * 16;
      float ow[3], dw[3], dd[3];
      offset_origin(p.position + g * 3, p.bias, p.normal[g * 3 + 0], p.normal[g * 3 + 1], p.normal[g * 3 + 2], ow[0], ow[1], ow[2]);
      transform_point(Wb, ow, o);
      rotate_t(We, d, dw);
      rotate(Wb, dw, dd);
      d[0] = dd[0], d[1] = dd[1], d[2] = dd[2];
      entered = unit_sphere_chord(o, d, near_, far_);
      if (AMBIENT) {
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
  OI_REQUIRE(p->n_pad >= 1 && p->n_vis >= 1 && p->n_vis <= sb->E * p->n_pad,
             "%s: n_pad=%lld, n_vis=%lld (n_pad >= 1, 1 <= n_vis <= E * n_pad)", what, p->n_pad, p->n_vis);
  OI_REQUIRE((long long)p->L * p->Sc * p->n_vis == sb->s.N, "%s: L=%d, Sc=%d, n_vis=%lld, N=%lld (N must be L * Sc * n_vis)", what,
             p->L, p->Sc, p->n_vis, sb->s.N);
  OI_TRY(check_bias(what, p->bias));
  OI_REQUIRE(!p->ambient || p->distance > 0.f, "%s: distance %g (> 0; INFINITY is allowed)", what, (double)p->distance);
  OI_REQUIRE(p->hit_points && p->grad && p->offset && p->elem && p->pixel && p->position && p->normal && p->w2b &&
                 (p->ambient || (p->lights && p->radius)),
             "%s: null input pointer", what);
  const hipStream_t st = oi::as_stream(stream);
  const dim3 grid(n_blocks(sb->s.N), sb->E);
  hipLaunchKernelGGL(scene_clear_kernel, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live);
  if (p->ambient)
    hipLaunchKernelGGL(scene_occlusion_begin_kernel<true>, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, *p);
  else
    hipLaunchKernelGGL(scene_occlusion_begin_kernel<false>, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, *p);
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
