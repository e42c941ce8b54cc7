// The secondary rays and the shade of E views in one chain for gfx950 (include/oi_occlusion_batch.h):
// trace.hip's, occlusion.hip's and local_light.hip's single-view kernels with blockIdx.y = element.  Small memory-bound
// kernels, one thread per ray or pixel, around the batched march, which is unchanged:
//   begin     per view the rays of a chunk of samples at its own hits, against its own field: trace_common.h's begin_ray,
//             the one separately compiled body that the single-view begin kernels run too (the hard shadow ray, a sample of
//             the light's cap or of the hemisphere, or one aimed at a local light); n_hit_e is read from the primary batch's
//             counters on the device, the slots behind it are written as ended rays
//   resolve   per view, light and pixel the chunk's rays that ended MISS, accumulated across chunks as integers; the last
//             chunk divides once
//   shade     trace_common.h's shading (surface_shade_pixel, surface_shade_local_at) on every view's slices in one launch
// The state a begin kernel writes and its compaction are trace_common.h's write_ray and enter_rays, as every begin kernel's;
// the clearing of the counters is scene_common.h's.  No float atomics, no scratch; the only atomics are the compaction's
// integer counters (one add and one max per workgroup).
#include "scene_common.h"

#include "../../include/oi_occlusion_batch.h"

namespace {

static_assert(OI_OCCLUSION_BATCH_SHADOW == BEGIN_SHADOW && OI_OCCLUSION_BATCH_CAP == BEGIN_CAP &&
                  OI_OCCLUSION_BATCH_HEMISPHERE == BEGIN_HEMISPHERE && OI_OCCLUSION_BATCH_LOCAL == BEGIN_LOCAL,
              "the header's modes are trace_common.h's ray kinds");

template <int MODE>
__global__ void __launch_bounds__(TR_THREADS) occlusion_batch_begin_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                           const float* __restrict__ hit_points,
                                                                           const float* __restrict__ grad,
                                                                           const int* __restrict__ hit_index,
                                                                           const int* __restrict__ counts, long long N,
                                                                           long long n_pad, int S, int j0, int Sc,
                                                                           const float* __restrict__ lights,
                                                                           const float* __restrict__ radius,
                                                                           const float* __restrict__ w2b, float bias,
                                                                           float distance, unsigned seed) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const long long e = blockIdx.y;
  const oi_trace_state v = element_view(s, e);
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  BeginRay ry = {};  // a slot behind the view's hits: origin, direction, near and far 0, OI_TRACE_MISS (== 0), not entered
  static_assert(OI_TRACE_MISS == 0, "the zero-initialised ray is an ended one");
  if (q < s.N) {
    const long long lj = q / n_pad, i = q - lj * n_pad;
    const long long l = lj / Sc;
    const unsigned j = (unsigned)j0 + (unsigned)(lj - l * Sc);
    if (i < counts[e * OI_TRACE_COUNT_WORDS + N_HIT_WORD])
      ry = begin_ray<MODE>(hit_points + e * n_pad * 3, grad + e * n_pad * 3, hit_index + e * N, i, l, j, S, lights, radius,
                           w2b + e * 16, bias, distance, seed);
    write_ray(v, q, ry.o, ry.d, 0.f, ry.far_, ry.status);
  }
  enter_rays(v, q, ry.entered, ry.o[0], ry.o[1], ry.o[2], lds, live);
}

__global__ void __launch_bounds__(TR_THREADS) occlusion_batch_resolve_kernel(const uint8_t* __restrict__ status,
                                                                             const int* __restrict__ hit_slot,
                                                                             const int* __restrict__ counts, long long N,
                                                                             long long n_pad, int L, int S, int j0, int Sc,
                                                                             int last, int* __restrict__ count,
                                                                             float* __restrict__ out) {
  const long long e = blockIdx.y;
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= N * L) return;
  const long long l = i / N, px = i - l * N;
  const long long slot = hit_slot[e * N + px], n_hit = counts[e * OI_TRACE_COUNT_WORDS + N_HIT_WORD];
  float* __restrict__ dst = out + (e * L + l) * N + px;
  // (the entries behind the view's hits belong to no pixel: pixel px clears entry px with the first chunk, so the array is written whole)
  if (j0 == 0 && px >= n_hit && px < n_pad) count[(e * L + l) * n_pad + px] = 0;
  if (slot < 0 || slot >= n_hit || slot >= n_pad) {  // off the mask (a slot that does not belong to these counts: nothing is read)
    if (last) *dst = 1.0f;
    return;
  }
  int* __restrict__ cnt = count + (e * L + l) * n_pad + slot;
  const uint8_t* __restrict__ st = status + (e * L + l) * Sc * n_pad + slot;
  int c = j0 > 0 ? *cnt : 0;
  for (int jj = 0; jj < Sc; ++jj) c += st[(long long)jj * n_pad] == OI_TRACE_MISS ? 1 : 0;
  *cnt = c;
  if (last) *dst = (float)c / (float)S;
}

// element e's slices of the batched shade parameters: a valid oi_surface_ao_params of one view (a null pointer stays null)
__device__ __forceinline__ oi_surface_ao_params shade_view(const oi_surface_ao_params& p, long long e, long long n_pad) {
  oi_surface_ao_params v = p;
  const long long r = e * p.N, h = e * n_pad * 3;
  v.rays_o = p.rays_o + r * 3, v.rays_d = p.rays_d + r * 3, v.t = p.t + r, v.status = p.status + r, v.hit_slot = p.hit_slot + r;
  v.hit_points = p.hit_points ? p.hit_points + h : nullptr;
  v.grad = p.grad ? p.grad + h : nullptr;
  v.rgb = p.rgb ? p.rgb + h : nullptr;
  v.w2b = p.w2b + e * 16;
  v.visibility = p.visibility ? p.visibility + r * p.L : nullptr;
  v.depth = p.depth ? p.depth + r : nullptr;
  v.mask = p.mask ? p.mask + r : nullptr;
  v.position = p.position ? p.position + r * 3 : nullptr;
  v.normal = p.normal ? p.normal + r * 3 : nullptr;
  v.normal_world = p.normal_world ? p.normal_world + r * 3 : nullptr;
  v.albedo = p.albedo ? p.albedo + r * 3 : nullptr;
  v.image = p.image ? p.image + r * p.L * 3 : nullptr;
  v.ambient_occlusion = p.ambient_occlusion ? p.ambient_occlusion + r : nullptr;
  return v;
}

template <bool LOCAL>
__global__ void __launch_bounds__(TR_THREADS) surface_shade_batch_kernel(const oi_surface_ao_params p, long long n_pad) {
  const oi_surface_ao_params v = shade_view(p, blockIdx.y, n_pad);
  if constexpr (LOCAL) {
    const long long r = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    if (r >= v.N) return;
    surface_shade_local_at(v, v.ambient_occlusion, r, v.status[r] == OI_TRACE_HIT, r, v.N);
  } else {
    surface_shade_pixel(v, v.ambient_occlusion);
  }
}

// the views and the padded hit lists of a primary batch as plain numbers
int check_views(const char* what, int E, long long N, long long n_pad, long long n_pad_min) {
  OI_TRY(check_scene_rays(what, E, N));
  OI_REQUIRE(n_pad >= n_pad_min && n_pad <= N, "%s: n_pad=%lld (%lld <= n_pad <= N=%lld)", what, n_pad, n_pad_min, N);
  return OI_OK;
}

}  // namespace

extern "C" {

int oi_occlusion_batch_begin(const oi_trace_batch* sb, int mode, const float* hit_points, const float* grad,
                             const int* hit_index, const int* counts, long long N, long long n_pad, int L, int S, int j0, int Sc,
                             const float* lights, const float* radius, const float* w2b, float bias, float distance,
                             unsigned seed, oi_stream_t stream) {
  const char* what = "oi_occlusion_batch_begin";
  OI_TRY(check_batch(sb, what));
  OI_REQUIRE(mode >= OI_OCCLUSION_BATCH_SHADOW && mode <= OI_OCCLUSION_BATCH_LOCAL,
             "%s: mode=%d (0 shadow, 1 cap, 2 hemisphere, 3 local)", what, mode);
  OI_TRY(check_chunk(what, L, S, j0, Sc));
  OI_REQUIRE(mode != OI_OCCLUSION_BATCH_SHADOW || (S == 1 && Sc == 1), "%s: S=%d, Sc=%d with the hard shadow ray (both must be 1)",
             what, S, Sc);
  OI_REQUIRE(mode != OI_OCCLUSION_BATCH_HEMISPHERE || L == 1, "%s: L=%d with the hemisphere (one set of rays: L must be 1)", what, L);
  OI_TRY(check_views(what, sb->E, N, n_pad, 1));
  OI_REQUIRE((long long)L * Sc * n_pad == sb->s.N, "%s: L=%d, Sc=%d, n_pad=%lld, N=%lld rays per element (must be L * Sc * n_pad)",
             what, L, Sc, n_pad, sb->s.N);
  OI_TRY(check_bias(what, bias));
  OI_REQUIRE(mode != OI_OCCLUSION_BATCH_HEMISPHERE || distance > 0.f, "%s: distance %g (> 0; INFINITY is allowed)", what,
             (double)distance);
  OI_REQUIRE(hit_points && grad && hit_index && counts, "%s: null input pointer", what);
  OI_REQUIRE(mode == OI_OCCLUSION_BATCH_HEMISPHERE || (lights && w2b), "%s: null input pointer (lights, w2b)", what);
  OI_REQUIRE(mode != OI_OCCLUSION_BATCH_CAP || radius, "%s: null radius (one angular radius per light, device memory)", what);
  const hipStream_t st = oi::as_stream(stream);
  const dim3 grid(n_blocks(sb->s.N), sb->E), block(TR_THREADS);
  hipLaunchKernelGGL(scene_clear_kernel, grid, block, 0, st, sb->s, sb->live);
#define OI_BEGIN_(M)                                                                                                               \
  hipLaunchKernelGGL(occlusion_batch_begin_kernel<M>, grid, block, 0, st, sb->s, sb->live, hit_points, grad, hit_index, counts, N, \
                     n_pad, S, j0, Sc, lights, radius, w2b, bias, distance, seed)
  switch (mode) {
    case OI_OCCLUSION_BATCH_SHADOW: OI_BEGIN_(OI_OCCLUSION_BATCH_SHADOW); break;
    case OI_OCCLUSION_BATCH_CAP: OI_BEGIN_(OI_OCCLUSION_BATCH_CAP); break;
    case OI_OCCLUSION_BATCH_HEMISPHERE: OI_BEGIN_(OI_OCCLUSION_BATCH_HEMISPHERE); break;
    default: OI_BEGIN_(OI_OCCLUSION_BATCH_LOCAL); break;
  }
#undef OI_BEGIN_
  return oi::check_launch(what);
}

int oi_occlusion_batch_resolve(const uint8_t* status, const int* hit_slot, const int* counts, int E, long long N,
                               long long n_pad, int L, int S, int j0, int Sc, int last, int* count, float* out,
                               oi_stream_t stream) {
  const char* what = "oi_occlusion_batch_resolve";
  OI_TRY(check_chunk(what, L, S, j0, Sc));
  OI_TRY(check_views(what, E, N, n_pad, 1));
  OI_REQUIRE((long long)E * L * Sc * n_pad < (1ll << 31), "%s: E * L * Sc * n_pad = %lld rays (below 2^31)", what,
             (long long)E * L * Sc * n_pad);
  OI_REQUIRE(status && hit_slot && counts && count && (out || !last), "%s: null pointer", what);
  hipLaunchKernelGGL(occlusion_batch_resolve_kernel, dim3(n_blocks(N * L), E), dim3(TR_THREADS), 0, oi::as_stream(stream), status,
                     hit_slot, counts, N, n_pad, L, S, j0, Sc, last, count, out);
  return oi::check_launch(what);
}

int oi_surface_shade_batch(const oi_surface_ao_params* p, int E, long long n_pad, int local, oi_stream_t stream) {
  const char* what = "oi_surface_shade_batch";
  OI_REQUIRE(p != nullptr, "%s: null params", what);
  OI_TRY(check_views(what, E, p->N, n_pad, 0));
  oi_surface_ao_params v = *p;
  v.n_hit = n_pad;  // (the single view's rule for the hit arrays, on the padded lists)
  OI_TRY(check_surface(what, &v));
  const dim3 grid(n_blocks(p->N), E);
  if (local) hipLaunchKernelGGL(surface_shade_batch_kernel<true>, grid, dim3(TR_THREADS), 0, oi::as_stream(stream), v, n_pad);
  else hipLaunchKernelGGL(surface_shade_batch_kernel<false>, grid, dim3(TR_THREADS), 0, oi::as_stream(stream), v, n_pad);
  return oi::check_launch(what);
}

}  // extern "C"
