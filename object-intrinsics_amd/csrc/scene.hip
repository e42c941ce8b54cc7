// A scene of many instances for gfx950 (include/oi_scene.h): the layer around the batched trace
// (trace_batch.hip) that makes E instances ONE picture.  Small memory-bound kernels, one thread per ray or scene pixel:
//   begin          the windowed rays of every instance (render.hip's make_ray), the bounding-sphere cull, the state of the
//                  batched trace with the entered rays compacted within their element
//   resolve        per scene pixel the nearest hit among the instances whose window covers it
//   visible        per instance the dense list of the rays that own their pixel: the input of the full MLP pass
//   shade          trace_common.h's per-pixel shading on the owner's slices, the instance map, world positions
//   points         the visible points of all instances as one world-frame list
//   shadow_begin   per occluder instance one shadow ray per (light, visible point): the owner's own ray by trace.hip's
//                  expressions, any other instance's moved into its box frame and culled against its unit sphere
//   visibility     a pixel is lit when its shadow ray missed every instance (scene_common.h's escaped_everywhere)
// The march, the finish, the gather and both MLP passes are the library's own.  The begin kernels store a ray through
// trace_common.h's write_ray and compact through its enter_rays, the first sample point passed from registers (wg_slot:
// one integer atomicAdd and one atomicMax per workgroup); resolve and visibility loop over the elements in a fixed order and
// use no atomics.  No LDS beyond the compaction's counter words, no scratch.
#include "ray_common.h"
#include "scene_common.h"

namespace {

__global__ void __launch_bounds__(TR_THREADS) scene_begin_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                 const float* __restrict__ c2b, const float* __restrict__ kinv,
                                                                 const int* __restrict__ window, int W, int S) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const int e = blockIdx.y;
  const oi_trace_state v = element_view(s, e);
  const long long r = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool entered = false;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (r < s.N) {
    const int j = (int)(r / W), i = (int)(r - (long long)j * W);
    const long long X = (long long)window[e * 2 + 0] + i, Y = (long long)window[e * 2 + 1] + j;
    const bool inside = X >= 0 && X < S && Y >= 0 && Y < S;
    // (a pixel outside the image has no ray: its slot holds pixel (0, 0)'s, never traced)
    const RayOD ry = make_ray(c2b + (long long)e * 16, kinv, 0.f, 0.f, S, inside ? (int)X : 0, inside ? (int)Y : 0);
    float near_ = 0.f, far_ = 0.f;
    entered = unit_sphere_chord(ry.o, ry.d, near_, far_) && inside;
    if (!entered) near_ = far_ = 0.f;
    write_ray(v, r, ry.o, ry.d, near_, far_, entered ? OI_TRACE_MARCH : OI_TRACE_MISS);
    px = __fmaf_rn(near_, ry.d[0], ry.o[0]), py = __fmaf_rn(near_, ry.d[1], ry.o[1]), pz = __fmaf_rn(near_, ry.d[2], ry.o[2]);
  }
  enter_rays(v, r, entered, px, py, pz, lds, live);
}

__global__ void __launch_bounds__(TR_THREADS) scene_resolve_kernel(const oi_trace_state s, int E, const int* __restrict__ window,
                                                                   int W, int S, int* __restrict__ owner,
                                                                   int* __restrict__ owner_ray) {
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= (long long)S * S) return;
  const int Y = (int)(q / S), X = (int)(q - (long long)Y * S);
  int best = -1, best_ray = -1;
  float best_t = INFINITY;
  for (int e = 0; e < E; ++e) {  // window: wave-uniform reads
    const long long i = (long long)X - window[e * 2 + 0], j = (long long)Y - window[e * 2 + 1];
    if (i < 0 || i >= W || j < 0 || j >= W) continue;
    const long long r = j * W + i, g = (long long)e * s.N + r;
    if (s.status[g] != OI_TRACE_HIT) continue;
    const float t = s.t[g];
    if (best < 0 || t < best_t) best = e, best_ray = (int)r, best_t = t;  // equal t: the lowest element index stays
  }
  owner[q] = best;
  owner_ray[q] = best_ray;
}

__global__ void __launch_bounds__(TR_THREADS) scene_clear_hits_kernel(int* __restrict__ counts, int* __restrict__ live, int E) {
  clear_hit_words(counts, live, E);
}

__global__ void __launch_bounds__(TR_THREADS) scene_visible_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                   const int* __restrict__ owner,
                                                                   const int* __restrict__ window, int W, int S,
                                                                   int* __restrict__ vis_index, int* __restrict__ vis_slot) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const int e = blockIdx.y;
  const long long r = (long long)blockIdx.x * TR_THREADS + threadIdx.x, base = (long long)e * s.N;
  bool mine = false;
  if (r < s.N) {
    const int j = (int)(r / W), i = (int)(r - (long long)j * W);
    const long long X = (long long)window[e * 2 + 0] + i, Y = (long long)window[e * 2 + 1] + j;
    mine = X >= 0 && X < S && Y >= 0 && Y < S && owner[Y * S + X] == e;
  }
  const long long slot = wg_slot(mine, s.counts + (long long)e * OI_TRACE_COUNT_WORDS + N_HIT_WORD, lds, live + N_HIT_WORD);
  if (r < s.N) vis_slot[base + r] = mine ? (int)slot : -1;
  if (mine) vis_index[base + slot] = (int)r;
}

__global__ void __launch_bounds__(TR_THREADS) scene_shade_kernel(const oi_scene_shade_params p) { scene_shade_pixel(p, nullptr); }

__global__ void __launch_bounds__(TR_THREADS) scene_points_kernel(const int* __restrict__ counts,
                                                                  const float* __restrict__ hit_points,
                                                                  const float* __restrict__ grad, long long n_pad,
                                                                  const int* __restrict__ offset, long long n_vis,
                                                                  const float* __restrict__ b2w, const float* __restrict__ w2b,
                                                                  float* __restrict__ position, float* __restrict__ normal,
                                                                  int* __restrict__ elem) {
  const int e = blockIdx.y;
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= n_pad || i >= counts[(long long)e * OI_TRACE_COUNT_WORDS + N_HIT_WORD]) return;
  const long long g = (long long)offset[e] + i, k = (long long)e * n_pad + i;
  if (g >= n_vis) return;  // (offsets that do not belong to these counts: nothing is written outside the lists)
  float w[3];
  transform_point(b2w + (long long)e * 16, hit_points + k * 3, w);
  float n[3];
  unit_normal(grad, k, n[0], n[1], n[2]);
  to_world(w2b + (long long)e * 16, n[0], n[1], n[2], normal[g * 3 + 0], normal[g * 3 + 1], normal[g * 3 + 2]);
  position[g * 3 + 0] = w[0], position[g * 3 + 1] = w[1], position[g * 3 + 2] = w[2];
  elem[g] = e;
}

__global__ void __launch_bounds__(TR_THREADS) scene_shadow_begin_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                        const float* __restrict__ hit_points,
                                                                        const float* __restrict__ grad, long long n_pad,
                                                                        const int* __restrict__ offset,
                                                                        const int* __restrict__ elem,
                                                                        const float* __restrict__ position,
                                                                        const float* __restrict__ normal, long long n_vis,
                                                                        const float* __restrict__ lights,
                                                                        const float* __restrict__ w2b, float bias) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const int eo = blockIdx.y;  // the occluder
  const oi_trace_state v = element_view(s, eo);
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool entered = false;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (q < s.N) {
    const long long l = q / n_vis, g = q - l * n_vis;
    const int e = elem[g];  // the point's owner
    const float* lt = lights + l * OI_RELIGHT_LIGHT_FLOATS;
    const ShadowRay own = shadow_ray(hit_points + (long long)e * n_pad * 3, grad + (long long)e * n_pad * 3, g - offset[e], lt,
                                     w2b + (long long)e * 16, bias);
    float o[3] = {own.o[0], own.o[1], own.o[2]}, d[3] = {own.l[0], own.l[1], own.l[2]}, near_ = 0.f, far_ = own.far_;
    unsigned status = OI_TRACE_BACKFACING;
    if (own.traced && e == eo) {
      entered = true;
      status = OI_TRACE_MARCH;
    } else if (own.traced) {
      const float* Wb = w2b + (long long)eo * 16;
      float ow[3];
      offset_origin(position + g * 3, bias, normal[g * 3 + 0], normal[g * 3 + 1], normal[g * 3 + 2], ow[0], ow[1], ow[2]);
      transform_point(Wb, ow, o);
      light_dir(lt, Wb, d[0], d[1], d[2]);
      entered = unit_sphere_chord(o, d, near_, far_);
      status = entered ? OI_TRACE_MARCH : OI_TRACE_MISS;
    }
    if (!entered) near_ = far_ = 0.f;
    write_ray(v, q, o, d, near_, far_, status);
    px = __fmaf_rn(near_, d[0], o[0]), py = __fmaf_rn(near_, d[1], o[1]), pz = __fmaf_rn(near_, d[2], o[2]);
  }
  enter_rays(v, q, entered, px, py, pz, lds, live);
}

__global__ void __launch_bounds__(TR_THREADS) scene_visibility_kernel(const uint8_t* __restrict__ status,
                                                                      const int* __restrict__ owner,
                                                                      const int* __restrict__ owner_ray,
                                                                      const int* __restrict__ vis_slot,
                                                                      const int* __restrict__ offset, int E, long long N, int L,
                                                                      long long n_vis, long long M, float* __restrict__ vis) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= M * L) return;
  const long long l = i / M, q = i - l * M;
  const int e = owner[q];
  float out = 1.0f;
  if (e >= 0) {
    const long long g = (long long)offset[e] + vis_slot[(long long)e * N + owner_ray[q]];
    out = escaped_everywhere(status, E, (long long)L * n_vis, l * n_vis + g) ? 1.0f : 0.0f;
  }
  vis[i] = out;
}

inline int check_scene(const oi_trace_batch* b, int W, int S, const char* what) {
  OI_TRY(check_batch(b, what));
  OI_REQUIRE(W >= 1 && (long long)W * W == b->s.N, "%s: W=%d, N=%lld rays per element (N must be W * W)", what, W, b->s.N);
  return check_resolution(what, "S", S);
}

}  // namespace

extern "C" {

int oi_scene_begin(const oi_trace_batch* b, const float* c2b, const float* kinv, const int* window, int W, int S,
                   oi_stream_t stream) {
  const char* what = "oi_scene_begin";
  OI_TRY(check_scene(b, W, S, what));
  OI_REQUIRE(c2b && kinv && window, "%s: null input pointer", what);
  const hipStream_t st = oi::as_stream(stream);
  const dim3 grid(n_blocks(b->s.N), b->E);
  hipLaunchKernelGGL(scene_clear_kernel, grid, dim3(TR_THREADS), 0, st, b->s, b->live);
  hipLaunchKernelGGL(scene_begin_kernel, grid, dim3(TR_THREADS), 0, st, b->s, b->live, c2b, kinv, window, W, S);
  return oi::check_launch(what);
}

int oi_scene_resolve(const oi_trace_batch* b, const int* window, int W, int S, int* owner, int* owner_ray,
                     oi_stream_t stream) {
  const char* what = "oi_scene_resolve";
  OI_TRY(check_scene(b, W, S, what));
  OI_REQUIRE(window && owner && owner_ray, "%s: null pointer", what);
  hipLaunchKernelGGL(scene_resolve_kernel, dim3(n_blocks((long long)S * S)), dim3(TR_THREADS), 0, oi::as_stream(stream), b->s,
                     b->E, window, W, S, owner, owner_ray);
  return oi::check_launch(what);
}

int oi_scene_visible(const oi_trace_batch* b, const int* owner, const int* window, int W, int S, int* vis_index,
                     int* vis_slot, oi_stream_t stream) {
  const char* what = "oi_scene_visible";
  OI_TRY(check_scene(b, W, S, what));
  OI_REQUIRE(owner && window && vis_index && vis_slot, "%s: null pointer", what);
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(scene_clear_hits_kernel, dim3(n_blocks(b->E)), dim3(TR_THREADS), 0, st, b->s.counts, b->live, b->E);
  hipLaunchKernelGGL(scene_visible_kernel, dim3(n_blocks(b->s.N), b->E), dim3(TR_THREADS), 0, st, b->s, b->live, owner, window,
                     W, S, vis_index, vis_slot);
  return oi::check_launch(what);
}

int oi_scene_shade(const oi_scene_shade_params* p, oi_stream_t stream) {
  const char* what = "oi_scene_shade";
  OI_TRY(check_scene_shade(p, what));
  hipLaunchKernelGGL(scene_shade_kernel, dim3(n_blocks((long long)p->S * p->S)), dim3(TR_THREADS), 0, oi::as_stream(stream), *p);
  return oi::check_launch(what);
}

int oi_scene_points(const oi_trace_batch* b, const float* hit_points, const float* grad, long long n_pad, const int* offset,
                    long long n_vis, const float* b2w, const float* w2b, float* position, float* normal, int* elem,
                    oi_stream_t stream) {
  const char* what = "oi_scene_points";
  OI_TRY(check_batch(b, what));
  OI_REQUIRE(n_pad >= 1 && n_pad <= b->s.N, "%s: n_pad=%lld (1 <= n_pad <= N=%lld)", what, n_pad, b->s.N);
  OI_REQUIRE(n_vis >= 1 && n_vis <= b->E * n_pad, "%s: n_vis=%lld (1 <= n_vis <= E * n_pad = %lld)", what, n_vis, b->E * n_pad);
  OI_REQUIRE(hit_points && grad && offset && b2w && w2b && position && normal && elem, "%s: null pointer", what);
  hipLaunchKernelGGL(scene_points_kernel, dim3(n_blocks(n_pad), b->E), dim3(TR_THREADS), 0, oi::as_stream(stream), b->s.counts,
                     hit_points, grad, n_pad, offset, n_vis, b2w, w2b, position, normal, elem);
  return oi::check_launch(what);
}

int oi_scene_shadow_begin(const oi_trace_batch* sb, const float* hit_points, const float* grad, long long n_pad,
                          const int* offset, const int* elem, const float* position, const float* normal, long long n_vis,
                          const float* lights, int L, const float* w2b, float bias, oi_stream_t stream) {
  const char* what = "oi_scene_shadow_begin";
  OI_TRY(check_batch(sb, what));
  OI_TRY(check_lights(what, L));
  OI_REQUIRE(n_vis >= 1 && n_vis * L == sb->s.N, "%s: n_vis=%lld, L=%d, N=%lld (N must be L * n_vis)", what, n_vis, L, sb->s.N);
  OI_REQUIRE(n_pad >= 1 && n_vis <= sb->E * n_pad, "%s: n_pad=%lld, n_vis=%lld (n_pad >= 1, n_vis <= E * n_pad)", what, n_pad,
             n_vis);
  OI_TRY(check_bias(what, bias));
  OI_REQUIRE(hit_points && grad && offset && elem && position && normal && lights && w2b, "%s: null input pointer", what);
  const hipStream_t st = oi::as_stream(stream);
  const dim3 grid(n_blocks(sb->s.N), sb->E);
  hipLaunchKernelGGL(scene_clear_kernel, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live);
  hipLaunchKernelGGL(scene_shadow_begin_kernel, grid, dim3(TR_THREADS), 0, st, sb->s, sb->live, hit_points, grad, n_pad, offset,
                     elem, position, normal, n_vis, lights, w2b, bias);
  return oi::check_launch(what);
}

int oi_scene_visibility(const uint8_t* shadow_status, const int* owner, const int* owner_ray, const int* vis_slot,
                        const int* offset, int E, long long N, int L, long long n_vis, int S, float* visibility,
                        oi_stream_t stream) {
  const char* what = "oi_scene_visibility";
  OI_TRY(check_scene_rays(what, E, N));
  OI_TRY(check_lights(what, L));
  OI_TRY(check_resolution(what, "S", S));
  OI_REQUIRE(n_vis >= 0 && n_vis <= E * N && (long long)E * L * n_vis < (1ll << 31),
             "%s: n_vis=%lld (0 <= n_vis <= E * N, E * L * n_vis < 2^31)", what, n_vis);
  OI_REQUIRE(owner && owner_ray && visibility && (n_vis == 0 || (shadow_status && vis_slot && offset)), "%s: null pointer", what);
  const long long M = (long long)S * S;
  hipLaunchKernelGGL(scene_visibility_kernel, dim3(n_blocks(M * L)), dim3(TR_THREADS), 0, oi::as_stream(stream), shadow_status,
                     owner, owner_ray, vis_slot, offset, E, N, L, n_vis, M, visibility);
  return oi::check_launch(what);
}

}  // extern "C"
