// Intrinsic mesh export: the vertex pass between the marching cubes of mesh.hip and a mesh file with normals and albedo
// (include/oi_mesh_attr.h).  Four small memory-bound kernels, one thread per vertex, around the
// library's own full MLP forward (oi_sdf_mlp_fwd, called by the host between them):
//   world      index-space vertex -> world point through the axis arrays oi_sdf_lattice took; clears the flags
//   newton     one projection step onto sdf = -threshold from the (sdf, gradient) of the last MLP pass, limited to half a
//              cell around the marching-cubes position; the residual before the step; sticky flags
//   finalize   unit normal, albedo, the last residual, optionally the interleaved 27-byte vertex record
//   record     the record alone from caller-supplied normals and colours
// No atomics, no scratch, every output element written by exactly one thread (the record: staged in LDS per workgroup and
// written out as whole dwords, since 27-byte records are not dword aligned).  64-bit indexing: V * 27 exceeds 2^31.
#include "oi_common.h"
#include "mesh_quant.h"
#include "../../include/oi_mesh_attr.h"

namespace {

constexpr int MA_THREADS = 256;
constexpr int MA_REC = OI_MESH_RECORD_BYTES;
constexpr int MA_REC_BLOCK = MA_THREADS * MA_REC;  // 6912 bytes: a whole number of dwords per workgroup
static_assert(MA_REC_BLOCK % 4 == 0, "a workgroup's records must end on a dword");

__device__ __forceinline__ bool finite_(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// one coordinate: x[i] exactly on a lattice plane, else the linear interpolation along the edge; never reads x[n]
__device__ __forceinline__ float axis_world(const float* __restrict__ x, int n, float c) {
  int i = (int)floorf(c);
  i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);   // (a NaN coordinate lands on 0)
  const float t = c - (float)i;
  const float x0 = x[i];
  if (t == 0.f || i + 1 > n - 1) return x0;
  return __fmaf_rn(t, x[i + 1] - x0, x0);
}

__global__ void __launch_bounds__(MA_THREADS) mesh_vertex_world_kernel(const float* __restrict__ vi, long long V,
                                                                       const float* __restrict__ xs,
                                                                       const float* __restrict__ ys,
                                                                       const float* __restrict__ zs, int nx, int ny, int nz,
                                                                       float* __restrict__ pos,
                                                                       uint8_t* __restrict__ flags) {
  const long long v = (long long)blockIdx.x * MA_THREADS + threadIdx.x;
  if (v >= V) return;
  pos[v * 3 + 0] = axis_world(xs, nx, vi[v * 3 + 0]);
  pos[v * 3 + 1] = axis_world(ys, ny, vi[v * 3 + 1]);
  pos[v * 3 + 2] = axis_world(zs, nz, vi[v * 3 + 2]);
  if (flags) flags[v] = 0;
}

__global__ void __launch_bounds__(MA_THREADS) mesh_newton_kernel(float* __restrict__ pos, const float* __restrict__ pos0,
                                                                 const float* __restrict__ sdf,
                                                                 const float* __restrict__ grad, long long V,
                                                                 float threshold, float lx, float ly, float lz,
                                                                 float* __restrict__ residual,
                                                                 uint8_t* __restrict__ flags) {
  const long long v = (long long)blockIdx.x * MA_THREADS + threadIdx.x;
  if (v >= V) return;
  const float s = sdf[v] + threshold;
  const float gx = grad[v * 3 + 0], gy = grad[v * 3 + 1], gz = grad[v * 3 + 2];
  const float g2 = gx * gx + gy * gy + gz * gz;
  if (residual) residual[v] = fabsf(s) / sqrtf(g2);
  unsigned f = 0;
  if (!(finite_(s) && finite_(gx) && finite_(gy) && finite_(gz))) {
    f = OI_MESH_FLAG_NONFINITE;
  } else if (g2 < OI_MESH_GRAD_EPS) {
    f = OI_MESH_FLAG_SMALL_GRADIENT;
  } else {
    const float k = s / fmaxf(g2, OI_MESH_GRAD_EPS);
    const float cx = pos[v * 3 + 0] - k * gx, cy = pos[v * 3 + 1] - k * gy, cz = pos[v * 3 + 2] - k * gz;
    // (negated <=: a NaN candidate counts as outside)
    if (!(fabsf(cx - pos0[v * 3 + 0]) <= lx && fabsf(cy - pos0[v * 3 + 1]) <= ly && fabsf(cz - pos0[v * 3 + 2]) <= lz)) {
      f = OI_MESH_FLAG_LIMIT;
    } else {
      pos[v * 3 + 0] = cx;
      pos[v * 3 + 1] = cy;
      pos[v * 3 + 2] = cz;
    }
  }
  if (f) flags[v] = (uint8_t)(flags[v] | f);
}

__device__ __forceinline__ void put_f32(unsigned char* dst, float v) {
  const unsigned w = __float_as_uint(v);
  dst[0] = (unsigned char)w, dst[1] = (unsigned char)(w >> 8), dst[2] = (unsigned char)(w >> 16), dst[3] = (unsigned char)(w >> 24);
}
using oi::quant8;   // (mesh_quant.h: the byte atlases of mesh_tex.hip hold the same rule)

// The workgroup's records: thread t has staged vertex v0 + t at lds + 27 t (when it has a vertex); the bytes go out as
// dwords (the workgroup's first byte is 6912 * blockIdx.x: dword aligned when `record` is), the last 1..3 of the mesh as bytes.
__device__ __forceinline__ void flush_records(const unsigned* lds32, unsigned char* __restrict__ record, long long V) {
  __syncthreads();
  const long long v0 = (long long)blockIdx.x * MA_THREADS;
  const long long left = V - v0;
  const int nbytes = (int)(left < MA_THREADS ? left : MA_THREADS) * MA_REC;
  unsigned char* out = record + v0 * MA_REC;
  unsigned* out32 = reinterpret_cast<unsigned*>(out);
  for (int i = threadIdx.x; i < nbytes / 4; i += MA_THREADS) out32[i] = lds32[i];
  const int done = nbytes & ~3;
  if ((int)threadIdx.x < nbytes - done)
    out[done + threadIdx.x] = reinterpret_cast<const unsigned char*>(lds32)[done + threadIdx.x];
}

__device__ __forceinline__ void stage_record(unsigned* lds32, const float p[3], const float n[3], const float c[3]) {
  unsigned char* r = reinterpret_cast<unsigned char*>(lds32) + threadIdx.x * MA_REC;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    put_f32(r + 4 * a, p[a]);
    put_f32(r + 12 + 4 * a, n[a]);
    r[24 + a] = quant8(c[a]);
  }
}

__global__ void __launch_bounds__(MA_THREADS) mesh_attr_finalize_kernel(const float* __restrict__ pos,
                                                                        const float* __restrict__ sdf,
                                                                        const float* __restrict__ grad,
                                                                        const float* __restrict__ rgb, long long V,
                                                                        float threshold, float* __restrict__ normals,
                                                                        float* __restrict__ albedo,
                                                                        float* __restrict__ residual,
                                                                        unsigned char* __restrict__ record) {
  __shared__ unsigned lds32[MA_REC_BLOCK / 4];
  const long long v = (long long)blockIdx.x * MA_THREADS + threadIdx.x;
  if (v < V) {
    const float g[3] = {grad[v * 3 + 0], grad[v * 3 + 1], grad[v * 3 + 2]};
    const float c[3] = {rgb[v * 3 + 0], rgb[v * 3 + 1], rgb[v * 3 + 2]};
    const float gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    const float inv = 1.0f / fmaxf(gn, 1e-6f);
    const float n[3] = {g[0] * inv, g[1] * inv, g[2] * inv};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (normals) normals[v * 3 + a] = n[a];
      if (albedo) albedo[v * 3 + a] = c[a];
    }
    if (residual) residual[v] = fabsf(sdf[v] + threshold) / gn;
    if (record) {
      const float p[3] = {pos[v * 3 + 0], pos[v * 3 + 1], pos[v * 3 + 2]};
      stage_record(lds32, p, n, c);
    }
  }
  if (record) flush_records(lds32, record, V);  // uniform over the workgroup
}

__global__ void __launch_bounds__(MA_THREADS) mesh_vertex_record_kernel(const float* __restrict__ pos,
                                                                        const float* __restrict__ normals,
                                                                        const float* __restrict__ rgb, long long V,
                                                                        unsigned char* __restrict__ record) {
  __shared__ unsigned lds32[MA_REC_BLOCK / 4];
  const long long v = (long long)blockIdx.x * MA_THREADS + threadIdx.x;
  if (v < V) {
    const float p[3] = {pos[v * 3 + 0], pos[v * 3 + 1], pos[v * 3 + 2]};
    const float n[3] = {normals[v * 3 + 0], normals[v * 3 + 1], normals[v * 3 + 2]};
    const float c[3] = {rgb[v * 3 + 0], rgb[v * 3 + 1], rgb[v * 3 + 2]};
    stage_record(lds32, p, n, c);
  }
  flush_records(lds32, record, V);
}

int check_count(long long V, const char* what) {
  OI_REQUIRE(V >= 0 && V < (1ll << 31), "%s: V=%lld vertices (0 <= V < 2^31)", what, V);
  return OI_OK;
}

inline unsigned n_blocks(long long V) { return (unsigned)((V + MA_THREADS - 1) / MA_THREADS); }

}  // namespace

extern "C" {

int oi_mesh_vertex_world(const float* verts_index, long long V, const float* xs, const float* ys, const float* zs, int nx,
                         int ny, int nz, float* pos, uint8_t* flags, oi_stream_t stream) {
  int rc = check_count(V, "oi_mesh_vertex_world");
  if (rc != OI_OK) return rc;
  OI_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "oi_mesh_vertex_world: lattice %d x %d x %d (every axis needs 2 points)", nx, ny,
             nz);
  OI_REQUIRE(xs && ys && zs, "oi_mesh_vertex_world: null axis array");
  if (V == 0) return OI_OK;
  OI_REQUIRE(verts_index && pos, "oi_mesh_vertex_world: null pointer");
  hipLaunchKernelGGL(mesh_vertex_world_kernel, dim3(n_blocks(V)), dim3(MA_THREADS), 0, oi::as_stream(stream), verts_index, V,
                     xs, ys, zs, nx, ny, nz, pos, flags);
  return oi::check_launch("oi_mesh_vertex_world");
}

int oi_mesh_newton(float* pos, const float* pos0, const float* sdf, const float* grad, long long V, float threshold,
                   float limit_x, float limit_y, float limit_z, float* residual, uint8_t* flags, oi_stream_t stream) {
  int rc = check_count(V, "oi_mesh_newton");
  if (rc != OI_OK) return rc;
  OI_REQUIRE(threshold == threshold && limit_x >= 0.f && limit_y >= 0.f && limit_z >= 0.f,
             "oi_mesh_newton: threshold %g, limits %g %g %g (a number; limits >= 0)", (double)threshold, (double)limit_x,
             (double)limit_y, (double)limit_z);
  if (V == 0) return OI_OK;
  OI_REQUIRE(pos && pos0 && sdf && grad && flags, "oi_mesh_newton: null pointer");
  hipLaunchKernelGGL(mesh_newton_kernel, dim3(n_blocks(V)), dim3(MA_THREADS), 0, oi::as_stream(stream), pos, pos0, sdf, grad, V,
                     threshold, limit_x, limit_y, limit_z, residual, flags);
  return oi::check_launch("oi_mesh_newton");
}

int oi_mesh_attr_finalize(const float* pos, const float* sdf, const float* grad, const float* rgb, long long V,
                          float threshold, float* normals, float* albedo, float* residual, void* record,
                          oi_stream_t stream) {
  int rc = check_count(V, "oi_mesh_attr_finalize");
  if (rc != OI_OK) return rc;
  OI_REQUIRE(threshold == threshold, "oi_mesh_attr_finalize: threshold is NaN");
  OI_REQUIRE((reinterpret_cast<uintptr_t>(record) & 3u) == 0, "oi_mesh_attr_finalize: record must be 4-byte aligned");
  if (V == 0) return OI_OK;
  OI_REQUIRE(grad && rgb && (!residual || sdf) && (!record || pos), "oi_mesh_attr_finalize: null pointer");
  hipLaunchKernelGGL(mesh_attr_finalize_kernel, dim3(n_blocks(V)), dim3(MA_THREADS), 0, oi::as_stream(stream), pos, sdf, grad,
                     rgb, V, threshold, normals, albedo, residual, reinterpret_cast<unsigned char*>(record));
  return oi::check_launch("oi_mesh_attr_finalize");
}

int oi_mesh_vertex_record(const float* pos, const float* normals, const float* rgb, long long V, void* record,
                          oi_stream_t stream) {
  int rc = check_count(V, "oi_mesh_vertex_record");
  if (rc != OI_OK) return rc;
  OI_REQUIRE((reinterpret_cast<uintptr_t>(record) & 3u) == 0, "oi_mesh_vertex_record: record must be 4-byte aligned");
  if (V == 0) return OI_OK;
  OI_REQUIRE(pos && normals && rgb && record, "oi_mesh_vertex_record: null pointer");
  hipLaunchKernelGGL(mesh_vertex_record_kernel, dim3(n_blocks(V)), dim3(MA_THREADS), 0, oi::as_stream(stream), pos, normals,
                     rgb, V, reinterpret_cast<unsigned char*>(record));
  return oi::check_launch("oi_mesh_vertex_record");
}

}  // extern "C"
