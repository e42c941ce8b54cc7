// Textured mesh export: the per-triangle atlas of include/oi_mesh_tex.h, gfx950.  Three small
// memory-bound kernels around the vertex pass's own chain (oi_sdf_mlp_fwd, oi_mesh_newton, oi_mesh_attr_finalize, called by
// the host between them), one thread per corner or per texel:
//   uv       the texture coordinates of every corner
//   points   the planar point of every texel of a chunk of triangles; clears the flags
//   store    the finalized normals and colours of a chunk to their pixels of up to four atlases
// No atomics, no scratch, no LDS; every output element is written by exactly one thread (the byte atlases: three byte
// stores per texel, no two threads share a byte).  64-bit indexing: F * n_T and the atlas' byte offsets pass 2^31.
#include "oi_common.h"
#include "mesh_quant.h"
#include "../../include/oi_mesh_tex.h"

namespace {

constexpr int MT_THREADS = 256;

// The atlas of include/oi_mesh_tex.h, host side.  -> false when F or T is out of range (nothing is written then).
struct Layout {
  int W, H, cols;
};
bool layout_of(long long F, int T, Layout* l) {
  if (F < 0 || F >= (1ll << 31) || T < OI_TEX_MIN_TEXEL || T > OI_TEX_MAX_TEXEL) return false;
  const long long ncells = (F + 1) >> 1;
  long long cols = 1;
  while (cols * cols < ncells) ++cols;   // at most 32768 steps, host only
  long long rows = (ncells + cols - 1) / cols;
  if (rows < 1) rows = 1;
  l->cols = (int)cols;
  l->W = (int)(cols * (T + 1));
  l->H = (int)(rows * T);
  return true;
}

// texel k of a triangle -> local (i, j): rows of falling length T, T - 1, .. 1.  Counted from the end the rows have the
// lengths 1, 2, 3, ..: r = n_T - 1 - k lies in row q from the end with q (q + 1) / 2 <= r < (q + 1)(q + 2) / 2.
__device__ __forceinline__ void texel_ij(int k, int T, int* i, int* j) {
  const int r = T * (T + 1) / 2 - 1 - k;
  int q = (int)((sqrtf(8.f * (float)r + 1.f) - 1.f) * 0.5f);   // r <= 2079: exact up to the correction below
  while (q * (q + 1) / 2 > r) --q;
  while ((q + 1) * (q + 2) / 2 <= r) ++q;
  *j = T - 1 - q;
  *i = k - (*j * T - *j * (*j - 1) / 2);
}

__global__ void __launch_bounds__(MT_THREADS) tex_uv_kernel(long long F, int T, int cols, float W, float H,
                                                            float* __restrict__ uv) {
  const long long idx = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
  if (idx >= 3 * F) return;
  const long long f = idx / 3;
  const int m = (int)(idx - 3 * f);
  const long long c = f >> 1;
  const float x0 = (float)((c % cols) * (T + 1)), y0 = (float)((c / cols) * T);
  const float cu = m == 1 ? (float)(T - 2) : 0.f, cv = m == 2 ? (float)(T - 2) : 0.f;
  float x, y;
  if (f & 1) {
    x = x0 + (float)T + 0.5f - cu;
    y = y0 + (float)T - 0.5f - cv;
  } else {
    x = x0 + 0.5f + cu;
    y = y0 + 0.5f + cv;
  }
  uv[idx * 2 + 0] = x / W;
  uv[idx * 2 + 1] = 1.f - y / H;
}

__global__ void __launch_bounds__(MT_THREADS) tex_points_kernel(const float* __restrict__ pos,
                                                                const int* __restrict__ triangles, long long f0,
                                                                long long n, int T, float* __restrict__ out,
                                                                uint8_t* __restrict__ flags) {
  const long long idx = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
  if (idx >= n) return;
  const int nT = T * (T + 1) / 2;
  const long long fl = idx / nT;
  int i, j;
  texel_ij((int)(idx - fl * nT), T, &i, &j);
  const float d = (float)(T - 2);
  const float b1 = __fdiv_rn((float)i, d), b2 = __fdiv_rn((float)j, d);
  const float b0 = __fsub_rn(__fsub_rn(1.f, b1), b2);
  const int* tri = triangles + (f0 + fl) * 3;
  const float* v0 = pos + (long long)tri[0] * 3;
  const float* v1 = pos + (long long)tri[1] * 3;
  const float* v2 = pos + (long long)tri[2] * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) out[idx * 3 + a] = __fmaf_rn(b2, v2[a], __fmaf_rn(b1, v1[a], __fmul_rn(b0, v0[a])));
  if (flags) flags[idx] = 0;
}

__global__ void __launch_bounds__(MT_THREADS) tex_store_kernel(const float* __restrict__ normals,
                                                               const float* __restrict__ rgb, long long f0, long long n,
                                                               int T, int cols, int W, float* __restrict__ albedo_f32,
                                                               float* __restrict__ normal_f32,
                                                               unsigned char* __restrict__ albedo_u8,
                                                               unsigned char* __restrict__ normal_u8) {
  const long long idx = (long long)blockIdx.x * MT_THREADS + threadIdx.x;
  if (idx >= n) return;
  const int nT = T * (T + 1) / 2;
  const long long fl = idx / nT;
  int i, j;
  texel_ij((int)(idx - fl * nT), T, &i, &j);
  const long long f = f0 + fl, c = f >> 1;
  const int x0 = (int)(c % cols) * (T + 1), y0 = (int)(c / cols) * T;
  const int x = (f & 1) ? x0 + T - i : x0 + i, y = (f & 1) ? y0 + T - 1 - j : y0 + j;
  const long long px = ((long long)y * W + x) * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float cc = rgb[idx * 3 + a], nn = normals[idx * 3 + a];
    if (albedo_f32) albedo_f32[px + a] = cc;
    if (normal_f32) normal_f32[px + a] = nn;
    if (albedo_u8) albedo_u8[px + a] = oi::quant8(cc);
    if (normal_u8) normal_u8[px + a] = oi::quant8(__fmaf_rn(nn, 0.5f, 0.5f));
  }
}

// a chunk: 0 <= f0, 0 <= nf, nf * n_T < 2^31 (T is checked before)
int check_chunk(long long f0, long long nf, int T, const char* what) {
  OI_REQUIRE(T >= OI_TEX_MIN_TEXEL && T <= OI_TEX_MAX_TEXEL, "%s: texel size T=%d (%d <= T <= %d)", what, T, OI_TEX_MIN_TEXEL,
             OI_TEX_MAX_TEXEL);
  OI_REQUIRE(f0 >= 0 && f0 < (1ll << 31) && nf >= 0 && nf < (1ll << 31) && nf * (T * (T + 1) / 2) < (1ll << 31),
             "%s: chunk f0=%lld nf=%lld at T=%d (0 <= f0, 0 <= nf, nf * n_T < 2^31)", what, f0, nf, T);
  return OI_OK;
}

inline unsigned n_blocks(long long n) { return (unsigned)((n + MT_THREADS - 1) / MT_THREADS); }

}  // namespace

extern "C" {

int oi_tex_layout(long long F, int T, int* W, int* H, int* cols) {
  OI_REQUIRE(T >= OI_TEX_MIN_TEXEL && T <= OI_TEX_MAX_TEXEL, "oi_tex_layout: texel size T=%d (%d <= T <= %d)", T,
             OI_TEX_MIN_TEXEL, OI_TEX_MAX_TEXEL);
  Layout l;
  OI_REQUIRE(layout_of(F, T, &l), "oi_tex_layout: F=%lld triangles (0 <= F < 2^31)", F);
  if (W) *W = l.W;
  if (H) *H = l.H;
  if (cols) *cols = l.cols;
  OI_REQUIRE(l.W <= OI_TEX_MAX_SIZE && l.H <= OI_TEX_MAX_SIZE,
             "oi_tex_layout: the atlas of %lld triangles at T=%d is %d x %d texels, above %d: use a smaller texel size", F, T,
             l.W, l.H, OI_TEX_MAX_SIZE);
  return OI_OK;
}

int oi_tex_uv(long long F, int T, float* uv, oi_stream_t stream) {
  Layout l;
  int rc = oi_tex_layout(F, T, &l.W, &l.H, &l.cols);
  if (rc != OI_OK) return rc;
  if (F == 0) return OI_OK;
  OI_REQUIRE(uv, "oi_tex_uv: null pointer");
  hipLaunchKernelGGL(tex_uv_kernel, dim3(n_blocks(3 * F)), dim3(MT_THREADS), 0, oi::as_stream(stream), F, T, l.cols,
                     (float)l.W, (float)l.H, uv);
  return oi::check_launch("oi_tex_uv");
}

int oi_tex_points(const float* pos, const int* triangles, long long f0, long long nf, int T, float* out, uint8_t* flags,
                  oi_stream_t stream) {
  int rc = check_chunk(f0, nf, T, "oi_tex_points");
  if (rc != OI_OK) return rc;
  if (nf == 0) return OI_OK;
  OI_REQUIRE(pos && triangles && out, "oi_tex_points: null pointer");
  const long long n = nf * (T * (T + 1) / 2);
  hipLaunchKernelGGL(tex_points_kernel, dim3(n_blocks(n)), dim3(MT_THREADS), 0, oi::as_stream(stream), pos, triangles, f0, n,
                     T, out, flags);
  return oi::check_launch("oi_tex_points");
}

int oi_tex_store(const float* normals, const float* rgb, long long f0, long long nf, int T, long long F, float* albedo_f32,
                 float* normal_f32, unsigned char* albedo_u8, unsigned char* normal_u8, oi_stream_t stream) {
  int rc = check_chunk(f0, nf, T, "oi_tex_store");
  if (rc != OI_OK) return rc;
  Layout l;
  rc = oi_tex_layout(F, T, &l.W, &l.H, &l.cols);
  if (rc != OI_OK) return rc;
  OI_REQUIRE(f0 + nf <= F, "oi_tex_store: chunk f0=%lld nf=%lld past the mesh's F=%lld triangles", f0, nf, F);
  if (nf == 0 || !(albedo_f32 || normal_f32 || albedo_u8 || normal_u8)) return OI_OK;
  OI_REQUIRE(normals && rgb, "oi_tex_store: null pointer");
  const long long n = nf * (T * (T + 1) / 2);
  hipLaunchKernelGGL(tex_store_kernel, dim3(n_blocks(n)), dim3(MT_THREADS), 0, oi::as_stream(stream), normals, rgb, f0, n, T,
                     l.cols, l.W, albedo_f32, normal_f32, albedo_u8, normal_u8);
  return oi::check_launch("oi_tex_store");
}

}  // extern "C"
