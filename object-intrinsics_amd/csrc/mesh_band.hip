// Narrow-band mesh extraction for gfx950 (include/oi_mesh_band.h has the rule, DESIGN section 4.14 the measurements): the
// classification of the blocks of a lattice from one coarse value per block, the fill of the inactive blocks and the list of
// the active ones.  It accelerates the reference's extract_fields (src/third_party/neus/models/renderer.py:15-41): the MLP
// then runs at the points of the listed blocks only (oi_sdf_lattice_band, csrc/mlp.hip).
//
// One launch.  Workgroup g takes the blocks [g * 256, (g + 1) * 256), one per thread:
//   decide   inactive iff uc is finite and |uc - iso| > thr, in double (thr = |scale| G m comes from the host);
//            the slopes to the +x, +y, +z neighbours, the maximum by an integer atomicMax on the bits of a float >= 0;
//   compact  the active blocks with a 64-bit ballot per wave (popcount on the lower lanes) and an LDS scan over the waves,
//            one atomicAdd per workgroup reserves the range of the list: the ORDER of the list depends on the arrival of the
//            workgroups, nothing else does (the field is a function of the coarse values alone);
//   fill     the workgroup writes uc to every lattice point of its inactive blocks, consecutive threads along z (runs of b
//            floats), ragged ends respected.
// 64-bit indices into the field; block ids fit 24 bits (256 blocks per axis at most).  No scratch, 16 VGPRs, 2100 B of LDS.
#include "oi_common.h"
#include "../../include/oi_mesh_band.h"

namespace {

constexpr int BAND_THREADS = 256;
constexpr int BAND_WAVES = BAND_THREADS / 64;

struct BandLattice {
  int nx, ny, nz;     // lattice points
  int nbx, nby, nbz;  // blocks
  int lb;             // log2 of the block size
  long long nblk;
};

struct BandCounters {  // device, zeroed before the launch; copied to the host in one piece
  unsigned active, above, below, slope_bits;
};

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }
inline size_t list_bytes(long long nblk) { return align256(sizeof(unsigned) * (size_t)nblk); }

__device__ __forceinline__ bool finite_(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ void __launch_bounds__(BAND_THREADS)
band_classify_kernel(const float* __restrict__ coarse, BandLattice L, double thr, float iso, double inv_dx, double inv_dy,
                     double inv_dz, float* __restrict__ field, unsigned* __restrict__ list, BandCounters* __restrict__ out) {
  __shared__ float s_uc[BAND_THREADS];
  __shared__ unsigned s_blk[BAND_THREADS];  // bi << 20 | bj << 10 | bk, bit 31: inactive
  __shared__ unsigned s_wave[3][BAND_WAVES];
  __shared__ unsigned s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long blk = (long long)blockIdx.x * BAND_THREADS + tid;
  const bool live = blk < L.nblk;

  float uc = 0.f;
  bool inactive = false, above = false;
  unsigned code = 0;
  float slope = 0.f;
  if (live) {
    const int nyz = L.nby * L.nbz;
    const int bi = (int)(blk / nyz), r = (int)(blk - (long long)bi * nyz), bj = r / L.nbz, bk = r - bj * L.nbz;
    uc = coarse[blk];
    const bool fin = finite_(uc);
    const double du = (double)uc - (double)iso;
    inactive = fin && fabs(du) > thr;
    above = inactive && du > 0.0;
    code = ((unsigned)bi << 20) | ((unsigned)bj << 10) | (unsigned)bk;
    if (fin) {
      double s = 0.0;
      if (bi + 1 < L.nbx) {
        const float un = coarse[blk + nyz];
        if (finite_(un)) s = fmax(s, fabs((double)uc - (double)un) * inv_dx);
      }
      if (bj + 1 < L.nby) {
        const float un = coarse[blk + L.nbz];
        if (finite_(un)) s = fmax(s, fabs((double)uc - (double)un) * inv_dy);
      }
      if (bk + 1 < L.nbz) {
        const float un = coarse[blk + 1];
        if (finite_(un)) s = fmax(s, fabs((double)uc - (double)un) * inv_dz);
      }
      slope = (float)s;  // >= 0; +inf when the double is out of float's range, which is above every finite bound
    }
  }
  s_uc[tid] = uc;
  s_blk[tid] = code | (inactive ? 0x80000000u : 0u);

  // ---- compaction of the active blocks, counts of the inactive ones
  const bool act = live && !inactive;
  const unsigned long long m_act = __ballot(act), m_abv = __ballot(above), m_blw = __ballot(inactive && !above);
  const unsigned pre = (unsigned)__popcll(m_act & ((1ull << lane) - 1ull));
  if (lane == 0) {
    s_wave[0][wave] = (unsigned)__popcll(m_act);
    s_wave[1][wave] = (unsigned)__popcll(m_abv);
    s_wave[2][wave] = (unsigned)__popcll(m_blw);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) slope = fmaxf(slope, __shfl_xor(slope, o, 64));
  if (lane == 0 && slope > 0.f) atomicMax(&out->slope_bits, __float_as_uint(slope));
  __syncthreads();
  if (tid == 0) {
    unsigned t[3] = {0, 0, 0};
#pragma unroll
    for (int w = 0; w < BAND_WAVES; ++w) t[0] += s_wave[0][w], t[1] += s_wave[1][w], t[2] += s_wave[2][w];
    s_base = t[0] ? atomicAdd(&out->active, t[0]) : 0u;
    if (t[1]) atomicAdd(&out->above, t[1]);
    if (t[2]) atomicAdd(&out->below, t[2]);
  }
  __syncthreads();
  if (act) {
    unsigned before = 0;
#pragma unroll
    for (int w = 0; w < BAND_WAVES; ++w) before += w < wave ? s_wave[0][w] : 0u;
    list[s_base + before + pre] = (unsigned)blk;  // s_base + workgroup total <= nblk: every active block is counted once
  }

  // ---- fill of the inactive blocks: slot s of the workgroup = point s % b^3 of its block s / b^3
  const int lb = L.lb, bm = (1 << lb) - 1, pts_lb = 3 * lb;
  for (int s = tid; s < (BAND_THREADS << pts_lb); s += BAND_THREADS) {
    const int q = s >> pts_lb, l = s & ((1 << pts_lb) - 1);
    const unsigned c = s_blk[q];
    if (!(c & 0x80000000u)) continue;
    const int ix = (int)(((c >> 20) & 0x3ffu) << lb) + (l >> (2 * lb));
    const int iy = (int)(((c >> 10) & 0x3ffu) << lb) + ((l >> lb) & bm);
    const int iz = (int)((c & 0x3ffu) << lb) + (l & bm);
    if (ix < L.nx && iy < L.ny && iz < L.nz) field[((long long)ix * L.ny + iy) * L.nz + iz] = s_uc[q];
  }
}

int check_args(int nx, int ny, int nz, int block, const char* what) {
  OI_REQUIRE(block == 4 || block == 8, "%s: block=%d (4 or 8)", what, block);
  OI_REQUIRE(nx >= OI_BAND_MIN_RES && ny >= OI_BAND_MIN_RES && nz >= OI_BAND_MIN_RES && nx <= OI_BAND_MAX_RES &&
                 ny <= OI_BAND_MAX_RES && nz <= OI_BAND_MAX_RES,
             "%s: lattice %d x %d x %d (every axis %d..%d)", what, nx, ny, nz, OI_BAND_MIN_RES, OI_BAND_MAX_RES);
  return OI_OK;
}

inline BandLattice make_lattice(int nx, int ny, int nz, int block) {
  BandLattice L;
  L.nx = nx, L.ny = ny, L.nz = nz;
  L.lb = block == 4 ? 2 : 3;
  L.nbx = (nx + block - 1) / block, L.nby = (ny + block - 1) / block, L.nbz = (nz + block - 1) / block;
  L.nblk = (long long)L.nbx * L.nby * L.nbz;
  return L;
}

inline bool pos_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

}  // namespace

extern "C" {

size_t oi_band_workspace_bytes(int nx, int ny, int nz, int block) {
  if (check_args(nx, ny, nz, block, "oi_band_workspace_bytes") != OI_OK) return 0;
  return list_bytes(make_lattice(nx, ny, nz, block).nblk) + 256;
}

int oi_band_classify(const float* coarse, int B, int nx, int ny, int nz, int block, double hx, double hy, double hz,
                     float iso, float scale, double lipschitz, float* field, void* workspace, size_t workspace_bytes,
                     long long* counts, float* max_slope, oi_stream_t stream) {
  OI_REQUIRE(B == 1, "oi_band_classify: B=%d (one element per call: a batch is refused)", B);
  int rc = check_args(nx, ny, nz, block, "oi_band_classify");
  if (rc != OI_OK) return rc;
  OI_REQUIRE(pos_finite(lipschitz), "oi_band_classify: lipschitz=%g (a finite bound > 0 on |grad sdf|)", lipschitz);
  OI_REQUIRE(pos_finite(hx) && pos_finite(hy) && pos_finite(hz), "oi_band_classify: spacings %g %g %g (finite, > 0)", hx, hy,
             hz);
  OI_REQUIRE(iso - iso == 0.f && scale - scale == 0.f && scale != 0.f, "oi_band_classify: iso=%g scale=%g (finite, scale != 0)",
             (double)iso, (double)scale);
  OI_REQUIRE(coarse && field && workspace && counts && max_slope, "oi_band_classify: null pointer");
  const BandLattice L = make_lattice(nx, ny, nz, block);
  OI_REQUIRE(workspace_bytes >= list_bytes(L.nblk) + 256,
             "oi_band_classify: workspace of %zu bytes, oi_band_workspace_bytes(%d, %d, %d, %d) needed", workspace_bytes, nx,
             ny, nz, block);
  unsigned* list = reinterpret_cast<unsigned*>(workspace);
  BandCounters* out = reinterpret_cast<BandCounters*>(reinterpret_cast<char*>(workspace) + list_bytes(L.nblk));
  // |scale| G m, m = d (1 + (b - 1) / 2): the order of the operations is the one of tests/helpers/band_ref.py
  const double as = fabs((double)scale);
  const double thr = (as * lipschitz) * (sqrt(hx * hx + hy * hy + hz * hz) * (1.0 + (block - 1) / 2.0));
  hipStream_t st = oi::as_stream(stream);
  if (oi::zero_async(reinterpret_cast<float*>(out), 4, st) != hipSuccess) return oi::check_launch("oi_band_classify(clear)");
  const unsigned nwg = (unsigned)((L.nblk + BAND_THREADS - 1) / BAND_THREADS);
  hipLaunchKernelGGL(band_classify_kernel, dim3(nwg), dim3(BAND_THREADS), 0, st, coarse, L, thr, iso,
                     1.0 / (as * block * hx), 1.0 / (as * block * hy), 1.0 / (as * block * hz), field, list, out);
  if ((rc = oi::check_launch("oi_band_classify")) != OI_OK) return rc;
  // the one synchronisation: the active count sizes the band launch, the slope decides whether there is one
  BandCounters h;
  if (hipMemcpyAsync(&h, out, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return oi::fail(OI_ERR_LAUNCH, "oi_band_classify: reading the counts failed");
  counts[0] = L.nblk, counts[1] = h.active, counts[2] = h.above, counts[3] = h.below;
  *max_slope = __builtin_bit_cast(float, h.slope_bits);
  if (counts[1] + counts[2] + counts[3] != L.nblk)
    return oi::fail(OI_ERR_LAUNCH, "oi_band_classify: %lld + %lld + %lld blocks counted, %lld expected", counts[1], counts[2],
                    counts[3], L.nblk);
  return OI_OK;
}

}  // extern "C"
