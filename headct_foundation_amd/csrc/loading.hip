// Device side of the loading chain (loading_transforms, src/data/transforms.py:108-178): what turns one decoded NIfTI volume
// into the fp16 cache item.  One volume per call (shapes differ from scan to scan), everything on the caller's stream, nothing
// waits for the host: the resampled shape comes from the header, the foreground box stays in device memory.
//
//   hct_volume_to_ras            : raw typed voxels * slope + inter -> fp32 in RAS voxel order (axis permutation and flips folded
//                                  into the read; where the file's contiguous axis is not the output's, through a 32 x 32 LDS
//                                  tile so that both the loads and the stores of a wave are contiguous)
//   hct_bspline3_resample        : Spacingd(1 mm, mode=3): cubic B-spline resampling as three 1-D passes in float64 (as MONAI
//                                  computes it), fp32 in and out.  Per axis every output voxel is one FIR of kTaps inputs
//                                  (prefilter and interpolation weights folded into one table on the host, see
//                                  nifti.bspline3_tables), so there is no serial recursion.  The two strided passes
//                                  walk the contiguous axis across lanes (a wave's loads are one contiguous run per tap, its
//                                  weights wave-uniform); the pass along the contiguous axis puts neighbouring outputs on
//                                  neighbouring lanes, which read overlapping windows of the same row through L1.
//   hct_foreground_bbox          : CropForegroundd's tight box of voxels > 0, integer min / max in two launches (no atomics)
//   hct_crop_window_resize_area  : box -> HU windows -> area resize -> fp16, one pass
#include "common.h"

#include <limits.h>

#include <algorithm>

namespace hct {

constexpr int kTaps = 32;          // = nifti.TAPS
constexpr int kMaxAxis = 1024;     // = nifti.MAX_AXIS
constexpr int kBoxMaxChunks = 1024;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

// ---- raw -> fp32 RAS -------------------------------------------------------------------------------------------------------
struct RasMap {
  int d[3];        // output (RAS) shape
  int64_t rs[3];   // raw element stride of output axis o
  int flip[3];
  int scaled;
  double slope, inter;
};

template <typename T>
__device__ __forceinline__ float raw_value(const T* __restrict__ raw, const RasMap& g, int x0, int x1, int x2) {
  const int64_t off = g.rs[0] * (g.flip[0] ? g.d[0] - 1 - x0 : x0) + g.rs[1] * (g.flip[1] ? g.d[1] - 1 - x1 : x1) +
                      g.rs[2] * (g.flip[2] ? g.d[2] - 1 - x2 : x2);
  const T v = raw[off];
  // nibabel scales integers in float64 (apply_read_scaling), MONAI then casts to float32
  return g.scaled ? (float)((double)v * g.slope + g.inter) : (float)v;
}

// the file's contiguous axis is the output's contiguous axis: a plain streaming copy
template <typename T>
__global__ void __launch_bounds__(256) to_ras_direct_kernel(const T* __restrict__ raw, float* __restrict__ out, RasMap g) {
  const int x2 = blockIdx.x * 256 + threadIdx.x;
  if (x2 >= g.d[2]) return;
  const int x1 = blockIdx.y, x0 = blockIdx.z;
  out[((int64_t)x0 * g.d[1] + x1) * g.d[2] + x2] = raw_value(raw, g, x0, x1, x2);
}

// the file's contiguous axis is output axis A (0 or 1): tiles of 32 (axis A) x 32 (axis 2), the third axis on blockIdx.z
template <typename T, int A>
__global__ void __launch_bounds__(256) to_ras_tile_kernel(const T* __restrict__ raw, float* __restrict__ out, RasMap g) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int a0 = blockIdx.x * 32, z0 = blockIdx.y * 32, xb = blockIdx.z;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int xa = a0 + tx, x2 = z0 + ty + 8 * r;
    if (xa < g.d[A] && x2 < g.d[2]) tile[ty + 8 * r][tx] = A == 0 ? raw_value(raw, g, xa, xb, x2) : raw_value(raw, g, xb, xa, x2);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int xa = a0 + ty + 8 * r, x2 = z0 + tx;
    if (xa < g.d[A] && x2 < g.d[2]) {
      const int x0 = A == 0 ? xa : xb, x1 = A == 0 ? xb : xa;
      out[((int64_t)x0 * g.d[1] + x1) * g.d[2] + x2] = tile[tx][ty + 8 * r];
    }
  }
}

template <typename T>
static void launch_to_ras(const void* raw, float* out, const RasMap& g, int contiguous_axis, hipStream_t s) {
  if (contiguous_axis == 2) {
    hipLaunchKernelGGL(to_ras_direct_kernel<T>, dim3((g.d[2] + 255) / 256, g.d[1], g.d[0]), dim3(256), 0, s, (const T*)raw, out, g);
  } else if (contiguous_axis == 0) {
    hipLaunchKernelGGL((to_ras_tile_kernel<T, 0>), dim3((g.d[0] + 31) / 32, (g.d[2] + 31) / 32, g.d[1]), dim3(256), 0, s, (const T*)raw, out, g);
  } else {
    hipLaunchKernelGGL((to_ras_tile_kernel<T, 1>), dim3((g.d[1] + 31) / 32, (g.d[2] + 31) / 32, g.d[0]), dim3(256), 0, s, (const T*)raw, out, g);
  }
}

// ---- cubic B-spline resampling, one axis per launch ------------------------------------------------------------------------
// MONAI's Spacing computes in float64 and casts the result to float32 once.  So does this: weights, accumulators and the two
// intermediate volumes are doubles, the input and the output fp32.  In fp32 the resampled volume is off by about 1e-3 HU (at
// +-1200 HU), which the narrowest window (80 HU wide) and the mean over a bin turn into a few steps of an fp16 cache value below
// 1e-4, i.e. of voxels just above a window's lower end; the passes are bound by their loads, not by the fused multiply-adds.
//
// [outer][n][inner] -> [outer][m][inner], inner contiguous: lanes along inner, output index j and outer on the grid
template <typename TIn, typename TOut>
__global__ void resample_strided_kernel(const TIn* __restrict__ in, TOut* __restrict__ out, int n, int m, int inner,
                                        const int32_t* __restrict__ base, const double* __restrict__ w) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= inner) return;
  const int j = blockIdx.y, o = blockIdx.z;
  const int b = base[j];
  const TIn* src = in + (int64_t)o * n * inner + idx;
  double acc = 0.0;
#pragma unroll 8
  for (int t = 0; t < kTaps; ++t) {
    const int r = min(max(b + t, 0), n - 1);  // the edge-extended signal; the table cannot move a read out of the row
    acc = fma(w[t * m + j], (double)src[(int64_t)r * inner], acc);
  }
  out[((int64_t)o * m + j) * inner + idx] = (TOut)acc;
}

// [rows][n] -> [rows][m]: lanes along the outputs of a row, 4 rows per thread share the weights
template <typename TIn, typename TOut>
__global__ void __launch_bounds__(256) resample_rows_kernel(const TIn* __restrict__ in, TOut* __restrict__ out, int64_t rows, int n, int m,
                                                            const int32_t* __restrict__ base, const double* __restrict__ w) {
  const int j = blockIdx.y * 256 + threadIdx.x;
  if (j >= m) return;
  const int64_t row0 = (int64_t)blockIdx.x * 4;
  const int nr = (int)min((int64_t)4, rows - row0);
  const int b = base[j];
  const TIn* src = in + row0 * n;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int t = 0; t < kTaps; ++t) {
    const int r = min(max(b + t, 0), n - 1);
    const double wt = w[t * m + j];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < nr) acc[q] = fma(wt, (double)src[(int64_t)q * n + r], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (q < nr) out[(row0 + q) * m + j] = (TOut)acc[q];
}

// ---- foreground box --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// mn[3] / mx[3] of a block's threads -> thread 0 (256 threads = 4 waves)
__device__ __forceinline__ void block_box(int mn[3], int mx[3]) {
  __shared__ int s[4][6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = wave_min_i(mn[a]);
    mx[a] = wave_max_i(mx[a]);
  }
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; ++a) {
      s[threadIdx.x >> 6][a] = mn[a];
      s[threadIdx.x >> 6][3 + a] = mx[a];
    }
  __syncthreads();
  for (int a = 0; a < 3; ++a) {
    mn[a] = min(min(s[0][a], s[1][a]), min(s[2][a], s[3][a]));
    mx[a] = max(max(s[0][3 + a], s[1][3 + a]), max(s[2][3 + a], s[3][3 + a]));
  }
}

static int box_chunks(int64_t rows) { return (int)std::min<int64_t>(kBoxMaxChunks, std::max<int64_t>(1, (rows + 3) / 4)); }

// partial [chunks][6]: one wave per row (x, y) of the volume, lanes along z
__global__ void __launch_bounds__(256) bbox_partial_kernel(const float* __restrict__ vol, int m0, int m1, int m2, int32_t* __restrict__ partial) {
  const int64_t rows = (int64_t)m0 * m1;
  const int lane = threadIdx.x & 63;
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {-1, -1, -1};
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const int x = (int)(row / m1), y = (int)(row - (int64_t)x * m1);
    const float* p = vol + row * m2;
    for (int z = lane; z < m2; z += 64)
      if (p[z] > 0.f) {
        mn[0] = min(mn[0], x); mx[0] = max(mx[0], x);
        mn[1] = min(mn[1], y); mx[1] = max(mx[1], y);
        mn[2] = min(mn[2], z); mx[2] = max(mx[2], z);
      }
  }
  block_box(mn, mx);
  if (threadIdx.x == 0)
    for (int a = 0; a < 3; ++a) {
      partial[blockIdx.x * 6 + a] = mn[a];
      partial[blockIdx.x * 6 + 3 + a] = mx[a];
    }
}

// box = start[3], size[3]; status = 1 where no voxel is > 0 (the box is then the whole volume, so that what follows stays in range)
__global__ void __launch_bounds__(256) bbox_fold_kernel(const int32_t* __restrict__ partial, int chunks, int m0, int m1, int m2,
                                                        int32_t* __restrict__ box, int32_t* __restrict__ status) {
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {-1, -1, -1};
  for (int c = threadIdx.x; c < chunks; c += 256)
    for (int a = 0; a < 3; ++a) {
      mn[a] = min(mn[a], partial[c * 6 + a]);
      mx[a] = max(mx[a], partial[c * 6 + 3 + a]);
    }
  block_box(mn, mx);
  if (threadIdx.x == 0) {
    const bool empty = mx[0] < 0;
    const int full[3] = {m0, m1, m2};
    for (int a = 0; a < 3; ++a) {
      box[a] = empty ? 0 : mn[a];
      box[3 + a] = empty ? full[a] : mx[a] - mn[a] + 1;
    }
    status[0] = empty ? HCT_LOAD_EMPTY_FOREGROUND : 0;
  }
}

// ---- box -> windows -> area resize -> fp16 ---------------------------------------------------------------------------------
// one thread makes 8 consecutive outputs of the contiguous axis for all C channels (a voxel is loaded once and windowed C times)
template <int C>
__global__ void __launch_bounds__(256) crop_window_resize_kernel(const float* __restrict__ vol, int m0, int m1, int m2, const int32_t* __restrict__ box,
                                                                 const float* __restrict__ a_min, const float* __restrict__ a_max,
                                                                 f16* __restrict__ out, int R0, int R1, int R2, int threads) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= threads) return;
  const int r8 = (R2 + 7) >> 3;
  const int k8 = t % r8, r = t / r8;
  const int j = r % R1, i = r / R1;
  // the box lives on the device and cannot be checked by the host: confined to the volume here
  const int s0 = min(max(box[0], 0), m0 - 1), s1 = min(max(box[1], 0), m1 - 1), s2 = min(max(box[2], 0), m2 - 1);
  const int n0 = min(max(box[3], 1), m0 - s0), n1 = min(max(box[4], 1), m1 - s1), n2 = min(max(box[5], 1), m2 - s2);
  float lo[C], range[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    lo[c] = a_min[c];
    range[c] = a_max[c] - a_min[c];
  }
  const int x0 = s0 + (i * n0) / R0, x1 = s0 + ((i + 1) * n0 + R0 - 1) / R0;
  const int y0 = s1 + (j * n1) / R1, y1 = s1 + ((j + 1) * n1 + R1 - 1) / R1;
  int z0[8], z1[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int k = min(k8 * 8 + q, R2 - 1);
    z0[q] = s2 + (k * n2) / R2;
    z1[q] = s2 + ((k + 1) * n2 + R2 - 1) / R2;
  }
  float acc[C][8];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[c][q] = 0.f;
  // fixed order: x, then y, then z ascending
  for (int x = x0; x < x1; ++x)
    for (int y = y0; y < y1; ++y) {
      const float* row = vol + ((int64_t)x * m1 + y) * m2;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        for (int z = z0[q]; z < z1[q]; ++z) {
          const float v = row[z];
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c][q] += fminf(fmaxf((v - lo[c]) / range[c], 0.0f), 1.0f);
        }
    }
  const float nxy = (float)((x1 - x0) * (y1 - y0));
#pragma unroll
  for (int c = 0; c < C; ++c) {
    f16* dst = out + (((int64_t)c * R0 + i) * R1 + j) * R2 + k8 * 8;
    f16x8 o;
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = (f16)(acc[c][q] / (nxy * (float)(z1[q] - z0[q])));
    if ((R2 & 7) == 0) {
      *reinterpret_cast<f16x8*>(dst) = o;
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (k8 * 8 + q < R2) dst[q] = o[q];
    }
  }
}

}  // namespace hct

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int hct_volume_to_ras(const void* raw, int nifti_datatype, int ni, int nj, int nk, const int* perm, const int* flip, int scaled, double slope,
                      double inter, float* out, void* stream) {
  HCT_REQUIRE(raw && out && perm && flip && raw != (const void*)out, "hct_volume_to_ras: null argument");
  HCT_REQUIRE(ni > 0 && nj > 0 && nk > 0 && ni <= 65535 && nj <= 65535 && nk <= 65535, "hct_volume_to_ras: bad shape (%d, %d, %d)", ni, nj, nk);
  HCT_REQUIRE(perm[0] >= 0 && perm[0] < 3 && perm[1] >= 0 && perm[1] < 3 && perm[2] >= 0 && perm[2] < 3 && perm[0] != perm[1] &&
                  perm[0] != perm[2] && perm[1] != perm[2], "hct_volume_to_ras: perm (%d, %d, %d) is not a permutation", perm[0], perm[1], perm[2]);
  const int nin[3] = {ni, nj, nk};
  const int64_t stride[3] = {1, ni, (int64_t)ni * nj};
  hct::RasMap g;
  int contiguous_axis = 0;
  for (int o = 0; o < 3; ++o) {
    g.d[o] = nin[perm[o]];
    g.rs[o] = stride[perm[o]];
    g.flip[o] = flip[o] ? 1 : 0;
    if (perm[o] == 0) contiguous_axis = o;
  }
  g.scaled = scaled ? 1 : 0;
  g.slope = slope;
  g.inter = inter;
  hipStream_t s = (hipStream_t)stream;
  switch (nifti_datatype) {  // NIfTI-1 datatype codes
    case 2: hct::launch_to_ras<uint8_t>(raw, out, g, contiguous_axis, s); break;
    case 4: hct::launch_to_ras<int16_t>(raw, out, g, contiguous_axis, s); break;
    case 8: hct::launch_to_ras<int32_t>(raw, out, g, contiguous_axis, s); break;
    case 16: hct::launch_to_ras<float>(raw, out, g, contiguous_axis, s); break;
    case 64: hct::launch_to_ras<double>(raw, out, g, contiguous_axis, s); break;
    case 256: hct::launch_to_ras<int8_t>(raw, out, g, contiguous_axis, s); break;
    case 512: hct::launch_to_ras<uint16_t>(raw, out, g, contiguous_axis, s); break;
    default: HCT_REQUIRE(false, "hct_volume_to_ras: NIfTI datatype code %d is not supported", nifti_datatype);
  }
  HCT_CHECK_LAUNCH("hct_volume_to_ras");
  return 0;
}

size_t hct_bspline3_resample_workspace_bytes(int n0, int n1, int n2, int m0, int m1, int m2) {
  (void)n0; (void)m2;
  if (n1 <= 0 || n2 <= 0 || m0 <= 0 || m1 <= 0) return 0;
  return hct::align_up((size_t)m0 * n1 * n2 * sizeof(double), 256) + hct::align_up((size_t)m0 * m1 * n2 * sizeof(double), 256);
}

int hct_bspline3_resample(const float* in, int n0, int n1, int n2, float* out, int m0, int m1, int m2, const int32_t* base, const double* weights,
                          void* workspace, size_t workspace_bytes, void* stream) {
  HCT_REQUIRE(in && out && base && weights && in != out, "hct_bspline3_resample: null argument");
  const int dims[6] = {n0, n1, n2, m0, m1, m2};
  for (int a = 0; a < 6; ++a)
    HCT_REQUIRE(dims[a] > 0 && dims[a] <= hct::kMaxAxis, "hct_bspline3_resample: axis of %d voxels (1 ... %d are taken, in and out)", dims[a], hct::kMaxAxis);
  HCT_REQUIRE(workspace && workspace_bytes >= hct_bspline3_resample_workspace_bytes(n0, n1, n2, m0, m1, m2), "hct_bspline3_resample: workspace too small");
  double* t1 = (double*)workspace;                                                                          // [m0][n1][n2]
  double* t2 = (double*)((char*)workspace + hct::align_up((size_t)m0 * n1 * n2 * sizeof(double), 256));     // [m0][m1][n2]
  const int32_t *b0 = base, *b1 = base + m0, *b2 = base + m0 + m1;                                          // tables of the three axes, one after the other
  const double *w0 = weights, *w1 = weights + (size_t)hct::kTaps * m0, *w2 = weights + (size_t)hct::kTaps * (m0 + m1);
  hipStream_t s = (hipStream_t)stream;
  auto block_for = [](int inner) { return inner > 128 ? 256 : inner > 64 ? 128 : 64; };
  {
    const int inner = n1 * n2, blk = block_for(inner);
    hipLaunchKernelGGL((hct::resample_strided_kernel<float, double>), dim3((inner + blk - 1) / blk, m0, 1), dim3(blk), 0, s, in, t1, n0, m0, inner, b0, w0);
  }
  {
    const int blk = block_for(n2);
    hipLaunchKernelGGL((hct::resample_strided_kernel<double, double>), dim3((n2 + blk - 1) / blk, m1, m0), dim3(blk), 0, s, (const double*)t1, t2, n1, m1,
                       n2, b1, w1);
  }
  const int64_t rows = (int64_t)m0 * m1;
  hipLaunchKernelGGL((hct::resample_rows_kernel<double, float>), dim3((unsigned)((rows + 3) / 4), (m2 + 255) / 256), dim3(256), 0, s, (const double*)t2, out,
                     rows, n2, m2, b2, w2);
  HCT_CHECK_LAUNCH("hct_bspline3_resample");
  return 0;
}

size_t hct_foreground_bbox_workspace_bytes(int m0, int m1, int m2) {
  (void)m2;
  if (m0 <= 0 || m1 <= 0) return 0;
  return (size_t)hct::box_chunks((int64_t)m0 * m1) * 6 * sizeof(int32_t);
}

int hct_foreground_bbox(const float* vol, int m0, int m1, int m2, int32_t* box, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  HCT_REQUIRE(vol && box && status, "hct_foreground_bbox: null argument");
  HCT_REQUIRE(m0 > 0 && m1 > 0 && m2 > 0 && m0 <= 65535 && m1 <= 65535 && m2 <= 65535, "hct_foreground_bbox: bad shape (%d, %d, %d)", m0, m1, m2);
  HCT_REQUIRE(workspace && workspace_bytes >= hct_foreground_bbox_workspace_bytes(m0, m1, m2), "hct_foreground_bbox: workspace too small");
  const int chunks = hct::box_chunks((int64_t)m0 * m1);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(hct::bbox_partial_kernel, dim3(chunks), dim3(256), 0, s, vol, m0, m1, m2, (int32_t*)workspace);
  hipLaunchKernelGGL(hct::bbox_fold_kernel, dim3(1), dim3(256), 0, s, (const int32_t*)workspace, chunks, m0, m1, m2, box, status);
  HCT_CHECK_LAUNCH("hct_foreground_bbox");
  return 0;
}

int hct_crop_window_resize_area(const float* vol, int m0, int m1, int m2, const int32_t* box, int n_windows, const float* a_min, const float* a_max,
                                void* out, int R0, int R1, int R2, void* stream) {
  HCT_REQUIRE(vol && box && a_min && a_max && out && (const void*)vol != out, "hct_crop_window_resize_area: null argument");
  HCT_REQUIRE(m0 > 0 && m1 > 0 && m2 > 0 && m0 <= 65535 && m1 <= 65535 && m2 <= 65535, "hct_crop_window_resize_area: bad shape (%d, %d, %d)", m0, m1, m2);
  HCT_REQUIRE(R0 > 0 && R1 > 0 && R2 > 0 && R0 <= 4096 && R1 <= 4096 && R2 <= 4096, "hct_crop_window_resize_area: bad roi (%d, %d, %d): 1 ... 4096 per axis", R0, R1, R2);
  HCT_REQUIRE(n_windows >= 1 && n_windows <= 4, "hct_crop_window_resize_area: %d windows (1 ... 4 are taken)", n_windows);
  const int64_t threads = (int64_t)R0 * R1 * ((R2 + 7) / 8);
  HCT_REQUIRE(threads <= (int64_t)1 << 30, "hct_crop_window_resize_area: roi too large");
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
#define HCT_CWR(C_) hipLaunchKernelGGL(hct::crop_window_resize_kernel<C_>, grid, block, 0, s, vol, m0, m1, m2, box, a_min, a_max, (hct::f16*)out, R0, R1, R2, (int)threads)
  if (n_windows == 1) HCT_CWR(1);
  else if (n_windows == 2) HCT_CWR(2);
  else if (n_windows == 3) HCT_CWR(3);
  else HCT_CWR(4);
#undef HCT_CWR
  HCT_CHECK_LAUNCH("hct_crop_window_resize_area");
  return 0;
}

}  // extern "C"
