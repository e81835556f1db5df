// Input feeding: the device-side cast of raw loader bytes and the native collation of
// a batch into the page-locked ring (host threads, no Python in the copy loop).
#include <hip/hip_fp16.h>
#include <string.h>
#include <thread>
#include <vector>
#include "common.h"

// ---- input feeding: raw loader bytes -> fp32 spectrograms ON THE DEVICE ----------------
// Replaces the per-item CPU conversion `torch.from_numpy(x).type(torch.FloatTensor)` of the reference's loader
// (ava/models/utils.py:444-446 applied in ava/models/vae_dataset.py:138-139): the batch crosses PCIe in the dtype it
// is stored in (float64 spectrograms as written by the preprocessing step: 2x the bytes but no 4M-element CPU pass;
// uint8: a quarter of the bytes) and is converted here with the same rounding as torch's cast (f64 -> f32
// round-to-nearest-even; u8 / f16 / bf16 -> f32 exact).  16 bytes per lane on the read side.
enum { AVA_DT_F32 = 0, AVA_DT_F64 = 1, AVA_DT_U8 = 2, AVA_DT_F16 = 3, AVA_DT_BF16 = 4 };

template <int DT>
__global__ __launch_bounds__(256) void cast_to_f32_kernel(const void* __restrict__ src, float* __restrict__ dst, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  if (DT == AVA_DT_F64) {                       // 2 doubles (16 B) per lane and iteration
    const double2* s2 = reinterpret_cast<const double2*>(src);
    float2* d2 = reinterpret_cast<float2*>(dst);
    const int64_t n2 = n / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += stride) {
      const double2 v = s2[i];
      d2[i] = make_float2((float)v.x, (float)v.y);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) dst[n - 1] = (float)reinterpret_cast<const double*>(src)[n - 1];
  } else if (DT == AVA_DT_U8) {                 // 16 bytes per lane -> four float4 stores
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    const int64_t n16 = n / 16;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
      const uint4 v = s4[i];
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        d4[4 * i + q] = make_float4((float)(w[q] & 0xffu), (float)((w[q] >> 8) & 0xffu), (float)((w[q] >> 16) & 0xffu),
                                    (float)(w[q] >> 24));
    }
    if (blockIdx.x == 0)
      for (int64_t i = n16 * 16 + threadIdx.x; i < n; i += 256) dst[i] = (float)reinterpret_cast<const unsigned char*>(src)[i];
  } else if (DT == AVA_DT_F16 || DT == AVA_DT_BF16) {     // 8 halves (16 B) per lane
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    const int64_t n8 = n / 8;
    auto cvt = [](unsigned short h) -> float {
      if (DT == AVA_DT_BF16) return __uint_as_float((unsigned)h << 16);
      return __half2float(__ushort_as_half(h));
    };
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
      const uint4 v = s4[i];
      d4[2 * i] = make_float4(cvt(v.x & 0xffff), cvt(v.x >> 16), cvt(v.y & 0xffff), cvt(v.y >> 16));
      d4[2 * i + 1] = make_float4(cvt(v.z & 0xffff), cvt(v.z >> 16), cvt(v.w & 0xffff), cvt(v.w >> 16));
    }
    if (blockIdx.x == 0)
      for (int64_t i = n8 * 8 + threadIdx.x; i < n; i += 256) dst[i] = cvt(reinterpret_cast<const unsigned short*>(src)[i]);
  } else {                                      // f32: plain copy (kept so that one call covers every loader dtype)
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    const int64_t n4 = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) d4[i] = s4[i];
    if (blockIdx.x == 0)
      for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += 256) dst[i] = reinterpret_cast<const float*>(src)[i];
  }
}

extern "C" int ava_cast_to_f32(const void* src, int src_dtype, int64_t n, float* dst, ava_stream_t s) {
  if (src == nullptr || dst == nullptr || n <= 0) return AVA_EINVAL;
  if ((reinterpret_cast<uintptr_t>(src) & 15) != 0 || (reinterpret_cast<uintptr_t>(dst) & 15) != 0) return AVA_EINVAL;
  int64_t work = src_dtype == AVA_DT_F64 ? n / 2 : (src_dtype == AVA_DT_U8 ? n / 16 : (src_dtype == AVA_DT_F32 ? n / 4 : n / 8));
  int blocks = (int)((work + 255) / 256);
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  hipStream_t st = to_stream(s);
  switch (src_dtype) {
    case AVA_DT_F32: hipLaunchKernelGGL(cast_to_f32_kernel<AVA_DT_F32>, dim3(blocks), dim3(256), 0, st, src, dst, n); break;
    case AVA_DT_F64: hipLaunchKernelGGL(cast_to_f32_kernel<AVA_DT_F64>, dim3(blocks), dim3(256), 0, st, src, dst, n); break;
    case AVA_DT_U8: hipLaunchKernelGGL(cast_to_f32_kernel<AVA_DT_U8>, dim3(blocks), dim3(256), 0, st, src, dst, n); break;
    case AVA_DT_F16: hipLaunchKernelGGL(cast_to_f32_kernel<AVA_DT_F16>, dim3(blocks), dim3(256), 0, st, src, dst, n); break;
    case AVA_DT_BF16: hipLaunchKernelGGL(cast_to_f32_kernel<AVA_DT_BF16>, dim3(blocks), dim3(256), 0, st, src, dst, n); break;
    default: return AVA_EINVAL;
  }
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

// ---- host side: gather n rows of row_bytes each, src[idx[i]] -> dst[i] (dst: a slot of the page-locked ring) --------
// Replaces default_collate's per-item torch.stack of the reference's DataLoader (ava/models/vae_dataset.py:89-96) for
// array-backed datasets.  Runs on `threads` std::threads (the copy is memory-bound: one core moves ~5 GB/s, a 16 MiB
// batch needs ~4 to keep up with a 2 ms step); ctypes releases the GIL for the duration of the call, so the Python
// thread that launches the step's kernels is not disturbed.  idx == NULL: rows first .. first + n - 1.
extern "C" int ava_host_gather_rows(void* dst, const void* src, const int64_t* idx, int64_t first, int64_t n,
                                    size_t row_bytes, int threads) {
  if (dst == nullptr || src == nullptr || n < 0 || row_bytes == 0) return AVA_EINVAL;
  if (n == 0) return AVA_OK;
  if (threads < 1) threads = 1;
  if (threads > 16) threads = 16;
  {  // at least 2 MiB per thread: starting a thread costs more than copying less (uint8 batches: 8 threads 2.1 ms, 4 threads 0.14 ms)
    const size_t per = (size_t)2 << 20, total = (size_t)n * row_bytes;
    const int cap = (int)(total / per);
    if (threads > cap) threads = cap < 1 ? 1 : cap;
  }
  if ((int64_t)threads > n) threads = (int)n;
  auto work = [=](int64_t lo, int64_t hi) {
    char* d = static_cast<char*>(dst);
    const char* s = static_cast<const char*>(src);
    if (idx == nullptr) {
      memcpy(d + (size_t)lo * row_bytes, s + (size_t)(first + lo) * row_bytes, (size_t)(hi - lo) * row_bytes);
    } else {
      for (int64_t i = lo; i < hi; ++i) memcpy(d + (size_t)i * row_bytes, s + (size_t)idx[i] * row_bytes, row_bytes);
    }
  };
  if (threads == 1) { work(0, n); return AVA_OK; }
  std::vector<std::thread> pool;
  const int64_t step = (n + threads - 1) / threads;
  for (int t = 1; t < threads; ++t) {
    const int64_t lo = t * step, hi = lo + step < n ? lo + step : n;
    if (lo < hi) pool.emplace_back(work, lo, hi);
  }
  work(0, step < n ? step : n);
  for (auto& th : pool) th.join();
  return AVA_OK;
}

// ---- device side: gather n rows of a resident dataset into one fp32 batch ---------------
// dst[j, :] = float(src[idx[j], :]): the device twin of ava_host_gather_rows + ava_cast_to_f32 for datasets that live
// in HBM (syllable_dataset.DeviceSyllableDataset).  Replaces SyllableDataset.__getitem__ + numpy_to_tensor + the
// DataLoader's collation (ava/models/vae_dataset.py:125-145, :89-96) with one launch per batch; same rounding as
// cast_to_f32_kernel.  A workgroup of 256 lanes holds 256 >> tpr_log2 rows of 1 << tpr_log2 lanes each (short rows
// share a workgroup, a long row spreads over gridDim.y workgroups), so no lane divides.  WIDE: every lane moves
// GatherVec<DT>::V elements per step with 16-byte loads and 16-byte stores; the host picks it only when a row is a
// whole number of such steps and both base pointers are 16-byte aligned, which makes every row start aligned too.
// Otherwise one element per lane and step.  A row whose index is outside [0, n_rows) is skipped: nothing is read,
// nothing is written.  All offsets are 64-bit.
template <int DT> struct GatherVec { enum { V = 4 }; };                   // f32: one float4; f64: two double2
template <> struct GatherVec<AVA_DT_U8> { enum { V = 16 }; };
template <> struct GatherVec<AVA_DT_F16> { enum { V = 8 }; };
template <> struct GatherVec<AVA_DT_BF16> { enum { V = 8 }; };

template <int DT>
__device__ __forceinline__ float gather_cvt16(unsigned short h) {
  if (DT == AVA_DT_BF16) return __uint_as_float((unsigned)h << 16);
  return __half2float(__ushort_as_half(h));
}

template <int DT, bool WIDE>
__global__ __launch_bounds__(256) void gather_rows_f32_kernel(const void* __restrict__ src, int64_t n_rows, int64_t row_elems,
                                                              const int64_t* __restrict__ idx, int64_t n,
                                                              float* __restrict__ dst, int tpr_log2) {
  const int tpr = 1 << tpr_log2;
  const int lane = threadIdx.x & (tpr - 1);
  const int64_t rows_per_wg = 256 >> tpr_log2;
  const int64_t steps = WIDE ? row_elems / GatherVec<DT>::V : row_elems;      // per row
  const int64_t step_stride = (int64_t)gridDim.y * tpr;
  for (int64_t j = (int64_t)blockIdx.x * rows_per_wg + (threadIdx.x >> tpr_log2); j < n; j += (int64_t)gridDim.x * rows_per_wg) {
    const int64_t r = idx[j];
    if (r < 0 || r >= n_rows) continue;
    const int64_t so = r * row_elems;                                         // in elements
    float* __restrict__ d = dst + j * row_elems;
    for (int64_t c = (int64_t)blockIdx.y * tpr + lane; c < steps; c += step_stride) {
      if (!WIDE) {
        float v;
        if (DT == AVA_DT_F64) v = (float)reinterpret_cast<const double*>(src)[so + c];
        else if (DT == AVA_DT_U8) v = (float)reinterpret_cast<const unsigned char*>(src)[so + c];
        else if (DT == AVA_DT_F16 || DT == AVA_DT_BF16) v = gather_cvt16<DT>(reinterpret_cast<const unsigned short*>(src)[so + c]);
        else v = reinterpret_cast<const float*>(src)[so + c];
        d[c] = v;
      } else if (DT == AVA_DT_F64) {
        const double2* s2 = reinterpret_cast<const double2*>(reinterpret_cast<const double*>(src) + so);
        const double2 a = s2[2 * c], b = s2[2 * c + 1];
        reinterpret_cast<float4*>(d)[c] = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
      } else if (DT == AVA_DT_U8) {
        const uint4 v = reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(src) + so)[c];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          reinterpret_cast<float4*>(d)[4 * c + q] = make_float4((float)(w[q] & 0xffu), (float)((w[q] >> 8) & 0xffu),
                                                                (float)((w[q] >> 16) & 0xffu), (float)(w[q] >> 24));
      } else if (DT == AVA_DT_F16 || DT == AVA_DT_BF16) {
        const uint4 v = reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(src) + so)[c];
        reinterpret_cast<float4*>(d)[2 * c] = make_float4(gather_cvt16<DT>(v.x & 0xffff), gather_cvt16<DT>(v.x >> 16),
                                                          gather_cvt16<DT>(v.y & 0xffff), gather_cvt16<DT>(v.y >> 16));
        reinterpret_cast<float4*>(d)[2 * c + 1] = make_float4(gather_cvt16<DT>(v.z & 0xffff), gather_cvt16<DT>(v.z >> 16),
                                                              gather_cvt16<DT>(v.w & 0xffff), gather_cvt16<DT>(v.w >> 16));
      } else {
        reinterpret_cast<float4*>(d)[c] = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(src) + so)[c];
      }
    }
  }
}

template <int DT>
static void gather_rows_launch(const void* src, int64_t n_rows, int64_t row_elems, const int64_t* idx, int64_t n,
                               float* dst, hipStream_t st) {
  const bool wide = row_elems % GatherVec<DT>::V == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const int64_t steps = wide ? row_elems / GatherVec<DT>::V : row_elems;
  int tpr_log2 = 0;                                   // lanes per row: the power of two that covers a row, at most 256
  while (tpr_log2 < 8 && ((int64_t)1 << tpr_log2) < steps) ++tpr_log2;
  const int64_t tpr = (int64_t)1 << tpr_log2, rows_per_wg = 256 / tpr;
  int64_t gx = (n + rows_per_wg - 1) / rows_per_wg;   // the kernel strides over what the caps leave
  if (gx > 65536) gx = 65536;
  int64_t gy = (steps + tpr - 1) / tpr;
  if (gy > 32) gy = 32;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (wide)
    hipLaunchKernelGGL((gather_rows_f32_kernel<DT, true>), grid, dim3(256), 0, st, src, n_rows, row_elems, idx, n, dst, tpr_log2);
  else
    hipLaunchKernelGGL((gather_rows_f32_kernel<DT, false>), grid, dim3(256), 0, st, src, n_rows, row_elems, idx, n, dst, tpr_log2);
}

extern "C" int ava_gather_rows_f32(const void* src, int src_dtype, int64_t n_rows, int64_t row_elems, const int64_t* idx,
                                   int64_t n, float* dst, ava_stream_t s) {
  if (src == nullptr || idx == nullptr || dst == nullptr || n <= 0 || row_elems <= 0 || n_rows <= 0) return AVA_EINVAL;
  hipStream_t st = to_stream(s);
  switch (src_dtype) {
    case AVA_DT_F32: gather_rows_launch<AVA_DT_F32>(src, n_rows, row_elems, idx, n, dst, st); break;
    case AVA_DT_F64: gather_rows_launch<AVA_DT_F64>(src, n_rows, row_elems, idx, n, dst, st); break;
    case AVA_DT_U8: gather_rows_launch<AVA_DT_U8>(src, n_rows, row_elems, idx, n, dst, st); break;
    case AVA_DT_F16: gather_rows_launch<AVA_DT_F16>(src, n_rows, row_elems, idx, n, dst, st); break;
    case AVA_DT_BF16: gather_rows_launch<AVA_DT_BF16>(src, n_rows, row_elems, idx, n, dst, st); break;
    default: return AVA_EINVAL;
  }
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}
