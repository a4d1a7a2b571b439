// Ragged copies of clip batches (include/vad_amd.h, "Clip batches"):
//   vad_batch_pack_*: the samples of n_clips clips, each wherever it lies in
//     device memory, into one packed buffer in which clip k starts at sample
//     start[k]; everything between the end of a clip and the start of the
//     next (the tail of its last hop slot) is written as zero;
//   vad_batch_compact_rows: out[row0[k] + i] = rows[frame0[k] + i], rows of
//     row_bytes bytes: the per-clip rows of a result over the global window
//     grid, clip after clip with the junk rows between the clips left out.
// Both are one kernel, ragged_copy_kernel, written as gather_kernel of
// segments_kernel.hip is: a persistent grid strides over DESTINATION tiles of
// 32 KB; per tile the segments (clips) of its first and last byte are found
// once, by binary search in the destination offsets; a tile inside one
// segment -- every tile but a few per clip for clips of seconds -- is copied
// with 8 independent 16-byte stores per lane and the widest loads the
// source's alignment allows (16, 8, 4, 2 or 1 bytes); the other tiles search
// per 16-byte destination chunk inside [first segment, last segment].  The
// destination is 16-byte aligned (the entries refuse another), so every store
// but those of the last, partial chunk is a 16-byte store.  Bits are copied,
// never converted.  No LDS, no atomics; no workgroup waits on another.
//
// Everything is counted in bytes; ES (4, 2 or 1) is the unit that every
// offset, length and source address is a multiple of: the element size of the
// samples, or the largest of 4 / 2 / 1 that divides row_bytes and the rows'
// address.
#include "vad_common.h"

namespace vad {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kCopyThreads = 256;
constexpr int kCopyChunks = 8;   // 16-byte chunks per lane and tile: 32 KB tiles
constexpr int kCopyGrid = 2048;  // 256 CUs x 8 workgroups of 4 waves
constexpr int64_t kTileBytes = (int64_t)kCopyThreads * kCopyChunks * 16;

// 16 bytes from an address aligned to AB bytes
template <int AB>
__device__ __forceinline__ u32x4 load16(const char* p) {
  if constexpr (AB == 16) {
    return *reinterpret_cast<const u32x4*>(p);
  } else if constexpr (AB == 8) {
    const u32x2 x = *reinterpret_cast<const u32x2*>(p), y = *reinterpret_cast<const u32x2*>(p + 8);
    return u32x4{x.x, x.y, y.x, y.y};
  } else if constexpr (AB == 4) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    return u32x4{q[0], q[1], q[2], q[3]};
  } else if constexpr (AB == 2) {
    const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
    return u32x4{q[0] | (uint32_t)q[1] << 16, q[2] | (uint32_t)q[3] << 16, q[4] | (uint32_t)q[5] << 16,
                 q[6] | (uint32_t)q[7] << 16};
  } else {
    const uint8_t* q = reinterpret_cast<const uint8_t*>(p);
    u32x4 v;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      v[w] = q[4 * w] | (uint32_t)q[4 * w + 1] << 8 | (uint32_t)q[4 * w + 2] << 16 | (uint32_t)q[4 * w + 3] << 24;
    return v;
  }
}

template <int ES>
__device__ __forceinline__ u32x4 load16_any(const char* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  if ((a & 15) == 0) return load16<16>(p);
  if ((a & 7) == 0) return load16<8>(p);
  if (ES == 4 || (a & 3) == 0) return load16<4>(p);
  if (ES == 2 || (a & 1) == 0) return load16<2>(p);
  return load16<1>(p);
}

// a whole tile inside one segment: lane t copies chunks t, t + 256, ...; all
// the loads are issued before the first store
template <int AB>
__device__ __forceinline__ void copy_tile(const char* src, char* dst) {
  u32x4 v[kCopyChunks];
#pragma unroll
  for (int j = 0; j < kCopyChunks; ++j) v[j] = load16<AB>(src + (size_t)(j * kCopyThreads + threadIdx.x) * 16);
#pragma unroll
  for (int j = 0; j < kCopyChunks; ++j)
    *reinterpret_cast<u32x4*>(dst + (size_t)(j * kCopyThreads + threadIdx.x) * 16) = v[j];
}

// Segment k of the destination: bytes [doff(k), doff(k) + len(k)) come from
// src(k); doff is non-decreasing in k (segments of no bytes repeat it) and
// the bytes of no segment are zero.
//   PACK 1: doff = start[k] * ES, len = lens[k] * ES, src = the address ptrs[k]
//   PACK 0: doff = row0[k] * row_bytes, len = n_rows[k] * row_bytes,
//           src = rows + frame0[k] * row_bytes
struct RaggedArgs {
  const int64_t* doff_el;  // start / row0
  const int64_t* len_el;   // lens / n_rows
  const int64_t* src_el;   // ptrs (addresses) / frame0
  int64_t n_seg;
  int64_t unit;            // bytes per element of the three tables: ES / row_bytes
  const char* base;        // PACK 0: the rows
  int64_t base_bytes;      // PACK 0: bytes readable at base
  char* dst;
  int64_t total;           // bytes of the destination
};

template <bool PACK>
struct SegTable {
  const RaggedArgs& a;
  __device__ int64_t doff(int64_t k) const { return a.doff_el[k] * a.unit; }
  // the bytes of segment k that may be read, clamped so that no table content
  // makes a load leave the rows (PACK 0) or turns a length negative
  __device__ int64_t len(int64_t k) const {
    int64_t l = a.len_el[k] * a.unit;
    if (!PACK) {
      const int64_t s = a.src_el[k] * a.unit;
      if (s < 0 || s > a.base_bytes) return 0;
      if (l > a.base_bytes - s) l = a.base_bytes - s;
    }
    return l > 0 ? l : 0;
  }
  __device__ const char* src(int64_t k) const {
    return PACK ? reinterpret_cast<const char*>(static_cast<uintptr_t>(a.src_el[k])) : a.base + a.src_el[k] * a.unit;
  }
  // the last segment in [lo, hi] whose doff is <= b; lo - 1 when there is none
  __device__ int64_t locate(int64_t b, int64_t lo, int64_t hi) const {
    int64_t below = lo - 1;
    while (lo <= hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (doff(mid) <= b) below = mid, lo = mid + 1; else hi = mid - 1;
    }
    return below;
  }
};

template <int ES, bool PACK>
__global__ __launch_bounds__(kCopyThreads) void ragged_copy_kernel(RaggedArgs a) {
  const SegTable<PACK> tab{a};
  constexpr int V = 16 / ES;
  for (int64_t b0 = (int64_t)blockIdx.x * kTileBytes; b0 < a.total; b0 += (int64_t)gridDim.x * kTileBytes) {
    const int64_t b_end = b0 + kTileBytes < a.total ? b0 + kTileBytes : a.total;
    const int64_t k_lo = tab.locate(b0, 0, a.n_seg - 1);
    const int64_t k_hi = tab.locate(b_end - 1, k_lo < 0 ? 0 : k_lo, a.n_seg - 1);
    if (k_lo >= 0 && k_lo == k_hi && b_end - b0 == kTileBytes) {
      const int64_t o = tab.doff(k_lo);
      if (b_end <= o + tab.len(k_lo)) {
        const char* src = tab.src(k_lo) + (b0 - o);
        char* dst = a.dst + b0;
        const uintptr_t al = reinterpret_cast<uintptr_t>(src);
        if ((al & 15) == 0) copy_tile<16>(src, dst);
        else if ((al & 7) == 0) copy_tile<8>(src, dst);
        else if (ES == 4 || (al & 3) == 0) copy_tile<4>(src, dst);
        else if (ES == 2 || (al & 1) == 0) copy_tile<2>(src, dst);
        else copy_tile<1>(src, dst);
        continue;
      }
    }
    for (int j = 0; j < kCopyChunks; ++j) {
      const int64_t b = b0 + ((int64_t)j * kCopyThreads + threadIdx.x) * 16;
      if (b >= a.total) break;
      int64_t k = k_lo == k_hi ? k_lo : tab.locate(b, k_lo < 0 ? 0 : k_lo, k_hi);
      int64_t o = 0, l = 0;
      const char* s = nullptr;
      if (k >= 0) o = tab.doff(k), l = tab.len(k), s = tab.src(k);
      u32x4 v;
      if (k >= 0 && b + 16 <= o + l) {
        v = load16_any<ES>(s + (b - o));
      } else {  // a chunk across the end of a segment: element by element, zero between segments
        v = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < V; ++t) {
          const int64_t eb = b + t * ES;
          if (eb >= a.total) break;
          while (k + 1 < a.n_seg && tab.doff(k + 1) <= eb) {
            ++k;
            o = tab.doff(k), l = tab.len(k), s = tab.src(k);
          }
          if (k < 0 || eb - o >= l) continue;
          const char* p = s + (eb - o);
          uint32_t x;
          if (ES == 4) x = *reinterpret_cast<const uint32_t*>(p);
          else if (ES == 2) x = *reinterpret_cast<const uint16_t*>(p);
          else x = *reinterpret_cast<const uint8_t*>(p);
          v[t * ES / 4] |= x << (8 * (t * ES % 4));
        }
      }
      if (b + 16 <= a.total) {
        *reinterpret_cast<u32x4*>(a.dst + b) = v;
      } else {  // the last chunk of a destination that is no multiple of 16 bytes
        for (int64_t eb = b; eb < a.total; ++eb)
          a.dst[eb] = (char)(v[(eb - b) / 4] >> (8 * ((eb - b) % 4)));
      }
    }
  }
}

template <int ES, bool PACK>
hipError_t launch_ragged(const RaggedArgs& a, hipStream_t st) {
  const int64_t tiles = (a.total + kTileBytes - 1) / kTileBytes;
  ragged_copy_kernel<ES, PACK><<<dim3((unsigned)(tiles < kCopyGrid ? tiles : kCopyGrid)), dim3(kCopyThreads), 0, st>>>(a);
  return hipGetLastError();
}

template <int ES>
int batch_pack(const int64_t* src_ptrs, const int64_t* lens, const int64_t* start, int64_t n_clips, void* dst,
               int64_t total, void* stream) {
  if (n_clips < 0 || total < 0 || total > INT64_MAX / 8) return VAD_EINVAL;
  if (n_clips > 0 && (!src_ptrs || !lens || !start)) return VAD_EINVAL;
  if (total == 0) return VAD_OK;
  if (!dst || reinterpret_cast<uintptr_t>(dst) % 16) return VAD_EINVAL;
  RaggedArgs a{};
  a.doff_el = start, a.len_el = lens, a.src_el = src_ptrs, a.n_seg = n_clips, a.unit = ES;
  a.dst = static_cast<char*>(dst), a.total = total * ES;
  return (int)launch_ragged<ES, true>(a, static_cast<hipStream_t>(stream));
}

}  // namespace
}  // namespace vad

using namespace vad;

extern "C" {

int vad_batch_pack_f32(const int64_t* src_ptrs, const int64_t* lens, const int64_t* start, int64_t n_clips,
                       float* dst, int64_t total, void* stream) {
  return batch_pack<4>(src_ptrs, lens, start, n_clips, dst, total, stream);
}

int vad_batch_pack_i16(const int64_t* src_ptrs, const int64_t* lens, const int64_t* start, int64_t n_clips,
                       int16_t* dst, int64_t total, void* stream) {
  return batch_pack<2>(src_ptrs, lens, start, n_clips, dst, total, stream);
}

int vad_batch_compact_rows(const void* rows, int64_t n_rows_in, int64_t row_bytes, const int64_t* frame0,
                           const int64_t* n_rows, const int64_t* row0, int64_t n_clips, void* out,
                           int64_t n_rows_out, void* stream) {
  if (n_clips < 0 || n_rows_in < 0 || n_rows_out < 0 || row_bytes <= 0) return VAD_EINVAL;
  if (n_rows_in > INT64_MAX / 2 / row_bytes || n_rows_out > INT64_MAX / 2 / row_bytes) return VAD_EINVAL;
  if (n_clips > 0 && (!frame0 || !n_rows || !row0)) return VAD_EINVAL;
  if (n_rows_out == 0) return VAD_OK;
  if (!out || reinterpret_cast<uintptr_t>(out) % 16 || (n_rows_in > 0 && !rows)) return VAD_EINVAL;
  if (overlap(rows, (size_t)(n_rows_in * row_bytes), out, (size_t)(n_rows_out * row_bytes))) return VAD_EINVAL;
  RaggedArgs a{};
  a.doff_el = row0, a.len_el = n_rows, a.src_el = frame0, a.n_seg = n_clips, a.unit = row_bytes;
  a.base = static_cast<const char*>(rows), a.base_bytes = n_rows_in * row_bytes;
  a.dst = static_cast<char*>(out), a.total = n_rows_out * row_bytes;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uintptr_t al = reinterpret_cast<uintptr_t>(rows) | (uintptr_t)row_bytes;
  if ((al & 3) == 0) return (int)launch_ragged<4, false>(a, st);
  if ((al & 1) == 0) return (int)launch_ragged<2, false>(a, st);
  return (int)launch_ragged<1, false>(a, st);
}

}  // extern "C"
