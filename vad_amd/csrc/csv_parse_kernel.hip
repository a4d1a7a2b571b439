// Dataset CSV text -> line index, feature rows and labels on the device
// (include/vad_amd.h, "Dataset CSV import"): the device form of the
// reference's create_file_index (dataset/file_index.py:7-23) and of the
// np.asarray(csv row, dtype) of load_csv / __get_features_from_line
// (dataset/file_processing.py:151-184, 236-242).
//
// Line index.  A line starts at byte 0 and after every '\n' that is not the
// text's last byte, so the rank of a line start is one plus the count of
// '\n' before it: a prefix count over tiles of VAD_CSV_TILE bytes, in the
// launch shape of segments_kernel.hip -- tile kernel (count per tile) ->
// carry kernel (ONE workgroup looping over the tile counts kCarryPass at a
// time, which also writes the line total) -> tile kernel (apply: each '\n'
// stores the offset after it at its rank).  The block scan and the carry loop
// are block_scan.h's.  No kernel waits on another workgroup and there are no
// atomics.
//
// Parse.  One wave per line, one wave per workgroup (so __syncthreads() is
// the wave's own ordering point and rows need no packing rule): the wave
// copies the line into LDS with aligned dword loads, finds the commas with a
// ballot and a lane prefix count per 64 bytes, and lane j parses output j
// (a used column, or the label) from LDS; lines with more than 64 outputs
// take several passes.  A field is parsed into at most 19 significant digits
// w and a decimal exponent q, and w * 10^q is rounded to the nearest double:
//   * w < 2^53 and |q| <= 22: both are exact doubles, one IEEE multiply or
//     divide (Clinger's fast path);
//   * otherwise the 64 x 128-bit product of the normalised w with the
//     truncated 128-bit power of five T(q) (pow5_table.h, Eisel-Lemire): for
//     0 <= q <= 55 T is exact and so is the product; elsewhere the true
//     product lies strictly between L = w * T and L + w, so when both have
//     the same 54 leading bits those bits and a set sticky bit are the true
//     ones, and the second 64-bit word of T is only multiplied in when the
//     first product's low nine bits are all ones.  When L and L + w differ
//     the value may be a dyadic number: for -27 <= q < 0 with 5^-q dividing
//     w it is (w / 5^-q) * 2^q exactly; anything else is left to the host.
// The device never guesses: more than 19 digits, an unresolved product,
// blanks, a signed nan and everything outside the grammar set the row's HOST
// bit, and the caller re-parses that row.  tests/csv_parse_reference.py is
// this algorithm in Python integers, checked against float().
#include "block_scan.h"
#include "pow5_table.h"

namespace vad {
namespace {

constexpr int kCsvThreads = 256;
static_assert(kCsvThreads == kScanThreads, "the line index kernels run block_scan.h's scan");
constexpr int kCsvItems = 16;  // bytes per thread: one 16-byte load
constexpr int kCsvTile = kCsvThreads * kCsvItems;
static_assert(kCsvTile == VAD_CSV_TILE, "the header's tile is the kernels' tile");
static_assert(kCarryPass == VAD_CSV_CARRY_PASS, "the header's pass is the carry loop's pass");
constexpr int kMaxLine = VAD_CSV_MAX_LINE;
constexpr int kMaxCols = VAD_CSV_MAX_COLS;
constexpr uint64_t kInfBits = 0x7FF0000000000000ull;
constexpr uint64_t kNanBits = 0x7FF8000000000000ull;
constexpr int kExpCap = 100000;  // exponent digits saturate here, far past any double

// Bit j: byte i0 + j is a '\n' that starts a line after it (not the last byte).
__device__ __forceinline__ uint32_t line_start_bits(const uint8_t* bytes, int64_t n, int64_t i0, bool aligned) {
  uint32_t m = 0;
  if (i0 >= n) return 0;
  if (aligned && i0 + kCsvItems <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(bytes + i0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < kCsvItems; ++j)
      if (((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) == '\n') m |= 1u << j;
  } else {
    for (int j = 0; j < kCsvItems; ++j)
      if (i0 + j < n && bytes[i0 + j] == '\n') m |= 1u << j;
  }
  if (n - 1 - i0 < kCsvItems) m &= ~(1u << (int)(n - 1 - i0));
  return m;
}

__global__ __launch_bounds__(kCsvThreads) void csv_count_kernel(const uint8_t* bytes, int64_t n, int64_t* tile_cnt) {
  __shared__ int64_t lds[kCsvThreads / 64];
  const bool aligned = (reinterpret_cast<uintptr_t>(bytes) & 15) == 0;
  const int64_t i0 = (int64_t)blockIdx.x * kCsvTile + (int64_t)threadIdx.x * kCsvItems;
  int64_t tot;
  block_excl<true>((int64_t)__popc(line_start_bits(bytes, n, i0, aligned)), OpSum(), (int64_t)0, lds, &tot);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

// carry[t] = line starts after a '\n' in tiles < t; *n_lines = all lines.
__global__ __launch_bounds__(kCsvThreads) void csv_carry_kernel(const int64_t* tile_cnt, int64_t n_tiles,
                                                                int64_t* carry, int64_t n, int64_t* n_lines) {
  __shared__ int64_t lds[kCsvThreads / 64];
  int64_t run = 0, tot;
  for (int64_t b = 0; b < n_tiles; b += kCarryPass) {
    const int64_t t = b + threadIdx.x;
    const int64_t ex = block_excl<true>(t < n_tiles ? tile_cnt[t] : (int64_t)0, OpSum(), (int64_t)0, lds, &tot);
    if (t < n_tiles) carry[t] = run + ex;
    run += tot;
  }
  if (threadIdx.x == 0) *n_lines = n > 0 ? run + 1 : 0;
}

// index[r - skip] = base + offset of line r, for skip <= r < skip + capacity.
__global__ __launch_bounds__(kCsvThreads) void csv_index_kernel(const uint8_t* bytes, int64_t n, const int64_t* carry,
                                                                int64_t skip, int64_t base, int64_t* index,
                                                                int64_t capacity) {
  __shared__ int64_t lds[kCsvThreads / 64];
  const bool aligned = (reinterpret_cast<uintptr_t>(bytes) & 15) == 0;
  const int64_t i0 = (int64_t)blockIdx.x * kCsvTile + (int64_t)threadIdx.x * kCsvItems;
  uint32_t m = line_start_bits(bytes, n, i0, aligned);
  int64_t tot;
  int64_t r = 1 + carry[blockIdx.x] + block_excl<true>((int64_t)__popc(m), OpSum(), (int64_t)0, lds, &tot) - skip;
  if (blockIdx.x == 0 && threadIdx.x == 0 && skip == 0 && capacity > 0 && n > 0) index[0] = base;
  while (m) {
    const int j = __ffs(m) - 1;
    m &= m - 1;
    if (r >= 0 && r < capacity) index[r] = base + i0 + j + 1;
    ++r;
  }
}

// ---------------------------------------------------------------------------
// Decimal -> double
// ---------------------------------------------------------------------------

// m54: the 54 leading bits (2^53 <= m54 < 2^54) of a value in [2^e2, 2^(e2+1));
// sticky: anything nonzero below them.  Round to nearest even into a double's
// bits, subnormals, zero and infinity included.
__device__ __forceinline__ uint64_t round_pack(uint64_t m54, bool sticky, int e2) {
  const bool normal = e2 >= -1022;
  const int d = normal ? 1 : -1021 - e2;  // bits dropped from m54
  if (d >= 64) return 0;
  uint64_t kept = m54 >> d;
  const bool rnd = (m54 >> (d - 1)) & 1;
  const bool st = sticky || (m54 & ((1ull << (d - 1)) - 1)) != 0;
  if (rnd && (st || (kept & 1))) ++kept;
  const uint64_t bits = (normal ? (uint64_t)(e2 + 1022) << 52 : 0ull) + kept;
  return bits >= kInfBits ? kInfBits : bits;
}

// Bits of the double nearest w * 10^q (w < 10^19); false: leave it to the host.
__device__ bool decimal_to_double(uint64_t w, int q, uint64_t* out) {
  if (w == 0 || q < kPow5MinExp) {
    *out = 0;
    return true;
  }
  if (q > kPow5MaxExp) {
    *out = kInfBits;
    return true;
  }
  if (w < (1ull << 53) && q >= -kCsvFastMaxExp && q <= kCsvFastMaxExp) {
    const double d = (double)(int64_t)w;
    *out = (uint64_t)__double_as_longlong(q < 0 ? d / kPow10Exact[-q] : d * kPow10Exact[q]);
    return true;
  }
  const int lz = __clzll((long long)w);
  const uint64_t wn = w << lz;
  const uint64_t thi = kPow5[q - kPow5MinExp][0], tlo = kPow5[q - kPow5MinExp][1];
  const bool exact = q >= 0 && q <= kPow5ExactMax;
  const uint64_t xh = __umul64hi(wn, thi), xl = wn * thi;
  uint64_t h = xh, m = 0, lo = 0;
  bool inexact_sticky = false;  // the value is known to lie strictly above (h, m, lo)
  if (tlo == 0) {
    m = xl;  // exact table entry of one word: the product is (xh, xl, 0)
  } else if (!exact && (xh & 0x1FF) != 0x1FF) {
    // the words below xh add less than 2^64 at xl's weight: a carry of at
    // most one into xh, which cannot reach the bits above the low nine
    inexact_sticky = true;
  } else {
    const uint64_t yh = __umul64hi(wn, tlo);
    lo = wn * tlo;
    m = xl + yh;
    h = xh + (m < xl ? 1 : 0);
    if (!exact) {
      const uint64_t lo2 = lo + wn;
      const uint64_t m2 = m + (lo2 < lo ? 1 : 0);
      const uint64_t h2 = h + (m2 < m ? 1 : 0);
      const int up1 = (int)(h >> 63), up2 = (int)(h2 >> 63);
      if (up1 != up2 || (h >> (9 + up1)) != (h2 >> (9 + up2))) {
        // L and L + wn round differently.  The one case with a rule: 5^-q
        // divides w, so the value is the dyadic number (w / 5^-q) * 2^q
        if (q < 0 && q >= -kPow5SmallMax) {
          const uint64_t p5 = kPow5Small[-q], quo = w / p5;
          if (quo * p5 == w) {
            const double scale = __longlong_as_double((long long)((uint64_t)(1023 + q) << 52));
            *out = (uint64_t)__double_as_longlong((double)quo * scale);
            return true;
          }
        }
        return false;
      }
      inexact_sticky = true;
    }
  }
  const int up = (int)(h >> 63);
  const uint64_t m54 = h >> (9 + up);
  const bool sticky = inexact_sticky || (h & ((1ull << (9 + up)) - 1)) != 0 || m != 0 || lo != 0;
  const int e2 = 63 + up + ((q * kLog2Of5Q16) >> 16) + q - lz;
  *out = round_pack(m54, sticky, e2);
  return true;
}

__device__ __forceinline__ bool is_digit(int c) { return c >= '0' && c <= '9'; }

// One field s[0..n) -> double bits; false: the host decides.  Grammar:
// [+-]?(digits[.digits*]|.digits)([eE][+-]?digits)?, nan, [+-]?inf(inity)?.
__device__ bool parse_field(const uint8_t* s, int n, uint64_t* out) {
  if (n <= 0) return false;
  int i = 0;
  bool neg = false, sign_seen = false;
  if (s[0] == '+' || s[0] == '-') {
    neg = s[0] == '-';
    sign_seen = true;
    i = 1;
  }
  const uint64_t sign = neg ? 1ull << 63 : 0ull;
  if (i < n && ((s[i] | 0x20) == 'n' || (s[i] | 0x20) == 'i')) {
    const int r = n - i;
    if (r != 3 && r != 8) return false;
    const char* word = (s[i] | 0x20) == 'n' ? "nan" : "infinity";
    if ((s[i] | 0x20) == 'n' && (r != 3 || sign_seen)) return false;
    for (int k = 0; k < r; ++k)
      if ((s[i + k] | 0x20) != word[k]) return false;
    *out = (s[i] | 0x20) == 'n' ? kNanBits : (kInfBits | sign);
    return true;
  }
  uint64_t w = 0;
  int nd = 0, frac = 0;
  bool seen_digit = false, seen_point = false;
  for (; i < n; ++i) {
    const int c = s[i];
    if (is_digit(c)) {
      seen_digit = true;
      if (w != 0 || c != '0') {
        if (nd < kCsvMaxDigits) w = w * 10 + (uint64_t)(c - '0');
        ++nd;
      }
      if (seen_point) ++frac;
    } else if (c == '.' && !seen_point) {
      seen_point = true;
    } else {
      break;
    }
  }
  if (!seen_digit) return false;
  int e = 0;
  if (i < n && (s[i] | 0x20) == 'e') {
    ++i;
    bool eneg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) {
      eneg = s[i] == '-';
      ++i;
    }
    if (i >= n || !is_digit(s[i])) return false;
    for (; i < n && is_digit(s[i]); ++i) {
      e = e * 10 + (s[i] - '0');
      if (e > kExpCap) e = kExpCap;
    }
    if (eneg) e = -e;
  }
  if (i != n || nd > kCsvMaxDigits) return false;
  uint64_t bits;
  if (!decimal_to_double(w, e - frac, &bits)) return false;
  *out = bits | sign;
  return true;
}

// ---------------------------------------------------------------------------
// Parse kernel
// ---------------------------------------------------------------------------
struct CsvParseArgs {
  const uint8_t* bytes;
  int64_t n_bytes;
  const int64_t* index;
  int64_t n_rows;
  int64_t base;
  int n_cols, n_used, has_cols;
  void* x;
  uint8_t* y;
  int32_t* status;
  int16_t cols[VAD_CSV_MAX_USED];
};

constexpr int kParseGrid = 256 * 16;  // one-wave workgroups: 16 per CU

template <bool F64>
__global__ __launch_bounds__(64) void csv_parse_kernel(const CsvParseArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t line[kMaxLine + 16];
  __shared__ uint16_t sep[kMaxCols];
  const int lane = threadIdx.x;
  const uint8_t* const buf_end = a.bytes + a.n_bytes;
  for (int64_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
    const int64_t start = a.index[r] - a.base;
    int64_t end = r + 1 < a.n_rows ? a.index[r + 1] - a.base : a.n_bytes;
    // offsets that are not an ascending index into the text: refuse the row
    if (start < 0 || end < start || end > a.n_bytes) {
      if (lane == 0) a.status[r] = VAD_CSV_ROW_MALFORMED;
      continue;
    }
    if (end > start && a.bytes[end - 1] == '\n') --end;
    if (end > start && a.bytes[end - 1] == '\r') --end;
    const int64_t len64 = end - start;
    if (len64 > kMaxLine) {
      if (lane == 0) a.status[r] = VAD_CSV_ROW_MALFORMED;
      continue;
    }
    const int len = (int)len64;
    const uint8_t* p = a.bytes + start;
    const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 3);
    const int words = (mis + len + 3) >> 2;  // <= (3 + 4096 + 3) / 4 = 1025 words
    for (int k = lane; k < words; k += 64) {
      const uint8_t* q = p - mis + 4 * k;
      uint32_t v = 0;
      if (q >= a.bytes && q + 4 <= buf_end) {
        v = *reinterpret_cast<const uint32_t*>(q);
      } else {
        for (int j = 0; j < 4; ++j)
          if (q + j >= a.bytes && q + j < buf_end) v |= (uint32_t)q[j] << (8 * j);
      }
      reinterpret_cast<uint32_t*>(line)[k] = v;
    }
    __syncthreads();
    const uint8_t* s = line + mis;
    int n_sep = 0;
    for (int c0 = 0; c0 < len; c0 += 64) {
      const int i = c0 + lane;
      const bool comma = i < len && s[i] == ',';
      const unsigned long long mask = __ballot(comma);
      const int k = n_sep + __popcll(mask & ((1ull << lane) - 1));
      if (comma && k < kMaxCols) sep[k] = (uint16_t)i;
      n_sep += __popcll(mask);
    }
    __syncthreads();
    if (n_sep + 1 != a.n_cols) {
      if (lane == 0) a.status[r] = VAD_CSV_ROW_MALFORMED;
      __syncthreads();
      continue;
    }
    int st = 0;
    for (int j0 = 0; j0 <= a.n_used; j0 += 64) {  // output n_used is the label
      const int j = j0 + lane;
      int mine = 0;
      if (j <= a.n_used) {
        const int col = j == a.n_used ? a.n_cols - 1 : (a.has_cols ? (int)a.cols[j] : j);
        const int fs = col == 0 ? 0 : sep[col - 1] + 1;
        const int fe = col == a.n_cols - 1 ? len : sep[col];
        uint64_t bits = 0;
        if (!parse_field(s + fs, fe - fs, &bits)) mine = VAD_CSV_ROW_HOST;
        const double d = __longlong_as_double((long long)bits);
        if (j == a.n_used) {
          // int(float(label)): truncation; the caller refuses what no uint8 holds
          const bool ok = d > -1.0 && d < 256.0;
          if (!ok && !mine) mine = VAD_CSV_ROW_LABEL;
          a.y[r] = ok ? (uint8_t)(int)d : (uint8_t)0;
        } else if (F64) {
          static_cast<double*>(a.x)[r * a.n_used + j] = d;
        } else {
          static_cast<float*>(a.x)[r * a.n_used + j] = (float)d;
        }
      }
      st |= mine;
    }
    const int any = (__ballot(st & VAD_CSV_ROW_HOST) ? VAD_CSV_ROW_HOST : 0) |
                    (__ballot(st & VAD_CSV_ROW_LABEL) ? VAD_CSV_ROW_LABEL : 0);
    if (lane == 0) a.status[r] = any;
    __syncthreads();  // line and sep are rewritten by the next row
  }
}

inline int64_t csv_tiles(int64_t n) { return (n + kCsvTile - 1) / kCsvTile; }

}  // namespace

// workspace: [tile counts] [tile carries], int64 each
size_t csv_workspace_bytes(int64_t n_bytes) {
  if (n_bytes < 0) return 0;
  return 2 * align_up(sizeof(int64_t) * (size_t)(csv_tiles(n_bytes) + 1), 256);
}

hipError_t launch_csv_count(const uint8_t* bytes, int64_t n, int64_t* n_lines, void* ws, hipStream_t st) {
  const int64_t nt = csv_tiles(n);
  int64_t* cnt = static_cast<int64_t*>(ws);
  int64_t* carry = reinterpret_cast<int64_t*>(static_cast<char*>(ws) + csv_workspace_bytes(n) / 2);
  if (nt > 0) csv_count_kernel<<<dim3((unsigned)nt), dim3(kCsvThreads), 0, st>>>(bytes, n, cnt);
  csv_carry_kernel<<<dim3(1), dim3(kCsvThreads), 0, st>>>(cnt, nt, carry, n, n_lines);
  return hipGetLastError();
}

hipError_t launch_csv_index(const uint8_t* bytes, int64_t n, int64_t skip, int64_t base, int64_t* index,
                            int64_t capacity, const void* ws, hipStream_t st) {
  const int64_t nt = csv_tiles(n);
  if (nt == 0 || capacity == 0) return hipSuccess;
  const int64_t* carry = reinterpret_cast<const int64_t*>(static_cast<const char*>(ws) + csv_workspace_bytes(n) / 2);
  csv_index_kernel<<<dim3((unsigned)nt), dim3(kCsvThreads), 0, st>>>(bytes, n, carry, skip, base, index, capacity);
  return hipGetLastError();
}

hipError_t launch_csv_parse(const uint8_t* bytes, int64_t n_bytes, const int64_t* index, int64_t n_rows, int64_t base,
                            int n_cols, const int32_t* columns, int n_used, bool f64, void* x, uint8_t* y,
                            int32_t* status, hipStream_t st) {
  if (n_rows == 0) return hipSuccess;
  CsvParseArgs a{};
  a.bytes = bytes, a.n_bytes = n_bytes, a.index = index, a.n_rows = n_rows, a.base = base;
  a.n_cols = n_cols, a.n_used = n_used, a.has_cols = columns != nullptr;
  a.x = x, a.y = y, a.status = status;
  for (int j = 0; columns && j < n_used; ++j) a.cols[j] = (int16_t)columns[j];
  const unsigned grid = (unsigned)(n_rows < kParseGrid ? n_rows : kParseGrid);
  if (f64)
    csv_parse_kernel<true><<<dim3(grid), dim3(64), 0, st>>>(a);
  else
    csv_parse_kernel<false><<<dim3(grid), dim3(64), 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace vad
