// extern "C" boundary of libvad_amd.so (include/vad_amd.h): plans, argument
// checking and kernel dispatch.  Host-side work here is one-off plan setup
// (filterbank -> sparse taps, lifter x DCT matrix, twiddles, FFN fragments);
// every hot entry point only validates and launches.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "vad_common.h"
#include "mel_tables.h"

using namespace vad;

// Host side of the MFCC kernel's XCD balance (vad_common.h MfccBalance):
// the kernel's paired-frame runs write (tiles, ticks) per workgroup into
// host-mapped memory; each launch folds the latest ones into per-XCD speed
// weights (workgroup b on XCD b mod 8) and passes them as a kernel argument,
// so every workgroup of a launch splits the tiles from the same 8 bytes.
// Opt-in (VAD_MFCC_BALANCE=1): on the boxes measured it moved the MFCC
// launch by -1 % but the whole C3 step by +0.6 %.
#ifndef VAD_BALANCE_DEFAULT
#define VAD_BALANCE_DEFAULT 0
#endif

namespace {
constexpr int kBalSlots = 1024;  // workgroups of a launch (<= CUs)
struct BalanceHost {
  unsigned long long* stats_host = nullptr;  // pinned, mapped
  unsigned long long* stats_dev = nullptr;
  float w[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
  unsigned long long word = 0;    // the weights in use
  unsigned long long calls = 0;
  unsigned long long forced = 0;  // VAD_MFCC_BALANCE_WORD (tests): fixed weights
  std::mutex mu;
};

BalanceHost* balance_create() {
  const char* env = getenv("VAD_MFCC_BALANCE");
  if (env ? atoi(env) == 0 : VAD_BALANCE_DEFAULT == 0) return nullptr;
  BalanceHost* b = new BalanceHost();
  void* h = nullptr;
  if (hipHostMalloc(&h, kBalSlots * sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess) {
    delete b;
    return nullptr;
  }
  memset(h, 0, kBalSlots * sizeof(unsigned long long));
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
    (void)hipHostFree(h);
    delete b;
    return nullptr;
  }
  b->stats_host = (unsigned long long*)h;
  b->stats_dev = (unsigned long long*)d;
  if (const char* fw = getenv("VAD_MFCC_BALANCE_WORD")) {
    b->forced = strtoull(fw, nullptr, 0);
    for (int x = 0; x < 8; ++x)  // every weight >= 1, or no forcing
      if (((b->forced >> (8 * x)) & 255u) == 0) b->forced = 0;
  }
  return b;
}

void balance_destroy(BalanceHost* b) {
  if (!b) return;
  (void)hipDeviceSynchronize();  // no launch of this plan may still write its stats
  (void)hipHostFree(b->stats_host);
  delete b;
}

// this launch's weights from the stats the earlier launches left (a launch
// still running leaves some of its blocks' entries old: any mix is a valid,
// if less even, split)
MfccBalance balance_for_launch(BalanceHost* b) {
  MfccBalance r;
  if (!b) return r;
  if (b->forced) {
    r.word = b->forced;
    r.stats = b->stats_dev;
    return r;
  }
  // one launch in kStatsEvery writes stats (their PCIe stores delay the
  // launch's end by ~1 us); the weights are refolded halfway to the next
  std::lock_guard<std::mutex> lk(b->mu);
  constexpr unsigned long long kStatsEvery = 16;
  const unsigned long long c = b->calls++;
  if (c % kStatsEvery == kStatsEvery / 2 || b->word == 0) {
    double tiles[8] = {}, ticks[8] = {};
    const volatile unsigned long long* st = b->stats_host;
    for (int i = 0; i < kBalSlots; ++i) {
      const unsigned long long v = st[i];
      if (!v) continue;
      tiles[i & 7] += (double)(v >> 40);
      ticks[i & 7] += (double)(v & ((1ull << 40) - 1));
    }
    bool all = true;
    double sp[8], mx = 0.;
    for (int x = 0; x < 8; ++x) {
      all = all && tiles[x] > 0. && ticks[x] > 0.;
      sp[x] = ticks[x] > 0. ? tiles[x] / ticks[x] : 0.;
      mx = sp[x] > mx ? sp[x] : mx;
    }
    if (all && mx > 0.) {
      // a block's speed is its tiles per tick whatever its share, so the new
      // weights are the speeds (smoothed: the clocks drift with load and
      // temperature)
      for (int x = 0; x < 8; ++x) b->w[x] = 0.5f * b->w[x] + 0.5f * (float)(sp[x] / mx);
    }
    float wm = 0.f;
    for (int x = 0; x < 8; ++x) wm = b->w[x] > wm ? b->w[x] : wm;
    unsigned long long word = 0;
    for (int x = 0; x < 8; ++x) {
      int q = (int)lrintf(255.f * b->w[x] / wm);
      q = q < 128 ? 128 : (q > 255 ? 255 : q);  // at most a 2x spread
      word |= (unsigned long long)q << (8 * x);
    }
    b->word = word;
    static const int dbg = getenv("VAD_MFCC_BALANCE_DEBUG") ? atoi(getenv("VAD_MFCC_BALANCE_DEBUG")) : 0;
    if (dbg) {
      fprintf(stderr, "balance: word %016llx speeds", word);
      for (int x = 0; x < 8; ++x) fprintf(stderr, " %.4f", sp[x]);
      fprintf(stderr, "\n");
    }
  }
  r.word = b->word;
  r.stats = c % kStatsEvery == 0 ? b->stats_dev : nullptr;
  return r;
}
}  // namespace

struct vad_mfcc_plan {
  MfccDev host;      // host copy (for introspection)
  MfccDev* dev;      // device copy read by the kernels
  int spec;          // 1/2: equals the compile-time Mel26/Mel40 tables bit for bit;
                     // kSpecWindow: an analysis window is set
  int table_spec;    // the compile-time table match without a window
  float* hop_blob;   // stream_hop_kernel's tables, one contiguous block (LDS-staged per launch)
  int hop_blob_n;    // floats (a multiple of 4)
  int n_taps;
  int fft_n;         // 512, or another length run by spec_generic.hip
  int bins;          // fft_n / 2 spectrum bins kept (mfcc.py:61)
  double2* tw_gen;   // exp(-2 pi i m / fft_n), m < fft_n (other lengths only)
  BalanceHost* bal;  // the MFCC kernel's XCD balance (null: equal runs)
  bool generic() const { return fft_n != kFftN; }
};

// n_hops > 1 blocks of n_streams hop rows: disjoint in either ordering
// (hop-major: each block past the previous block's last row; stream-major:
// each row's K hops before the next row), never repeating (block stride > 0)
static bool vad_hop_layout_disjoint(int64_t n_streams, int32_t n_hops, int64_t block_stride, int64_t hop_stride,
                                    int32_t hop_len) {
  if (block_stride <= 0) return false;
  if (block_stride >= (n_streams - 1) * hop_stride + hop_len) return true;
  // stream-major: a stream's K hops apart from each other, then the next stream
  return block_stride >= hop_len && hop_stride >= (int64_t)(n_hops - 1) * block_stride + hop_len;
}

// The spec a launch passes: a windowed plan whose bank is a compiled one
// says which (kSpecWindow26 / 40), so the reference framing keeps the
// generated mel code; vad_mfcc_plan_variant still reports kSpecWindow.
static int launch_spec(const vad_mfcc_plan* p) {
  if (p->spec != kSpecWindow) return p->spec;
  return p->table_spec == 1 ? kSpecWindow26 : p->table_spec == 2 ? kSpecWindow40 : kSpecWindow;
}

// Does the runtime plan equal compile-time table T (taps, ranges, DCT rows)?
template <class T>
static bool matches_table(const MfccDev& h) {
  if (h.n_filters != T::NF || h.mfcc_n != T::NC) return false;
  for (int m = 0; m < T::NF; ++m) {
    if (h.f_lo[m] != T::lo[m] || h.f_len[m] != T::len[m]) return false;
    for (int k = 0; k < kBins; ++k) {
      const bool in = k >= T::lo[m] && k < T::lo[m] + T::len[m];
      const float v = in ? h.taps[h.f_off[m] + k - T::lo[m]] : 0.f;
      if (memcmp(&v, &T::w[m][k], sizeof(float)) != 0) return false;
    }
  }
  for (int c = 0; c < T::NC; ++c)
    for (int m = 0; m < T::NF; ++m)
      if (memcmp(&h.dct[c * kMaxFilters + m], &T::dct[c][m], sizeof(float)) != 0) return false;
  return true;
}

struct vad_ffn_plan {
  FfnDev net;        // by-value kernel argument, frag -> device buffer
  float* frag_dev;
  uint32_t* fragh_dev;  // split-f16 weights (null when the topology has none)
  float* wraw_dev;      // the weights as given (streaming hop kernel)
};

#define VAD_TRY(x)                          \
  do {                                      \
    hipError_t e_ = (x);                    \
    if (e_ != hipSuccess) return (int)e_;   \
  } while (0)

extern "C" {

const char* vad_version(void) { return "vad_amd 0.1 (gfx950)"; }

int64_t vad_n_frames(int64_t n_samples, int32_t frame_size, int32_t hop) {
  if (frame_size <= 0 || hop <= 0 || n_samples <= frame_size) return 0;
  return (n_samples - frame_size - 1) / hop + 1;  // while len - offset > frame_size
}

int vad_mfcc_plan_create(const double* fb, int32_t n_filters, int32_t fft_n, int32_t mfcc_n,
                         int32_t lifter_L, vad_mfcc_plan** out) {
  if (!fb || !out || n_filters <= 0 || mfcc_n <= 0) return VAD_EINVAL;
  if (fft_n < 2 || fft_n > VAD_MAX_FFT_N) return VAD_EUNSUPPORTED;
  if (n_filters > VAD_MAX_FILTERS || mfcc_n > VAD_MAX_MFCC || mfcc_n > n_filters)
    return VAD_EUNSUPPORTED;
  vad_mfcc_plan* p = (vad_mfcc_plan*)calloc(1, sizeof(vad_mfcc_plan));
  if (!p) return VAD_ENOMEM;
  MfccDev& h = p->host;
  h.n_filters = n_filters;
  h.mfcc_n = mfcc_n;
  p->fft_n = fft_n;
  p->bins = fft_n / 2;
  const int bins = p->bins;
  // filterbank rows -> contiguous tap ranges [first non-zero, last non-zero]
  // (NaN counts as non-zero: a degenerate reference filter stays NaN).
  int off = 0;
  std::vector<int> cost(n_filters);
  for (int m = 0; m < n_filters; ++m) {
    const double* row = fb + (size_t)m * bins;
    int lo = -1, hi = -1;
    for (int k = 0; k < bins; ++k)
      if (row[k] != 0.0) { if (lo < 0) lo = k; hi = k; }
    const int n = lo < 0 ? 0 : hi - lo + 1;
    if (off + n > VAD_MAX_TAPS) { free(p); return VAD_EUNSUPPORTED; }
    h.f_lo[m] = lo < 0 ? 0 : lo;
    h.f_len[m] = n;
    h.f_off[m] = off;
    // x 2^-20: the FFT path produces |2X|^2 and P = |X/512|^2 = |2X|^2 2^-20
    // (exact); the direct DFT of other lengths produces P itself
    const float tsc = p->generic() ? 1.f : 0x1p-20f;
    for (int t = 0; t < n; ++t) h.taps[off + t] = (float)row[lo + t] * tsc;
    off += n;
    cost[m] = n + 8;  // taps + (==0 -> eps) + log10, in VALU-op units
  }
  // balance contiguous filter bands over the 8 waves of phase 2
  {
    const int waves = 8;
    long total = 0;
    for (int m = 0; m < n_filters; ++m) total += cost[m];
    int m = 0;
    long acc = 0;
    for (int w = 0; w < 16; ++w) { h.wave_fbeg[w] = n_filters; h.wave_fend[w] = n_filters; }
    for (int w = 0; w < waves; ++w) {
      h.wave_fbeg[w] = m;
      const long target = total * (w + 1) / waves;
      while (m < n_filters && (acc + cost[m] / 2 <= target || w == waves - 1)) acc += cost[m++];
      h.wave_fend[w] = m;
    }
  }
  // lifter (mfcc.py:85-90) x DCT-II ortho (scipy.fftpack, mfcc.py:76), [c][m]
  for (int c = 0; c < kMaxCoefs; ++c) {
    const double lift = lifter_L > 0 ? 1.0 + (lifter_L / 2.0) * sin(M_PI * c / lifter_L) : 1.0;
    const double sc = c == 0 ? sqrt(1.0 / (4.0 * n_filters)) : sqrt(1.0 / (2.0 * n_filters));
    for (int m = 0; m < kMaxFilters; ++m) {
      double v = 0.0;
      if (c < mfcc_n && m < n_filters)
        v = lift * sc * 2.0 * cos(M_PI * c * (2.0 * m + 1.0) / (2.0 * n_filters));
      h.dct[c * kMaxFilters + m] = (float)v;
    }
  }
  for (int n2 = 0; n2 < 16; ++n2)
    for (int k1 = 0; k1 < 16; ++k1) {
      const double a = -2.0 * M_PI * n2 * k1 / 256.0;
      h.tw_a[n2 * 16 + k1] = make_float2((float)cos(a), (float)sin(a));
    }
  for (int k = 0; k < 256; ++k) {
    const double a = -2.0 * M_PI * k / 512.0;
    h.tw_b[k] = make_float2((float)cos(a), (float)sin(a));
  }
  p->spec = p->table_spec = p->generic() ? 0 : matches_table<Mel26>(h) ? 1 : matches_table<Mel40>(h) ? 2 : 0;
  if (p->generic()) {
    std::vector<double2> tw(fft_n);
    for (int m = 0; m < fft_n; ++m) {
      const double a = -2.0 * M_PI * (double)m / (double)fft_n;
      tw[m] = make_double2(cos(a), sin(a));
    }
    hipError_t e = hipMalloc((void**)&p->tw_gen, tw.size() * sizeof(double2));
    if (e == hipSuccess) e = hipMemcpy(p->tw_gen, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(p->tw_gen); free(p); return (int)e; }
  }
  // the streaming hop kernel's tables as one block: W512^k (256 complex);
  // per filter its first bin rounded down to 4, its tap count from there
  // rounded up to 4 and its row offset (as int bits); the 16-B aligned tap
  // rows (the filter's taps at their bins, zero around them: a lane reads
  // four taps and four power bins per pair of 16-B reads, and the zero taps
  // add +0 to a sum of non-negative terms); the DCT rows
  std::vector<float> rows;
  std::vector<int> lo4(n_filters), n4(n_filters), off4(n_filters);
  for (int m = 0; m < n_filters; ++m) {
    const int lo = h.f_lo[m], n = h.f_len[m];
    lo4[m] = lo & ~3;
    n4[m] = n > 0 ? ((lo + n + 3) & ~3) - lo4[m] : 0;
    off4[m] = (int)rows.size();
    for (int t = 0; t < n4[m]; ++t) {
      const int bin = lo4[m] + t;
      rows.push_back(bin >= lo && bin < lo + n ? h.taps[h.f_off[m] + bin - lo] : 0.f);
    }
  }
  p->n_taps = (int)rows.size();  // a multiple of 4
  std::vector<float> blob;
  for (int k = 0; k < 256; ++k) { blob.push_back(h.tw_b[k].x); blob.push_back(h.tw_b[k].y); }
  for (const std::vector<int>* arr : {&lo4, &n4, &off4})
    for (int m = 0; m < n_filters; ++m) { float f; memcpy(&f, &(*arr)[m], 4); blob.push_back(f); }
  while (blob.size() % 4) blob.push_back(0.f);
  blob.insert(blob.end(), rows.begin(), rows.end());
  // the DCT rows (16-B aligned: every tap row is a multiple of 4 floats) at
  // stride vec_row_stride(nf), zero padded
  for (int c = 0; c < mfcc_n; ++c)
    for (int m = 0; m < vec_row_stride(n_filters); ++m)
      blob.push_back(m < n_filters ? h.dct[c * kMaxFilters + m] : 0.f);
  while (blob.size() % 4) blob.push_back(0.f);
  p->hop_blob_n = (int)blob.size();
  hipError_t e = hipMalloc((void**)&p->hop_blob, blob.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(p->hop_blob, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(p->hop_blob); (void)hipFree(p->tw_gen); free(p); return (int)e; }
  e = hipMalloc((void**)&p->dev, sizeof(MfccDev));
  if (e != hipSuccess) { (void)hipFree(p->hop_blob); (void)hipFree(p->tw_gen); free(p); return (int)e; }
  e = hipMemcpy(p->dev, &h, sizeof(MfccDev), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(p->dev); (void)hipFree(p->hop_blob); (void)hipFree(p->tw_gen); free(p); return (int)e;
  }
  p->bal = balance_create();
  *out = p;
  return VAD_OK;
}

int vad_mfcc_plan_destroy(vad_mfcc_plan* p) {
  if (!p) return VAD_OK;
  balance_destroy(p->bal);
  (void)hipFree(p->dev);
  (void)hipFree(p->hop_blob);
  (void)hipFree(p->tw_gen);
  free(p);
  return VAD_OK;
}

int32_t vad_mfcc_plan_variant(const vad_mfcc_plan* p) { return p ? p->spec : -1; }

int vad_mfcc_plan_set_window(vad_mfcc_plan* p, const float* window_host, int32_t len) {
  if (!p) return VAD_EINVAL;
  if (p->generic()) return VAD_EUNSUPPORTED;  // the window multiplies the radix-16 kernels' frames
  if (window_host && (len <= 0 || len > kFftN)) return VAD_EINVAL;
  for (int t = 0; t < kFftN; ++t) p->host.window[t] = window_host && t < len ? window_host[t] : 0.f;
  const hipError_t e = hipMemcpy(p->dev->window, p->host.window, sizeof(p->host.window), hipMemcpyHostToDevice);
  if (e != hipSuccess) return (int)e;
  p->spec = window_host ? kSpecWindow : p->table_spec;
  return VAD_OK;
}

int vad_preemphasis_f32(const float* x, float* y, int64_t n_rows, int64_t row_len, int64_t row_stride,
                        float coeff, void* stream) {
  if (n_rows < 0 || row_len < 0 || row_stride < row_len) return VAD_EINVAL;
  if (n_rows == 0 || row_len == 0) return VAD_OK;
  if (!x || !y || x == y) return VAD_EINVAL;
  return (int)launch_preemphasis(x, y, n_rows, row_len, row_stride, coeff, (hipStream_t)stream);
}

int vad_mfcc_plan_set_variant(vad_mfcc_plan* p, int32_t variant) {
  if (!p) return VAD_EINVAL;
  if (p->spec == kSpecWindow) return VAD_EINVAL;  // windowed plans run the runtime-table kernel
  if (variant == 0) { p->spec = 0; return VAD_OK; }
  if (p->generic()) return VAD_EINVAL;
  if (variant == 1 && matches_table<Mel26>(p->host)) { p->spec = 1; return VAD_OK; }
  if (variant == 2 && matches_table<Mel40>(p->host)) { p->spec = 2; return VAD_OK; }
  return VAD_EINVAL;
}

static int check_frames(const vad_mfcc_plan* p, const void* src, int64_t stride, int32_t len,
                        int64_t n, const void* dst) {
  if (!p || n < 0) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!src || !dst || stride < 0 || len <= 0) return VAD_EINVAL;
  return VAD_OK;
}

int vad_spec_f32(const vad_mfcc_plan* p, const float* src, int64_t stride, int32_t len, int64_t n,
                 float* spec, void* stream) {
  int r = check_frames(p, src, stride, len, n, spec);
  if (r || n == 0) return r;
  if (p->generic()) return (int)launch_generic(1, p->dev, src, stride, len, n, p->fft_n, p->tw_gen, spec,
                                               (hipStream_t)stream);
  return (int)launch_mfcc(1, p->dev, launch_spec(p), src, stride, len, n, spec, (hipStream_t)stream);
}

int vad_mfcc_f32(const vad_mfcc_plan* p, const float* src, int64_t stride, int32_t len, int64_t n,
                 float* mfcc, void* stream) {
  int r = check_frames(p, src, stride, len, n, mfcc);
  if (r || n == 0) return r;
  if (p->generic()) return (int)launch_generic(0, p->dev, src, stride, len, n, p->fft_n, p->tw_gen, mfcc,
                                               (hipStream_t)stream);
  return (int)launch_mfcc(0, p->dev, launch_spec(p), src, stride, len, n, mfcc, (hipStream_t)stream,
                         balance_for_launch(p->bal));
}

int vad_spec_i16(const vad_mfcc_plan* p, const int16_t* src, int64_t stride, int32_t len, int64_t n,
                 float* spec, void* stream) {
  int r = check_frames(p, src, stride, len, n, spec);
  if (r || n == 0) return r;
  if (p->generic()) return (int)launch_generic_i16(1, p->dev, src, stride, len, n, p->fft_n, p->tw_gen, spec,
                                                   (hipStream_t)stream);
  return (int)launch_mfcc_i16(1, p->dev, launch_spec(p), src, stride, len, n, spec, (hipStream_t)stream);
}

int vad_mfcc_i16(const vad_mfcc_plan* p, const int16_t* src, int64_t stride, int32_t len, int64_t n,
                 float* mfcc, void* stream) {
  int r = check_frames(p, src, stride, len, n, mfcc);
  if (r || n == 0) return r;
  if (p->generic()) return (int)launch_generic_i16(0, p->dev, src, stride, len, n, p->fft_n, p->tw_gen, mfcc,
                                                   (hipStream_t)stream);
  return (int)launch_mfcc_i16(0, p->dev, launch_spec(p), src, stride, len, n, mfcc, (hipStream_t)stream,
                             balance_for_launch(p->bal));
}

int vad_mfcc_from_spec_f32(const vad_mfcc_plan* p, const float* spec, int64_t n, float* mfcc,
                           void* stream) {
  if (!p) return VAD_EINVAL;
  int r = check_frames(p, spec, p->bins, p->bins, n, mfcc);
  if (r || n == 0) return r;
  if (p->generic()) return (int)launch_generic(2, p->dev, spec, p->bins, p->bins, n, p->fft_n, p->tw_gen, mfcc,
                                               (hipStream_t)stream);
  return (int)launch_mfcc(2, p->dev, launch_spec(p), spec, kBins, kBins, n, mfcc, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// FFN plan
// ---------------------------------------------------------------------------
int vad_ffn_plan_create(int32_t n_layers, const int32_t* dims, const float* const* W,
                        const float* const* b, vad_ffn_plan** out) {
  if (!dims || !W || !b || !out || n_layers < 1) return VAD_EINVAL;
  if (n_layers > VAD_MAX_FFN_LAYERS) return VAD_EUNSUPPORTED;
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] <= 0) return VAD_EINVAL;
  if (dims[0] > 64 || dims[n_layers] > 4) return VAD_EUNSUPPORTED;
  for (int l = 1; l < n_layers; ++l)
    if (dims[l] > 64) return VAD_EUNSUPPORTED;
  for (int l = 0; l < n_layers; ++l)
    if (!W[l] || !b[l]) return VAD_EINVAL;

  FfnDev net;
  memset(&net, 0, sizeof(net));
  net.n_layers = n_layers;
  for (int l = 0; l <= n_layers; ++l) net.dims[l] = dims[l];
  net.n_classes = dims[n_layers];
  // natural shape; the kernels specialise two topologies, everything else
  // runs on a padded generic shape (ks0 16, 4 tiles per hidden layer)
  int ks0 = (dims[0] + 3) / 4;
  int tiles[VAD_MAX_FFN_LAYERS] = {0, 0, 0, 0};
  for (int l = 0; l < n_layers; ++l) tiles[l] = l + 1 < n_layers ? (dims[l + 1] + 15) / 16 : 1;
  const bool ref39 = n_layers == 4 && ks0 == 10 && tiles[0] == 4 && tiles[1] == 2 &&
                     tiles[2] == 1 && tiles[3] == 1;
  const bool bl13 = n_layers == 3 && ks0 == 4 && tiles[0] == 4 && tiles[1] == 4 && tiles[2] == 1;
  if (!ref39 && !bl13) {
    ks0 = 16;
    for (int l = 0; l < n_layers; ++l) tiles[l] = l + 1 < n_layers ? 4 : 1;
  }
  net.ks0 = ks0;
  for (int l = 0; l < VAD_MAX_FFN_LAYERS; ++l) net.tiles[l] = tiles[l];

  // fragments, in the kernels' slot order
  auto w_at = [&](int l, int k, int o) -> float {  // W_l[k][o] (Keras (in, out))
    if (k >= dims[l] || o >= dims[l + 1]) return 0.f;
    return W[l][(size_t)k * dims[l + 1] + o];
  };
  auto b_at = [&](int l, int o) -> float { return o < dims[l + 1] ? b[l][o] : 0.f; };
  std::vector<float> frag;
  auto push_slot = [&](auto fn) {
    for (int lane = 0; lane < 64; ++lane) frag.push_back(fn(lane >> 4, lane & 15));
  };
  // layer 0 A: slot mt*ks0 + s -> W0[4s + g][16mt + i]
  for (int mt = 0; mt < tiles[0]; ++mt)
    for (int s = 0; s < ks0; ++s)
      push_slot([&](int g, int i) { return w_at(0, 4 * s + g, 16 * mt + i); });
  // layer l >= 1 A: slot (mt*TI + t)*4 + r -> W_l[16t + 4g + r][16mt + i]
  for (int l = 1; l < n_layers; ++l)
    for (int mt = 0; mt < tiles[l]; ++mt)
      for (int t = 0; t < tiles[l - 1]; ++t)
        for (int r = 0; r < 4; ++r)
          push_slot([&](int g, int i) { return w_at(l, 16 * t + 4 * g + r, 16 * mt + i); });
  // biases: layer l, slot mt*4 + r -> b_l[16mt + 4g + r]
  for (int l = 0; l < n_layers; ++l)
    for (int mt = 0; mt < tiles[l]; ++mt)
      for (int r = 0; r < 4; ++r) push_slot([&](int g, int) { return b_at(l, 16 * mt + 4 * g + r); });
  // output layer on the VALU (kernels' Topo::VL: >= 2 input tiles): slot
  // (c*TIL + t)*4 + r -> W_last[16t + 4g + r][c] for 4 classes, then b_last[c]
  if (n_layers >= 2 && tiles[n_layers - 2] >= 2) {
    const int l = n_layers - 1, til = tiles[n_layers - 2];
    for (int c = 0; c < 4; ++c)
      for (int t = 0; t < til; ++t)
        for (int r = 0; r < 4; ++r)
          push_slot([&](int g, int) { return w_at(l, 16 * t + 4 * g + r, c); });
    for (int c = 0; c < 4; ++c) push_slot([&](int, int) { return b_at(l, c); });
  }

  // split-f16 weights for the specialised topologies (ffn_kernel.hip
  // dense_h3): W = hi + lo, both f16 (RNE), per (layer l, tile mt, K-step s)
  // a hi slot and a lo slot of 8 halves per lane.  A[i][k] with row i = lane
  // & 15 -> output unit 16 mt + i and k = 8 (lane >> 4) + q -> input unit
  // 32 s + k at layer 0, else 16 (2 s + (q >> 2)) + 4 (lane >> 4) + (q & 3):
  // the previous layer's accumulator rows as the lane holds them.
  std::vector<uint32_t> fragh;
  const bool use_h3 = ref39 || bl13;
  const bool merge0 = dims[0] <= 16;  // == kMerge0<KS0> of the kernels (bl13)
  if (use_h3) {
    // every layer, output included: the block kernel runs bl13's output
    // layer on the VALU and reads only the hidden layers' slots (the first
    // ones); the wave kernel runs all of them on the MFMA
    for (int l = 0; l < n_layers; ++l) {
      const int ks = l == 0 ? (dims[0] + 31) / 32 : (tiles[l - 1] + 1) / 2;
      for (int mt = 0; mt < tiles[l]; ++mt)
        for (int s = 0; s < ks; ++s)
          for (int part = 0; part < 2; ++part)
            for (int lane = 0; lane < 64; ++lane) {
              const int i = lane & 15, g = lane >> 4;
              _Float16 h[8];
              for (int q = 0; q < 8; ++q) {
                if (l == 0 && merge0) {
                  // <= 16 inputs: one K-step holds both halves of the input,
                  // k = 0..15 its hi halves, 16..31 its lo halves (ffn_dev.h
                  // dense_h3 MERGE0); part 0 = [W_hi | W_hi], part 1 = [W_lo | 0]
                  const int k = 8 * g + q;
                  const float w = w_at(0, k & 15, 16 * mt + i);
                  const _Float16 hi = (_Float16)w;
                  h[q] = part == 0 ? hi : (k < 16 ? (_Float16)(w - (float)hi) : (_Float16)0.f);
                  continue;
                }
                const int k = l == 0 ? 32 * s + 8 * g + q
                                     : 16 * (2 * s + (q >> 2)) + 4 * g + (q & 3);
                const bool in_range = l == 0 || 2 * s + (q >> 2) < tiles[l - 1];
                const float w = in_range ? w_at(l, k, 16 * mt + i) : 0.f;
                const _Float16 hi = (_Float16)w;
                h[q] = part == 0 ? hi : (_Float16)(w - (float)hi);
              }
              uint32_t word[4];
              memcpy(word, h, sizeof(word));
              for (int q = 0; q < 4; ++q) fragh.push_back(word[q]);
            }
    }
  }

  // the streaming forward's weights (FfnDev::wraw): first the weights as
  // given, W_l (in, out) row-major then b_l, with zero rows past the last
  // layer; then each W_l transposed from that flat array, row o holding
  // flat[W_l + k dout + o] for k < din rounded up to 4 -- past din these are
  // the same values (the next rows of the flat array) a four-at-a-time read
  // of the (in, out) layout met, against zero inputs, so the forward's
  // arithmetic is unchanged -- and the biases
  std::vector<float> flat;
  int flat_w[VAD_MAX_FFN_LAYERS], flat_b[VAD_MAX_FFN_LAYERS];
  for (int l = 0; l < n_layers; ++l) {
    flat_w[l] = (int)flat.size();
    flat.insert(flat.end(), W[l], W[l] + (size_t)dims[l] * dims[l + 1]);
    flat_b[l] = (int)flat.size();
    flat.insert(flat.end(), b[l], b[l] + dims[l + 1]);
  }
  flat.insert(flat.end(), 3 * 64 + 4, 0.f);
  std::vector<float> wraw;
  for (int l = 0; l < n_layers; ++l) {
    const int din = dims[l], dout = dims[l + 1], S = vec_row_stride(din);
    net.wstride[l] = S;
    net.woff[l] = (int)wraw.size();
    for (int o = 0; o < dout; ++o)
      for (int k = 0; k < S; ++k)
        wraw.push_back(k < ((din + 3) & ~3) ? flat[flat_w[l] + (size_t)k * dout + o] : 0.f);
    net.boff[l] = (int)wraw.size();
    wraw.insert(wraw.end(), b[l], b[l] + dout);
    while (wraw.size() % 4) wraw.push_back(0.f);
  }
  net.wraw_n = (int)wraw.size();
  // layer-1 inputs of a 13-input network on analyser features (|Mn| <=
  // sqrt(5), ffn_dev.h wave_tile_in_bounded): bounded by max_j |b0_j| +
  // sqrt(5) sum_k |W0[k][j]|; a bound under 32768 leaves 2x headroom to the
  // f16 range for the split-f16 rounding of layer 0 (the check it skips only
  // ever answers "scale 1" then)
  net.h1_bounded = 0;
  if (n_layers >= 2 && dims[0] == 13) {
    double worst = 0.0;
    for (int j = 0; j < dims[1]; ++j) {
      double acc = fabs((double)b[0][j]);
      for (int k = 0; k < dims[0]; ++k) acc += sqrt(5.0) * fabs((double)W[0][(size_t)k * dims[1] + j]);
      worst = acc > worst ? acc : worst;
    }
    net.h1_bounded = worst < 32768.0 ? 1 : 0;
  }

  vad_ffn_plan* p = (vad_ffn_plan*)calloc(1, sizeof(vad_ffn_plan));
  if (!p) return VAD_ENOMEM;
  hipError_t e = hipMalloc((void**)&p->wraw_dev, wraw.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(p->wraw_dev, wraw.data(), wraw.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(p->wraw_dev); free(p); return (int)e; }
  net.wraw = p->wraw_dev;
  e = hipMalloc((void**)&p->frag_dev, frag.size() * sizeof(float));
  if (e != hipSuccess) { free(p); return (int)e; }
  e = hipMemcpy(p->frag_dev, frag.data(), frag.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(p->frag_dev); (void)hipFree(p->wraw_dev); free(p); return (int)e; }
  net.frag = p->frag_dev;
  net.fragh = nullptr;
  if (!fragh.empty()) {
    e = hipMalloc((void**)&p->fragh_dev, fragh.size() * sizeof(uint32_t));
    if (e == hipSuccess)
      e = hipMemcpy(p->fragh_dev, fragh.data(), fragh.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(p->fragh_dev);
      (void)hipFree(p->frag_dev);
      (void)hipFree(p->wraw_dev);
      free(p);
      return (int)e;
    }
    net.fragh = p->fragh_dev;
  }
  p->net = net;
  *out = p;
  return VAD_OK;
}

int32_t vad_ffn_plan_arith(const vad_ffn_plan* p) {
  if (!p) return -1;
  return p->net.fragh ? VAD_FFN_SPLIT_F16 : VAD_FFN_EXACT_F32;
}

int vad_ffn_plan_set_arith(vad_ffn_plan* p, int32_t arith) {
  if (!p) return VAD_EINVAL;
  if (arith == VAD_FFN_EXACT_F32) { p->net.fragh = nullptr; return VAD_OK; }
  if (arith == VAD_FFN_SPLIT_F16 && p->fragh_dev) { p->net.fragh = p->fragh_dev; return VAD_OK; }
  return VAD_EINVAL;
}

int vad_ffn_plan_destroy(vad_ffn_plan* p) {
  if (!p) return VAD_OK;
  (void)hipFree(p->frag_dev);
  if (p->fragh_dev) (void)hipFree(p->fragh_dev);
  (void)hipFree(p->wraw_dev);
  free(p);
  return VAD_OK;
}

struct vad_tree_plan {
  TreeNode* nodes_dev;
  TreeNodeC* cnodes_dev;  // compact copy for the LDS-resident window walk
  int n_nodes;
  int n_features;
  float* score_dev;      // (n_score_classes, n_nodes) node scores, or null (vad_tree_plan_set_scores)
  int n_score_classes;
  int n_classes;         // 1 + the largest leaf class
};

int vad_tree_plan_create(int32_t n_nodes, const int32_t* feature, const double* threshold,
                         const int32_t* left, const int32_t* right, const int32_t* leaf_class,
                         const uint8_t* nan_left, int32_t n_features, vad_tree_plan** out) {
  if (!feature || !threshold || !left || !right || !leaf_class || !out || n_nodes <= 0 ||
      n_features <= 0)
    return VAD_EINVAL;
  if (n_nodes > (1 << 24) || n_features > 3 * VAD_MAX_MFCC + 16) return VAD_EUNSUPPORTED;
  std::vector<TreeNode> h((size_t)n_nodes);
  for (int i = 0; i < n_nodes; ++i) {
    TreeNode& nd = h[i];
    nd.feature = feature[i] >= 0 ? feature[i] : -1;
    nd.threshold = threshold[i];
    nd.left = left[i];
    nd.right = right[i];
    nd.leaf = (short)(leaf_class[i] < 0 || leaf_class[i] > 255 ? -1 : leaf_class[i]);
    nd.nan_left = (short)(nan_left ? (nan_left[i] != 0) : 0);
    if (nd.feature >= 0) {  // internal: children in range, feature in the row
      if (nd.feature >= n_features || nd.left <= 0 || nd.left >= n_nodes || nd.right <= 0 ||
          nd.right >= n_nodes)
        return VAD_EINVAL;
    } else if (nd.leaf < 0) {
      return VAD_EINVAL;
    }
  }
  std::vector<TreeNodeC> c((size_t)n_nodes);
  for (int i = 0; i < n_nodes; ++i) {
    const TreeNode& nd = h[i];
    TreeNodeC& cn = c[i];
    float f = (float)nd.threshold;  // round down to a float: x <= f  <=>  (double)x <= threshold
    if ((double)f > nd.threshold) f = nextafterf(f, -INFINITY);
    cn.thr = f;
    cn.feature = nd.feature >= 0 ? (nd.feature | (nd.nan_left ? 1 << 30 : 0)) : -1 - nd.leaf;
    cn.left = nd.left;
    cn.right = nd.right;
  }
  vad_tree_plan* p = (vad_tree_plan*)calloc(1, sizeof(vad_tree_plan));
  if (!p) return VAD_ENOMEM;
  hipError_t e = hipMalloc((void**)&p->nodes_dev, h.size() * sizeof(TreeNode));
  if (e != hipSuccess) { free(p); return (int)e; }
  e = hipMalloc((void**)&p->cnodes_dev, c.size() * sizeof(TreeNodeC));
  if (e != hipSuccess) { (void)hipFree(p->nodes_dev); free(p); return (int)e; }
  e = hipMemcpy(p->nodes_dev, h.data(), h.size() * sizeof(TreeNode), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(p->cnodes_dev, c.data(), c.size() * sizeof(TreeNodeC), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(p->nodes_dev);
    (void)hipFree(p->cnodes_dev);
    free(p);
    return (int)e;
  }
  p->n_nodes = n_nodes;
  p->n_features = n_features;
  for (const TreeNode& nd : h)
    if (nd.feature < 0 && nd.leaf + 1 > p->n_classes) p->n_classes = nd.leaf + 1;
  *out = p;
  return VAD_OK;
}

int vad_tree_plan_destroy(vad_tree_plan* p) {
  if (!p) return VAD_OK;
  (void)hipFree(p->nodes_dev);
  (void)hipFree(p->cnodes_dev);
  if (p->score_dev) (void)hipFree(p->score_dev);
  free(p);
  return VAD_OK;
}

// The plan's score table: row c holds, per node, the score of class index c
// (TreeClassifier.score_table(c)); the scored hop entries read row `active`.
int vad_tree_plan_set_scores(vad_tree_plan* p, const float* table, int32_t n_classes) {
  if (!p || !table || n_classes <= 0 || n_classes > 255) return VAD_EINVAL;
  float* dev = nullptr;
  const size_t bytes = (size_t)n_classes * (size_t)p->n_nodes * sizeof(float);
  hipError_t e = hipMalloc((void**)&dev, bytes);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpy(dev, table, bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(dev);
    return (int)e;
  }
  if (p->score_dev) (void)hipFree(p->score_dev);  // hipFree waits for the kernels that read it
  p->score_dev = dev;
  p->n_score_classes = n_classes;
  return VAD_OK;
}

int32_t vad_tree_plan_score_classes(const vad_tree_plan* p) { return p ? p->n_score_classes : -1; }

int vad_tree_predict(const vad_tree_plan* t, const float* x, int64_t n, uint8_t* labels,
                     void* stream) {
  if (!t || n < 0) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!x || !labels) return VAD_EINVAL;
  return (int)launch_tree_rows(t->nodes_dev, t->n_nodes, x, n, t->n_features, labels,
                               (hipStream_t)stream);
}

int vad_features_tree(const vad_tree_plan* t, const float* mfcc, int64_t n_frames, int32_t mfcc_n,
                      int32_t mode, uint8_t* labels, void* stream) {
  if (!t || n_frames < 0 || mfcc_n <= 0 || mfcc_n > VAD_MAX_MFCC || (mode != 0 && mode != 1))
    return VAD_EINVAL;
  if (t->n_features > 3 * mfcc_n) return VAD_EINVAL;
  const int64_t rows = n_frames > 5 ? n_frames - 5 : 0;
  if (rows == 0) return VAD_OK;
  if (!mfcc || !labels) return VAD_EINVAL;
  return (int)launch_tree_windows(t->nodes_dev, t->cnodes_dev, t->n_nodes, mfcc, rows, mfcc_n, mode, labels,
                                  (hipStream_t)stream);
}

// The tree's scores (score_kernel.hip): the two entries above with the leaf's
// entry of node_score written in place of its class.
int vad_tree_predict_scores(const vad_tree_plan* t, const float* node_score, const float* x, int64_t n,
                            float* scores, void* stream) {
  if (!t || n < 0) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!x || !scores || !node_score) return VAD_EINVAL;
  if (n > INT64_MAX / 4 / t->n_features || overlap(x, (size_t)n * t->n_features * 4, scores, (size_t)n * 4))
    return VAD_EINVAL;
  return (int)launch_tree_row_scores(t->nodes_dev, t->n_nodes, node_score, x, n, t->n_features, scores,
                                     (hipStream_t)stream);
}

int vad_features_tree_scores(const vad_tree_plan* t, const float* node_score, const float* mfcc, int64_t n_frames,
                             int32_t mfcc_n, int32_t mode, float* scores, void* stream) {
  if (!t || n_frames < 0 || mfcc_n <= 0 || mfcc_n > VAD_MAX_MFCC || (mode != 0 && mode != 1))
    return VAD_EINVAL;
  if (t->n_features > 3 * mfcc_n) return VAD_EINVAL;
  const int64_t rows = n_frames > 5 ? n_frames - 5 : 0;
  if (rows == 0) return VAD_OK;
  if (!mfcc || !scores || !node_score) return VAD_EINVAL;
  if (n_frames > INT64_MAX / 64 || overlap(mfcc, (size_t)n_frames * mfcc_n * 4, scores, (size_t)rows * 4))
    return VAD_EINVAL;
  return (int)launch_tree_window_scores(t->nodes_dev, t->cnodes_dev, t->n_nodes, node_score, mfcc, rows, mfcc_n,
                                        mode, scores, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// Random forest (forest_kernel.hip)
// ---------------------------------------------------------------------------
struct vad_forest {
  TreeNode* nodes_dev;
  TreeNodeC* cnodes_dev;  // compact copy for the LDS-resident window walk
  int* roots_dev;         // n_trees + 1
  double* proba_dev;      // (n_nodes, n_classes)
  int n_nodes;
  int n_trees;
  int n_classes;
  int n_features;
  int max_lds_tree;  // nodes of the largest tree the window kernel stages in LDS
  int max_tree;      // nodes of the largest tree
  int* roots_host;   // n_trees + 1: the hop kernels' staging rule reads it (stream_forest_lds_trees)
};

int vad_forest_create(int32_t n_nodes, const int32_t* feature, const double* threshold, const int32_t* left,
                      const int32_t* right, const uint8_t* nan_left, int32_t n_trees, const int32_t* roots,
                      int32_t n_classes, const double* proba, int32_t n_features, vad_forest** out) {
  if (!feature || !threshold || !left || !right || !roots || !proba || !out || n_nodes <= 0 || n_features <= 0 ||
      n_trees < 1 || n_classes < 1 || n_classes > VAD_FOREST_MAX_CLASSES)
    return VAD_EINVAL;
  if (n_nodes > (1 << 24) || n_features > 3 * VAD_MAX_MFCC + 16) return VAD_EUNSUPPORTED;
  if (n_trees > n_nodes || roots[0] != 0) return VAD_EINVAL;
  for (int t = 1; t < n_trees; ++t)
    if (roots[t] <= roots[t - 1] || roots[t] >= n_nodes) return VAD_EINVAL;
  std::vector<int> r(roots, roots + n_trees);
  r.push_back(n_nodes);
  std::vector<TreeNode> h((size_t)n_nodes);
  std::vector<TreeNodeC> c((size_t)n_nodes);
  int max_lds_tree = 0, max_tree = 0;
  for (int t = 0; t < n_trees; ++t) {
    const int lo = r[t], hi = r[t + 1];
    if (hi - lo > max_tree) max_tree = hi - lo;
    if (hi - lo <= 3072 && hi - lo > max_lds_tree) max_lds_tree = hi - lo;  // kLdsNodes of the tree kernels
    for (int i = lo; i < hi; ++i) {
      TreeNode& nd = h[i];
      nd.feature = feature[i] >= 0 ? feature[i] : -1;
      nd.threshold = threshold[i];
      nd.leaf = 0;
      nd.nan_left = (short)(nan_left ? (nan_left[i] != 0) : 0);
      nd.left = nd.right = -1;
      TreeNodeC& cn = c[i];
      cn.thr = 0.f;
      cn.feature = -1;
      cn.left = cn.right = -1;
      if (nd.feature < 0) continue;
      // internal: the children inside the tree and past its root, the feature in the row
      if (nd.feature >= n_features || left[i] <= lo || left[i] >= hi || right[i] <= lo || right[i] >= hi)
        return VAD_EINVAL;
      nd.left = left[i] - lo;
      nd.right = right[i] - lo;
      float f = (float)nd.threshold;  // round down to a float: x <= f  <=>  (double)x <= threshold
      if ((double)f > nd.threshold) f = nextafterf(f, -INFINITY);
      cn.thr = f;
      cn.feature = nd.feature | (nd.nan_left ? 1 << 30 : 0);
      cn.left = nd.left;
      cn.right = nd.right;
    }
  }
  vad_forest* p = (vad_forest*)calloc(1, sizeof(vad_forest));
  if (!p) return VAD_ENOMEM;
  const size_t pb = (size_t)n_nodes * (size_t)n_classes * sizeof(double);
  p->roots_host = (int*)malloc(r.size() * sizeof(int));
  if (!p->roots_host) {
    free(p);
    return VAD_ENOMEM;
  }
  memcpy(p->roots_host, r.data(), r.size() * sizeof(int));
  hipError_t e = hipMalloc((void**)&p->nodes_dev, h.size() * sizeof(TreeNode));
  if (e == hipSuccess) e = hipMalloc((void**)&p->cnodes_dev, c.size() * sizeof(TreeNodeC));
  if (e == hipSuccess) e = hipMalloc((void**)&p->roots_dev, r.size() * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&p->proba_dev, pb);
  if (e == hipSuccess) e = hipMemcpy(p->nodes_dev, h.data(), h.size() * sizeof(TreeNode), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->cnodes_dev, c.data(), c.size() * sizeof(TreeNodeC), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->roots_dev, r.data(), r.size() * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(p->proba_dev, proba, pb, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    vad_forest_destroy(p);
    return (int)e;
  }
  p->n_nodes = n_nodes;
  p->n_trees = n_trees;
  p->n_classes = n_classes;
  p->n_features = n_features;
  p->max_lds_tree = max_lds_tree;
  p->max_tree = max_tree;
  *out = p;
  return VAD_OK;
}

int vad_forest_destroy(vad_forest* p) {
  if (!p) return VAD_OK;
  if (p->nodes_dev) (void)hipFree(p->nodes_dev);
  if (p->cnodes_dev) (void)hipFree(p->cnodes_dev);
  if (p->roots_dev) (void)hipFree(p->roots_dev);
  if (p->proba_dev) (void)hipFree(p->proba_dev);
  free(p->roots_host);
  free(p);
  return VAD_OK;
}

static ForestDev forest_dev(const vad_forest* p) {
  return ForestDev{p->nodes_dev, p->cnodes_dev, p->roots_dev, p->proba_dev, p->n_trees, p->n_classes};
}

int vad_forest_predict(const vad_forest* f, const float* x, int64_t n, int32_t active, uint8_t* labels, float* scores,
                       void* stream) {
  if (!f || n < 0 || active < 0 || active >= f->n_classes) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!x || !labels) return VAD_EINVAL;
  if (n > INT64_MAX / 4 / f->n_features) return VAD_EINVAL;
  const size_t xb = (size_t)n * f->n_features * 4;
  if (overlap(x, xb, labels, (size_t)n) || overlap(x, xb, scores, scores ? (size_t)n * 4 : 0) ||
      overlap(labels, (size_t)n, scores, scores ? (size_t)n * 4 : 0))
    return VAD_EINVAL;
  return (int)launch_forest_rows(forest_dev(f), x, n, f->n_features, active, labels, scores, (hipStream_t)stream);
}

int vad_features_forest(const vad_forest* f, const float* mfcc, int64_t n_frames, int32_t mfcc_n, int32_t mode,
                        int32_t active, uint8_t* labels, float* scores, void* stream) {
  if (!f || n_frames < 0 || mfcc_n <= 0 || mfcc_n > VAD_MAX_MFCC || (mode != 0 && mode != 1) || active < 0 ||
      active >= f->n_classes)
    return VAD_EINVAL;
  if (f->n_features > 3 * mfcc_n) return VAD_EINVAL;
  const int64_t rows = n_frames > 5 ? n_frames - 5 : 0;
  if (rows == 0) return VAD_OK;
  if (!mfcc || !labels || n_frames > INT64_MAX / 64) return VAD_EINVAL;
  const size_t mb = (size_t)n_frames * mfcc_n * 4;
  if (overlap(mfcc, mb, labels, (size_t)rows) || overlap(mfcc, mb, scores, scores ? (size_t)rows * 4 : 0) ||
      overlap(labels, (size_t)rows, scores, scores ? (size_t)rows * 4 : 0))
    return VAD_EINVAL;
  return (int)launch_forest_windows(forest_dev(f), f->max_lds_tree, mfcc, rows, mfcc_n, mode, active, labels, scores,
                                    (hipStream_t)stream);
}

int vad_simple_features(const float* frames, int64_t n_frames, int32_t frame_len,
                        int64_t frame_stride, int32_t fft_len, int32_t pad, int32_t band_bins,
                        int32_t n_bands, double* out, void* stream) {
  if (n_frames < 0 || frame_len < 2 || pad < 0 || frame_stride < 0 || band_bins < 1 || n_bands < 0)
    return VAD_EINVAL;
  if (fft_len != frame_len + 2 * pad || frame_len > 8192 || fft_len > 8193 || n_bands * band_bins > fft_len)
    return VAD_EUNSUPPORTED;
  if (n_frames == 0) return VAD_OK;
  if (!frames || !out) return VAD_EINVAL;
  return (int)launch_simple_features(frames, n_frames, frame_len, frame_stride, fft_len, pad,
                                     band_bins, n_bands, out, (hipStream_t)stream);
}

// Streams of that analyser (simple_stream_kernel.hip): every argument is
// checked before the first launch.
size_t vad_simple_stream_state_bytes(int32_t noise_buf_len) {
  if (noise_buf_len < 1 || noise_buf_len > VAD_SIMPLE_MAX_NOISE) return 0;
  return (size_t)(6 * noise_buf_len + 6) * sizeof(double) + 4 * sizeof(int32_t);
}

static bool simple_stream_common_ok(int64_t n_streams, int32_t noise_buf_len, const void* state) {
  return n_streams >= 1 && vad_simple_stream_state_bytes(noise_buf_len) != 0 && state &&
         reinterpret_cast<uintptr_t>(state) % 8 == 0;
}

int vad_simple_stream_init(const double* feats, int64_t n_streams, int32_t noise_buf_len, void* state, void* stream) {
  if (!simple_stream_common_ok(n_streams, noise_buf_len, state) || !feats) return VAD_EINVAL;
  return (int)launch_simple_stream_init(feats, n_streams, noise_buf_len, state, (hipStream_t)stream);
}

// The session words of the sessions entries: all three, the int32 ones aligned.
static bool simple_sessions_ok(const int32_t* frame_counts, const uint8_t* restart, const int32_t* init_left) {
  return frame_counts && restart && init_left && reinterpret_cast<uintptr_t>(frame_counts) % 4 == 0 &&
         reinterpret_cast<uintptr_t>(init_left) % 4 == 0;
}

static int simple_stream_state_entry(const double* feats, int64_t n_streams, int32_t n_frames, int32_t noise_buf_len,
                                     void* state, uint8_t* labels, int64_t label_block_stride, bool sessions,
                                     const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                     void* stream) {
  if (!simple_stream_common_ok(n_streams, noise_buf_len, state) || n_frames < 0 || !feats || !labels)
    return VAD_EINVAL;
  if (n_frames > 1 && label_block_stride < n_streams) return VAD_EINVAL;
  if (sessions && !simple_sessions_ok(frame_counts, restart, init_left)) return VAD_EINVAL;
  if (n_frames == 0) return VAD_OK;
  return (int)launch_simple_stream_state(feats, n_streams, n_frames, noise_buf_len, state, labels, label_block_stride,
                                         nullptr, 0, 0, 0, nullptr, 0, nullptr, frame_counts, restart, init_left,
                                         (hipStream_t)stream);
}

int vad_simple_stream_state(const double* feats, int64_t n_streams, int32_t n_frames, int32_t noise_buf_len,
                            void* state, uint8_t* labels, int64_t label_block_stride, void* stream) {
  return simple_stream_state_entry(feats, n_streams, n_frames, noise_buf_len, state, labels, label_block_stride,
                                   false, nullptr, nullptr, nullptr, stream);
}

int vad_simple_stream_state_sessions(const double* feats, int64_t n_streams, int32_t n_frames, int32_t noise_buf_len,
                                     void* state, uint8_t* labels, int64_t label_block_stride,
                                     const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                     void* stream) {
  return simple_stream_state_entry(feats, n_streams, n_frames, noise_buf_len, state, labels, label_block_stride, true,
                                   frame_counts, restart, init_left, stream);
}

static int simple_stream_block_entry(const void* frames, int in_bytes, int64_t block_stride, int64_t stream_stride,
                                     int32_t frame_len, int32_t fft_len, int32_t pad, int32_t band_bins,
                                     int64_t n_streams, int32_t n_frames, int32_t noise_buf_len, void* state,
                                     uint8_t* labels, int64_t label_block_stride, double* features_out, void* voiced,
                                     int64_t voiced_stride, int32_t* voiced_len, bool sessions,
                                     const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                     void* stream) {
  if (!simple_stream_common_ok(n_streams, noise_buf_len, state) || n_frames < 0 || !frames || !labels)
    return VAD_EINVAL;
  if (sessions && !simple_sessions_ok(frame_counts, restart, init_left)) return VAD_EINVAL;
  if (frame_len < 2 || frame_len > 8192 || pad < 0 || fft_len != frame_len + 2 * pad || fft_len > 8193)
    return VAD_EINVAL;
  if (band_bins < 1 || 4 * (int64_t)band_bins > fft_len) return VAD_EINVAL;  // "FFTN is small"
  if ((voiced == nullptr) != (voiced_len == nullptr)) return VAD_EINVAL;
  if ((int64_t)n_frames * frame_len > INT32_MAX) return VAD_EINVAL;
  if (stream_stride < 0 || (n_streams > 1 && stream_stride < frame_len)) return VAD_EINVAL;
  if (n_frames > 1) {
    if (!vad_hop_layout_disjoint(n_streams, n_frames, block_stride, stream_stride, frame_len)) return VAD_EINVAL;
    if (label_block_stride < n_streams) return VAD_EINVAL;
  }
  if (voiced && n_streams > 1 && voiced_stride < (int64_t)n_frames * frame_len) return VAD_EINVAL;
  const bool one_kernel = simple_stream_block_fits(fft_len);
  if (!one_kernel && (in_bytes != 4 || !features_out)) return VAD_EINVAL;
  if (n_frames == 0) return VAD_OK;
  hipStream_t st = (hipStream_t)stream;
  if (one_kernel)
    return (int)launch_simple_stream_block(frames, in_bytes, block_stride, stream_stride, frame_len, fft_len, pad,
                                           band_bins, n_streams, n_frames, noise_buf_len, state, labels,
                                           label_block_stride, features_out, voiced, voiced_stride, voiced_len,
                                           frame_counts, restart, init_left, st);
  // any other length: the rows of every (frame, stream) pair, then the state steps
  const float* x = static_cast<const float*>(frames);
  if (n_frames == 1 || block_stride == n_streams * stream_stride) {
    VAD_TRY(launch_simple_features(x, (int64_t)n_frames * n_streams, frame_len, stream_stride, fft_len, pad,
                                   band_bins, 4, features_out, st));
  } else {
    for (int32_t k = 0; k < n_frames; ++k)
      VAD_TRY(launch_simple_features(x + k * block_stride, n_streams, frame_len, stream_stride, fft_len, pad,
                                     band_bins, 4, features_out + (int64_t)k * n_streams * 7, st));
  }
  return (int)launch_simple_stream_state(features_out, n_streams, n_frames, noise_buf_len, state, labels,
                                         label_block_stride, x, block_stride, stream_stride, frame_len,
                                         static_cast<float*>(voiced), voiced_stride, voiced_len, frame_counts, restart,
                                         init_left, st);
}

int vad_simple_stream_block_f32(const float* frames, int64_t block_stride, int64_t stream_stride, int32_t frame_len,
                                int32_t fft_len, int32_t pad, int32_t band_bins, int64_t n_streams, int32_t n_frames,
                                int32_t noise_buf_len, void* state, uint8_t* labels, int64_t label_block_stride,
                                double* features_out, float* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                void* stream) {
  return simple_stream_block_entry(frames, 4, block_stride, stream_stride, frame_len, fft_len, pad, band_bins,
                                   n_streams, n_frames, noise_buf_len, state, labels, label_block_stride,
                                   features_out, voiced, voiced_stride, voiced_len, false, nullptr, nullptr, nullptr,
                                   stream);
}

int vad_simple_stream_block_i16(const int16_t* frames, int64_t block_stride, int64_t stream_stride, int32_t frame_len,
                                int32_t fft_len, int32_t pad, int32_t band_bins, int64_t n_streams, int32_t n_frames,
                                int32_t noise_buf_len, void* state, uint8_t* labels, int64_t label_block_stride,
                                double* features_out, int16_t* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                void* stream) {
  return simple_stream_block_entry(frames, 2, block_stride, stream_stride, frame_len, fft_len, pad, band_bins,
                                   n_streams, n_frames, noise_buf_len, state, labels, label_block_stride,
                                   features_out, voiced, voiced_stride, voiced_len, false, nullptr, nullptr, nullptr,
                                   stream);
}

int vad_simple_stream_block_sessions_f32(const float* frames, int64_t block_stride, int64_t stream_stride,
                                         int32_t frame_len, int32_t fft_len, int32_t pad, int32_t band_bins,
                                         int64_t n_streams, int32_t n_frames, int32_t noise_buf_len, void* state,
                                         uint8_t* labels, int64_t label_block_stride, double* features_out,
                                         float* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                         const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                         void* stream) {
  return simple_stream_block_entry(frames, 4, block_stride, stream_stride, frame_len, fft_len, pad, band_bins,
                                   n_streams, n_frames, noise_buf_len, state, labels, label_block_stride,
                                   features_out, voiced, voiced_stride, voiced_len, true, frame_counts, restart,
                                   init_left, stream);
}

int vad_simple_stream_block_sessions_i16(const int16_t* frames, int64_t block_stride, int64_t stream_stride,
                                         int32_t frame_len, int32_t fft_len, int32_t pad, int32_t band_bins,
                                         int64_t n_streams, int32_t n_frames, int32_t noise_buf_len, void* state,
                                         uint8_t* labels, int64_t label_block_stride, double* features_out,
                                         int16_t* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                         const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                         void* stream) {
  return simple_stream_block_entry(frames, 2, block_stride, stream_stride, frame_len, fft_len, pad, band_bins,
                                   n_streams, n_frames, noise_buf_len, state, labels, label_block_stride,
                                   features_out, voiced, voiced_stride, voiced_len, true, frame_counts, restart,
                                   init_left, stream);
}

size_t vad_scale_workspace_bytes(void) { return scale_workspace_bytes(); }

int vad_scale_features(float* rows, int64_t n_rows, int32_t mfcc_n, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (n_rows < 0 || mfcc_n <= 0 || mfcc_n > VAD_MAX_MFCC) return VAD_EINVAL;
  if (n_rows == 0) return VAD_OK;
  if (!rows || !workspace || workspace_bytes < scale_workspace_bytes()) return VAD_EINVAL;
  return (int)launch_scale_features(rows, n_rows, mfcc_n, (double*)workspace, (hipStream_t)stream);
}

int64_t vad_format_csv_rows(const float* rows, int64_t n_rows, int32_t n_cols, double label,
                            char* buf, int64_t buf_size) {
  if (n_rows < 0 || n_cols <= 0 || (n_rows > 0 && !rows)) return VAD_EINVAL;
  if (n_rows == 0) return 0;
  return format_csv_rows(rows, n_rows, n_cols, label, buf, buf_size);
}

size_t vad_csv_workspace_bytes(int64_t n_bytes) { return csv_workspace_bytes(n_bytes); }

static bool csv_ws_ok(const void* ws, size_t ws_bytes, int64_t n_bytes) {
  return ws && reinterpret_cast<uintptr_t>(ws) % 8 == 0 && ws_bytes >= csv_workspace_bytes(n_bytes);
}

int vad_csv_count_lines(const uint8_t* bytes, int64_t n_bytes, int64_t* n_lines, void* ws, size_t ws_bytes,
                        void* stream) {
  if (n_bytes < 0 || n_bytes > (int64_t)1 << 42 || (n_bytes > 0 && !bytes) || !n_lines) return VAD_EINVAL;
  if (reinterpret_cast<uintptr_t>(n_lines) % 8 || !csv_ws_ok(ws, ws_bytes, n_bytes)) return VAD_EINVAL;
  return (int)launch_csv_count(bytes, n_bytes, n_lines, ws, (hipStream_t)stream);
}

int vad_csv_index(const uint8_t* bytes, int64_t n_bytes, int64_t skip, int64_t base, int64_t* index,
                  int64_t capacity, const void* ws, size_t ws_bytes, void* stream) {
  if (n_bytes < 0 || n_bytes > (int64_t)1 << 42 || (n_bytes > 0 && !bytes)) return VAD_EINVAL;
  if (skip < 0 || base < 0 || capacity < 0 || (capacity > 0 && !index)) return VAD_EINVAL;
  if (reinterpret_cast<uintptr_t>(index) % 8 || !csv_ws_ok(ws, ws_bytes, n_bytes)) return VAD_EINVAL;
  return (int)launch_csv_index(bytes, n_bytes, skip, base, index, capacity, ws, (hipStream_t)stream);
}

int vad_csv_parse(const uint8_t* bytes, int64_t n_bytes, const int64_t* index, int64_t n_rows, int64_t base,
                  int32_t n_cols, const int32_t* columns, int32_t n_used, int32_t out_f64, void* X, uint8_t* y,
                  int32_t* row_status, void* stream) {
  if (n_bytes < 0 || n_rows < 0 || base < 0 || n_cols < 2 || n_cols > VAD_CSV_MAX_COLS) return VAD_EINVAL;
  if (n_used < 1 || n_used > VAD_CSV_MAX_USED || (!columns && n_used != n_cols - 1)) return VAD_EINVAL;
  for (int j = 0; columns && j < n_used; ++j)
    if (columns[j] < 0 || columns[j] >= n_cols) return VAD_EINVAL;
  if (n_rows > 0 && (!bytes || !index || !X || !y || !row_status || n_bytes == 0)) return VAD_EINVAL;
  if (reinterpret_cast<uintptr_t>(index) % 8 || reinterpret_cast<uintptr_t>(X) % (out_f64 ? 8 : 4) ||
      reinterpret_cast<uintptr_t>(row_status) % 4)
    return VAD_EINVAL;
  return (int)launch_csv_parse(bytes, n_bytes, index, n_rows, base, n_cols, columns, n_used, out_f64 != 0, X, y,
                               row_status, (hipStream_t)stream);
}

int vad_features_f32(const float* mfcc, int64_t n_frames, int32_t mfcc_n, int32_t mode,
                     float* features, void* stream) {
  if (n_frames < 0 || mfcc_n <= 0 || mfcc_n > VAD_MAX_MFCC || (mode != 0 && mode != 1))
    return VAD_EINVAL;
  const int64_t rows = n_frames > 5 ? n_frames - 5 : 0;
  if (rows == 0) return VAD_OK;
  if (!mfcc || !features) return VAD_EINVAL;
  return (int)launch_features(mfcc, rows, mfcc_n, mode, features, (hipStream_t)stream);
}

int vad_features_ffn(const vad_ffn_plan* ffn, const float* mfcc, int64_t n_frames, int32_t mfcc_n,
                     int32_t mode, uint8_t* labels, void* stream) {
  if (!ffn || n_frames < 0 || mfcc_n <= 0 || mfcc_n > VAD_MAX_MFCC || (mode != 0 && mode != 1))
    return VAD_EINVAL;
  if (ffn->net.dims[0] > 3 * mfcc_n) return VAD_EINVAL;
  const int64_t rows = n_frames > 5 ? n_frames - 5 : 0;
  if (rows == 0) return VAD_OK;
  if (!mfcc || !labels) return VAD_EINVAL;
  return (int)launch_ffn(ffn->net, 0, mfcc, rows, mfcc_n, mode, labels, (hipStream_t)stream);
}

int vad_features_ffn_logits(const vad_ffn_plan* ffn, const float* mfcc, int64_t n_frames, int32_t mfcc_n,
                            int32_t mode, uint8_t* labels, float* logits, void* stream) {
  if (!ffn || n_frames < 0 || mfcc_n <= 0 || mfcc_n > VAD_MAX_MFCC || (mode != 0 && mode != 1))
    return VAD_EINVAL;
  if (ffn->net.dims[0] > 3 * mfcc_n) return VAD_EINVAL;
  const int64_t rows = n_frames > 5 ? n_frames - 5 : 0;
  if (rows == 0) return VAD_OK;
  if (!mfcc || !labels || !logits) return VAD_EINVAL;
  FfnDev net = ffn->net;
  net.logits = logits;
  return (int)launch_ffn(net, 0, mfcc, rows, mfcc_n, mode, labels, (hipStream_t)stream);
}

int vad_ffn_predict(const vad_ffn_plan* ffn, const float* x, int64_t n, uint8_t* labels,
                    void* stream) {
  if (!ffn || n < 0) return VAD_EINVAL;
  if (n == 0) return VAD_OK;
  if (!x || !labels) return VAD_EINVAL;
  return (int)launch_ffn(ffn->net, 1, x, n, 0, 0, labels, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// FFN training
// ---------------------------------------------------------------------------
static bool train_shape_ok(int32_t n_layers, const int32_t* dims) {
  if (!dims || n_layers < 1 || n_layers > VAD_MAX_FFN_LAYERS) return false;
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] < 1 || dims[l] > 64) return false;
  return dims[n_layers] <= 4;
}

int64_t vad_ffn_train_param_count(int32_t n_layers, const int32_t* dims) {
  if (!train_shape_ok(n_layers, dims)) return -1;
  int64_t c = 0;
  for (int l = 0; l < n_layers; ++l) c += (int64_t)dims[l] * dims[l + 1] + dims[l + 1];
  return c;
}

int vad_ffn_train_steps(int32_t n_layers, const int32_t* dims, float* state, int64_t n_models, const float* x,
                        const uint8_t* y, int64_t n_rows, const int32_t* order, int64_t order_model_stride,
                        int32_t batch, int64_t n_steps, const float* hyper, float* step_loss, void* stream) {
  if (!train_shape_ok(n_layers, dims) || batch < 1 || batch > 64) return VAD_EINVAL;
  if (n_models < 0 || n_models > INT32_MAX || n_rows < 0 || n_steps < 0 || order_model_stride < 0) return VAD_EINVAL;
  if (n_steps > INT64_MAX / 64) return VAD_EINVAL;
  if (order_model_stride != 0 && order_model_stride < n_steps * batch) return VAD_EINVAL;
  if (n_models == 0 || n_steps == 0) return VAD_OK;
  if (!state || !x || !y || !order || !hyper || n_rows == 0) return VAD_EINVAL;
  if (ffn_train_lds_bytes(n_layers, dims, batch, true) > 160 * 1024) return VAD_EUNSUPPORTED;
  return (int)launch_ffn_train(n_layers, dims, state, n_models, x, y, order, order_model_stride, batch, n_steps,
                               hyper, step_loss, (hipStream_t)stream);
}

int64_t vad_ffn_train_eval_chunks(int64_t n_rows) {
  if (n_rows < 0) return -1;
  return n_rows / VAD_TRAIN_EVAL_CHUNK_ROWS + (n_rows % VAD_TRAIN_EVAL_CHUNK_ROWS != 0);
}

int vad_ffn_train_eval(int32_t n_layers, const int32_t* dims, const float* state, int64_t n_models, const float* x,
                       const uint8_t* y, int64_t n_rows, float* loss_sums, int32_t* correct, void* stream) {
  if (!train_shape_ok(n_layers, dims) || n_models < 0 || n_rows < 0) return VAD_EINVAL;
  if (n_models == 0 || n_rows == 0) return VAD_OK;
  if (!state || !x || !y || !loss_sums || !correct) return VAD_EINVAL;
  const int64_t n_chunks = vad_ffn_train_eval_chunks(n_rows);
  if (n_models > INT32_MAX / n_chunks) return VAD_EUNSUPPORTED;
  if (ffn_train_lds_bytes(n_layers, dims, 64, false) > 160 * 1024) return VAD_EUNSUPPORTED;
  return (int)launch_ffn_eval(n_layers, dims, state, n_models, x, y, n_rows, n_chunks, loss_sums, correct,
                              (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// Decision-tree training
// ---------------------------------------------------------------------------
int64_t vad_tree_train_node_capacity(int64_t n_rows, int32_t min_samples_leaf) {
  if (n_rows < 1 || min_samples_leaf < 1) return -1;
  const int64_t c = 2 * (n_rows / min_samples_leaf) - 1;
  return c < 1 ? 1 : c;
}

static bool tree_train_shape_ok(int64_t n_rows, int32_t n_features, int32_t n_classes, int32_t n_jobs,
                                const vad_tree_job* jobs) {
  if (n_rows < 1 || n_rows >= (1ll << VAD_TREE_TRAIN_ROW_BITS)) return false;
  if (n_features < 1 || n_features > 64 || n_classes < 2 || n_classes > VAD_TREE_TRAIN_MAX_CLASSES) return false;
  if (n_jobs < 1 || n_jobs > 4096 || !jobs) return false;
  int64_t nodes = 0;
  int single = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const vad_tree_job& b = jobs[j];
    if (b.n_rows < 1 || b.n_rows > n_rows || b.max_depth < 1 || b.min_samples_split < 2 || b.min_samples_leaf < 1 ||
        b.reserved != 0)
      return false;
    if (b.node_capacity < 1 || b.node_capacity > (1 << 28)) return false;
    nodes += b.node_capacity;
    single += b.n_rows == 1;
  }
  return nodes < (1ll << 31) && single <= 1024;
}

size_t vad_tree_train_workspace_bytes(int64_t n_rows, int32_t n_features, int32_t n_classes, int32_t n_jobs,
                                      const vad_tree_job* jobs) {
  if (!tree_train_shape_ok(n_rows, n_features, n_classes, n_jobs, jobs)) return 0;
  return tree_train_ws_bytes(n_rows, n_features, n_jobs, jobs);
}

int vad_tree_train(const float* x, const uint8_t* y, int64_t n_rows, int32_t n_features, int32_t n_classes,
                   const int32_t* order, const uint8_t* mask, int32_t n_jobs, const vad_tree_job* jobs,
                   const vad_tree_tables* tables, void* workspace, size_t workspace_bytes, int32_t* n_levels,
                   void* stream) {
  return vad_tree_train_features(x, y, n_rows, n_features, n_classes, order, mask, nullptr, n_jobs, jobs, tables,
                                 workspace, workspace_bytes, n_levels, stream);
}

int vad_tree_train_features(const float* x, const uint8_t* y, int64_t n_rows, int32_t n_features, int32_t n_classes,
                            const int32_t* order, const uint8_t* mask, const uint64_t* feature_masks, int32_t n_jobs,
                            const vad_tree_job* jobs, const vad_tree_tables* tables, void* workspace,
                            size_t workspace_bytes, int32_t* n_levels, void* stream) {
  if (!tree_train_shape_ok(n_rows, n_features, n_classes, n_jobs, jobs)) return VAD_EINVAL;
  if (feature_masks) {  // every job needs a feature it may split on
    const uint64_t all = n_features == 64 ? ~0ull : (1ull << n_features) - 1;
    for (int j = 0; j < n_jobs; ++j)
      if (!(feature_masks[j] & all)) return VAD_EINVAL;
  }
  if (!x || !y || !order || !tables || !workspace) return VAD_EINVAL;
  const vad_tree_tables& t = *tables;
  if (!t.feature || !t.threshold || !t.left || !t.right || !t.leaf || !t.nan_left || !t.n_node_samples || !t.depth ||
      !t.value || !t.n_nodes || !t.status)
    return VAD_EINVAL;
  if (((uintptr_t)workspace & 255) || ((uintptr_t)t.threshold & 7)) return VAD_EINVAL;
  if (!mask)
    for (int j = 0; j < n_jobs; ++j)
      if (jobs[j].n_rows != n_rows) return VAD_EINVAL;
  const size_t need = tree_train_ws_bytes(n_rows, n_features, n_jobs, jobs);
  if (need == 0) return VAD_EUNSUPPORTED;
  if (workspace_bytes < need) return VAD_EINVAL;
  return tree_train_run(x, y, n_rows, n_features, n_classes, order, mask, feature_masks, n_jobs, jobs, t, workspace,
                        workspace_bytes, n_levels, (hipStream_t)stream);
}

size_t vad_tree_train_weighted_workspace_bytes(int64_t n_rows, int32_t n_features, int32_t n_classes, int32_t n_jobs,
                                               const vad_tree_job* jobs) {
  if (!tree_train_shape_ok(n_rows, n_features, n_classes, n_jobs, jobs)) return 0;
  return tree_train_ws_bytes(n_rows, n_features, n_jobs, jobs, true);
}

int vad_tree_train_weighted(const float* x, const uint8_t* y, int64_t n_rows, int32_t n_features, int32_t n_classes,
                            const int32_t* order, const uint8_t* weights, const uint64_t* feature_masks,
                            int32_t n_jobs, const vad_tree_job* jobs, const vad_tree_tables* tables, void* workspace,
                            size_t workspace_bytes, int32_t* n_levels, void* stream) {
  if (!tree_train_shape_ok(n_rows, n_features, n_classes, n_jobs, jobs)) return VAD_EINVAL;  // (n_rows of 0 included)
  if (feature_masks) {
    const uint64_t all = n_features == 64 ? ~0ull : (1ull << n_features) - 1;
    for (int j = 0; j < n_jobs; ++j)
      if (!(feature_masks[j] & all)) return VAD_EINVAL;
  }
  if (!x || !y || !order || !tables || !workspace) return VAD_EINVAL;
  const vad_tree_tables& t = *tables;
  if (!t.feature || !t.threshold || !t.left || !t.right || !t.leaf || !t.nan_left || !t.n_node_samples || !t.depth ||
      !t.value || !t.n_nodes || !t.status)
    return VAD_EINVAL;
  if (((uintptr_t)workspace & 255) || ((uintptr_t)t.threshold & 7)) return VAD_EINVAL;
  if (!weights)  // all ones: every job takes every row, which the host can see
    for (int j = 0; j < n_jobs; ++j)
      if (jobs[j].n_rows != n_rows) return VAD_EINVAL;
  // a row weighs at most 255: a job of more rows than this cannot stay within the limit
  for (int j = 0; weights && j < n_jobs; ++j)
    if (jobs[j].n_rows > VAD_TREE_TRAIN_MAX_WEIGHT) return VAD_EINVAL;
  const size_t need = tree_train_ws_bytes(n_rows, n_features, n_jobs, jobs, true);
  if (need == 0) return VAD_EUNSUPPORTED;
  if (workspace_bytes < need) return VAD_EINVAL;
  // weights of all ones are the unweighted rule: the unweighted kernels run
  return tree_train_run(x, y, n_rows, n_features, n_classes, order, weights, feature_masks, n_jobs, jobs, t, workspace,
                        workspace_bytes, n_levels, (hipStream_t)stream, weights != nullptr);
}

size_t vad_mfcc_ffn_workspace_bytes(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, int64_t n_samples,
                                    int32_t frame_size, int32_t hop) {
  if (!plan || !ffn) return 0;
  const int64_t f = vad_n_frames(n_samples, frame_size, hop);
  return (size_t)f * plan->host.mfcc_n * sizeof(float);
}

int32_t vad_mfcc_ffn_fusable(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, int32_t frame_size, int32_t hop) {
  if (!plan || !ffn) return 0;
  return mfcc_ffn_fusable(plan->spec, ffn->net, frame_size, hop, nullptr, 4) ? 1 : 0;
}

// Shared body of vad_mfcc_ffn / vad_mfcc_ffn_i16: with a workspace, the MFCC
// kernel writes the rows there and the window kernel classifies them (the
// faster form on gfx950); without one, the fused kernel keeps
// them on chip.
static int mfcc_ffn_entry(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, const void* audio, int tin_bytes,
                          int64_t n_samples, int32_t frame_size, int32_t hop, int32_t mode, uint8_t* labels,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (!plan || !ffn || n_samples < 0 || frame_size <= 0 || hop <= 0 || (mode != 0 && mode != 1))
    return VAD_EINVAL;
  const int64_t f = vad_n_frames(n_samples, frame_size, hop);
  if (f <= 5) return VAD_OK;
  if (!audio || !labels) return VAD_EINVAL;
  if (ffn->net.dims[0] > 3 * plan->host.mfcc_n) return VAD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (!workspace) {
    if (plan->generic()) return VAD_EUNSUPPORTED;  // the fused kernel is the fft_n = 512 pipeline
    if (!mfcc_ffn_fusable(plan->spec, ffn->net, frame_size, hop, audio, tin_bytes)) return VAD_EINVAL;
    return (int)launch_mfcc_ffn(plan->dev, ffn->net, audio, tin_bytes, f, mode, labels, st);
  }
  const size_t need = (size_t)f * plan->host.mfcc_n * sizeof(float);
  if (workspace_bytes < need) return VAD_EINVAL;
  float* mf = (float*)workspace;
  if (plan->generic() && tin_bytes == 2)
    VAD_TRY(launch_generic_i16(0, plan->dev, (const int16_t*)audio, hop, frame_size, f, plan->fft_n, plan->tw_gen,
                               mf, st));
  else if (plan->generic())
    VAD_TRY(launch_generic(0, plan->dev, (const float*)audio, hop, frame_size, f, plan->fft_n, plan->tw_gen, mf,
                           st));
  else if (tin_bytes == 2)
    VAD_TRY(launch_mfcc_i16(0, plan->dev, launch_spec(plan), (const int16_t*)audio, hop, frame_size, f, mf, st,
                            balance_for_launch(plan->bal)));
  else
    VAD_TRY(launch_mfcc(0, plan->dev, launch_spec(plan), (const float*)audio, hop, frame_size, f, mf, st,
                        balance_for_launch(plan->bal)));
  return (int)launch_ffn(ffn->net, 0, mf, f - 5, plan->host.mfcc_n, mode, labels, st);
}

int vad_mfcc_ffn(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, const float* audio,
                 int64_t n_samples, int32_t frame_size, int32_t hop, int32_t mode,
                 uint8_t* labels, void* workspace, size_t workspace_bytes, void* stream) {
  return mfcc_ffn_entry(plan, ffn, audio, 4, n_samples, frame_size, hop, mode, labels, workspace,
                        workspace_bytes, stream);
}

int vad_mfcc_ffn_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, const int16_t* audio,
                     int64_t n_samples, int32_t frame_size, int32_t hop, int32_t mode,
                     uint8_t* labels, void* workspace, size_t workspace_bytes, void* stream) {
  return mfcc_ffn_entry(plan, ffn, audio, 2, n_samples, frame_size, hop, mode, labels, workspace,
                        workspace_bytes, stream);
}

int64_t vad_stream_ring_floats(int64_t n_streams, int32_t mfcc_n) {
  return n_streams * 5 * (int64_t)mfcc_n;
}

// The streaming entries take the hop samples as fp32 or as int16 PCM
// (hop_bytes 4 / 2, strides in elements either way): one body each, the same
// checks in the same order before any HIP call.
static int stream_push_entry(float* frames, int64_t frame_stride, int32_t frame_len, const void* hop,
                             int hop_bytes, int64_t hop_stride, int32_t hop_len, int64_t n_streams,
                             void* stream) {
  if (n_streams < 0 || frame_len <= 0 || frame_len > 1024 || hop_len <= 0 || hop_len > frame_len ||
      frame_stride < frame_len || hop_stride < hop_len)
    return VAD_EINVAL;
  if (n_streams == 0) return VAD_OK;
  if (!frames || !hop) return VAD_EINVAL;
  return (int)launch_stream_push(frames, frame_stride, frame_len, hop, hop_bytes, hop_stride, hop_len, n_streams,
                                 (hipStream_t)stream);
}

int vad_stream_push_hop(float* frames, int64_t frame_stride, int32_t frame_len, const float* hop,
                        int64_t hop_stride, int32_t hop_len, int64_t n_streams, void* stream) {
  return stream_push_entry(frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len, n_streams, stream);
}

int vad_stream_push_hop_i16(float* frames, int64_t frame_stride, int32_t frame_len, const int16_t* hop,
                            int64_t hop_stride, int32_t hop_len, int64_t n_streams, void* stream) {
  return stream_push_entry(frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len, n_streams, stream);
}

static int stream_hops_entry(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames,
                             int64_t frame_stride, int32_t frame_len, const void* hop, int hop_bytes,
                             int64_t hop_stride, int32_t hop_len, int64_t n_streams, int32_t n_hops,
                             int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels,
                             int64_t label_block_stride, void* stream, bool scored = false, int32_t active = 0,
                             float* scores = nullptr, int64_t score_block_stride = 0) {
  if (!plan || !ffn || n_streams < 0 || n_hops < 0 || frame_len <= 0 || frame_len > 1024 || hop_len <= 0 ||
      hop_len > frame_len || frame_stride < frame_len || hop_stride < hop_len)
    return VAD_EINVAL;
  if (n_hops > 1 && label_block_stride < n_streams) return VAD_EINVAL;  // label rows of two hops would overlap
  if (scored && (active < 0 || active >= ffn->net.n_classes)) return VAD_EINVAL;
  if (scored && n_hops > 1 && score_block_stride < n_streams) return VAD_EINVAL;  // score rows likewise
  // hop k's block must not be hop k-1's (a zero or negative stride would
  // replay, or walk backwards over, the new samples), and no two (hop,
  // stream) rows may overlap: either ordering of a disjoint layout is fine,
  // hop-major (blocks of S rows) or stream-major ((S, K*hop) viewed as
  // (K, S, hop): block stride hop, row stride K*hop)
  if (n_hops > 1 && !vad_hop_layout_disjoint(n_streams, n_hops, hop_block_stride, hop_stride, hop_len))
    return VAD_EINVAL;
  if (n_streams == 0 || n_hops == 0) return VAD_OK;
  if (!frames || !hop || !ring || !count || !labels || (scored && !scores)) return VAD_EINVAL;
  if (ffn->net.dims[0] > 3 * plan->host.mfcc_n) return VAD_EINVAL;
  if (plan->generic()) return VAD_EUNSUPPORTED;  // its FFT is the 256-point Stockham of fft_n = 512
  if (plan->spec == kSpecWindow) return VAD_EUNSUPPORTED;  // its table blob carries no analysis window
  if (scored)
    return (int)launch_stream_hop_scores(plan->hop_blob, plan->hop_blob_n, plan->host.n_filters, plan->n_taps,
                                         ffn->net, frames, frame_stride, frame_len, hop, hop_bytes, hop_stride,
                                         hop_len, n_streams, plan->host.mfcc_n, ring, count, labels, n_hops,
                                         hop_block_stride, label_block_stride, active, scores, score_block_stride,
                                         (hipStream_t)stream);
  return (int)launch_stream_hop(plan->hop_blob, plan->hop_blob_n, plan->host.n_filters, plan->n_taps, ffn->net,
                                frames, frame_stride, frame_len, hop, hop_bytes, hop_stride, hop_len, n_streams,
                                plan->host.mfcc_n, ring, count, labels, n_hops, hop_block_stride,
                                label_block_stride, (hipStream_t)stream);
}

int vad_stream_hops(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                    int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams,
                    int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels,
                    int64_t label_block_stride, void* stream) {
  return stream_hops_entry(plan, ffn, frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len, n_streams,
                           n_hops, hop_block_stride, ring, count, labels, label_block_stride, stream);
}

int vad_stream_hops_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                        int32_t frame_len, const int16_t* hop, int64_t hop_stride, int32_t hop_len,
                        int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count,
                        uint8_t* labels, int64_t label_block_stride, void* stream) {
  return stream_hops_entry(plan, ffn, frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len, n_streams,
                           n_hops, hop_block_stride, ring, count, labels, label_block_stride, stream);
}

// The scored forms: the label entries plus one fp32 score of class `active`
// per (hop, stream), scores[k * score_block_stride + s].
int vad_stream_hops_scores(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                           int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len,
                           int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count,
                           uint8_t* labels, int64_t label_block_stride, int32_t active, float* scores,
                           int64_t score_block_stride, void* stream) {
  return stream_hops_entry(plan, ffn, frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len, n_streams,
                           n_hops, hop_block_stride, ring, count, labels, label_block_stride, stream, true, active,
                           scores, score_block_stride);
}

int vad_stream_hops_scores_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames,
                               int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                               int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                               float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                               int32_t active, float* scores, int64_t score_block_stride, void* stream) {
  return stream_hops_entry(plan, ffn, frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len, n_streams,
                           n_hops, hop_block_stride, ring, count, labels, label_block_stride, stream, true, active,
                           scores, score_block_stride);
}

int vad_stream_hop(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                   int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams,
                   float* ring, int32_t* count, uint8_t* labels, void* stream) {
  return vad_stream_hops(plan, ffn, frames, frame_stride, frame_len, hop, hop_stride, hop_len, n_streams, 1, 0,
                         ring, count, labels, 0, stream);
}

int vad_stream_hop_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                       int32_t frame_len, const int16_t* hop, int64_t hop_stride, int32_t hop_len,
                       int64_t n_streams, float* ring, int32_t* count, uint8_t* labels, void* stream) {
  return vad_stream_hops_i16(plan, ffn, frames, frame_stride, frame_len, hop, hop_stride, hop_len, n_streams, 1, 0,
                             ring, count, labels, 0, stream);
}

int vad_stream_step(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, const float* frames,
                    int64_t frame_stride, int32_t frame_len, int64_t n_streams, float* ring,
                    int32_t* count, uint8_t* labels, float* mfcc_scratch, void* stream) {
  if (!plan || !ffn || n_streams < 0 || frame_len <= 0 || frame_stride < 0) return VAD_EINVAL;
  if (n_streams == 0) return VAD_OK;
  if (!frames || !ring || !count || !labels || !mfcc_scratch) return VAD_EINVAL;
  if (ffn->net.dims[0] > 3 * plan->host.mfcc_n) return VAD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (plan->generic())
    VAD_TRY(launch_generic(0, plan->dev, frames, frame_stride, frame_len, n_streams, plan->fft_n, plan->tw_gen,
                           mfcc_scratch, st));
  else
    VAD_TRY(launch_mfcc(0, plan->dev, launch_spec(plan), frames, frame_stride, frame_len, n_streams, mfcc_scratch, st));
  return (int)launch_stream_ffn(ffn->net, mfcc_scratch, ring, count, n_streams, plan->host.mfcc_n,
                                labels, st);
}

// The same entries with the decision tree (stream_tree_kernel.hip): the
// checks of stream_hops_entry in its order, the tree's feature count in place
// of the network's input width (a node's feature index is an offset into the
// wave's LDS row), and the walk selector.
int64_t vad_stream_tree_max_lds_nodes(const vad_mfcc_plan* plan) {
  if (!plan || !plan->hop_blob || plan->hop_blob_n <= 0) return -1;
  return stream_tree_max_lds_nodes(plan->hop_blob_n);
}

// The hop kernels' launch rule as a query: the launchers call the same
// functions (stream_hop_block_waves and the table sizes).
int64_t vad_stream_hop_table_bytes(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn) {
  if (!plan || !ffn || !plan->hop_blob || plan->hop_blob_n <= 0) return VAD_EINVAL;
  return (int64_t)stream_hop_ffn_table_bytes(plan->hop_blob_n, ffn->net);
}

int64_t vad_stream_hop_tree_table_bytes(const vad_mfcc_plan* plan, const vad_tree_plan* tree, int32_t walk) {
  if (!plan || !tree || !plan->hop_blob || plan->hop_blob_n <= 0) return VAD_EINVAL;
  if (walk != VAD_TREE_WALK_AUTO && walk != VAD_TREE_WALK_GLOBAL) return VAD_EINVAL;
  return (int64_t)stream_hop_tree_table_bytes(
      plan->hop_blob_n,
      stream_tree_lds_nodes(plan->hop_blob_n, tree->cnodes_dev, tree->n_nodes, walk == VAD_TREE_WALK_GLOBAL));
}

int32_t vad_stream_hop_block_waves(int64_t table_bytes, int64_t n_streams, int32_t n_hops) {
  if (table_bytes < 0 || n_streams < 0 || n_hops < 0) return VAD_EINVAL;
  if (n_streams == 0 || n_hops == 0) return 0;  // the entries return before any launch
  const int waves = stream_hop_block_waves((size_t)table_bytes, n_streams, n_hops);
  return waves > 0 ? waves : VAD_EINVAL;  // the launchers refuse tables that leave no wave its scratch
}

static int stream_hops_tree_entry(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                  int64_t frame_stride, int32_t frame_len, const void* hop, int hop_bytes,
                                  int64_t hop_stride, int32_t hop_len, int64_t n_streams, int32_t n_hops,
                                  int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels,
                                  int64_t label_block_stride, int32_t walk, void* stream, bool scored = false,
                                  int32_t active = 0, float* scores = nullptr, int64_t score_block_stride = 0) {
  if (!plan || !tree || n_streams < 0 || n_hops < 0 || frame_len <= 0 || frame_len > 1024 || hop_len <= 0 ||
      hop_len > frame_len || frame_stride < frame_len || hop_stride < hop_len)
    return VAD_EINVAL;
  if (walk != VAD_TREE_WALK_AUTO && walk != VAD_TREE_WALK_GLOBAL) return VAD_EINVAL;
  if (n_hops > 1 && label_block_stride < n_streams) return VAD_EINVAL;  // label rows of two hops would overlap
  if (scored && !tree->score_dev) return VAD_EINVAL;  // vad_tree_plan_set_scores first
  if (scored && (active < 0 || active >= tree->n_score_classes)) return VAD_EINVAL;
  if (scored && n_hops > 1 && score_block_stride < n_streams) return VAD_EINVAL;
  if (n_hops > 1 && !vad_hop_layout_disjoint(n_streams, n_hops, hop_block_stride, hop_stride, hop_len))
    return VAD_EINVAL;
  if (n_streams == 0 || n_hops == 0) return VAD_OK;
  if (!frames || !hop || !ring || !count || !labels || (scored && !scores)) return VAD_EINVAL;
  if (tree->n_features > 3 * plan->host.mfcc_n) return VAD_EINVAL;
  if (plan->generic()) return VAD_EUNSUPPORTED;  // its FFT is the 256-point Stockham of fft_n = 512
  if (plan->spec == kSpecWindow) return VAD_EUNSUPPORTED;  // its table blob carries no analysis window
  if (scored)
    return (int)launch_stream_hop_tree_scores(
        plan->hop_blob, plan->hop_blob_n, plan->host.n_filters, plan->n_taps, tree->cnodes_dev, tree->nodes_dev,
        tree->n_nodes, walk == VAD_TREE_WALK_GLOBAL, frames, frame_stride, frame_len, hop, hop_bytes, hop_stride,
        hop_len, n_streams, plan->host.mfcc_n, ring, count, labels, n_hops, hop_block_stride, label_block_stride,
        tree->score_dev + (size_t)active * (size_t)tree->n_nodes, scores, score_block_stride, (hipStream_t)stream);
  return (int)launch_stream_hop_tree(plan->hop_blob, plan->hop_blob_n, plan->host.n_filters, plan->n_taps,
                                     tree->cnodes_dev, tree->nodes_dev, tree->n_nodes, walk == VAD_TREE_WALK_GLOBAL,
                                     frames, frame_stride, frame_len, hop, hop_bytes, hop_stride, hop_len, n_streams,
                                     plan->host.mfcc_n, ring, count, labels, n_hops, hop_block_stride,
                                     label_block_stride, (hipStream_t)stream);
}

int vad_stream_hops_tree(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames, int64_t frame_stride,
                         int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams,
                         int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels,
                         int64_t label_block_stride, int32_t walk, void* stream) {
  return stream_hops_tree_entry(plan, tree, frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len, n_streams,
                                n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk, stream);
}

int vad_stream_hops_tree_i16(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                             int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                             int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring,
                             int32_t* count, uint8_t* labels, int64_t label_block_stride, int32_t walk, void* stream) {
  return stream_hops_tree_entry(plan, tree, frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len, n_streams,
                                n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk, stream);
}

int vad_stream_hops_tree_scores(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                int64_t frame_stride, int32_t frame_len, const float* hop, int64_t hop_stride,
                                int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride, int32_t walk,
                                int32_t active, float* scores, int64_t score_block_stride, void* stream) {
  return stream_hops_tree_entry(plan, tree, frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len, n_streams,
                                n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk, stream, true,
                                active, scores, score_block_stride);
}

int vad_stream_hops_tree_scores_i16(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                    int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                                    int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                    float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                    int32_t walk, int32_t active, float* scores, int64_t score_block_stride,
                                    void* stream) {
  return stream_hops_tree_entry(plan, tree, frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len, n_streams,
                                n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk, stream, true,
                                active, scores, score_block_stride);
}

int vad_stream_step_tree(const vad_mfcc_plan* plan, const vad_tree_plan* tree, const float* frames,
                         int64_t frame_stride, int32_t frame_len, int64_t n_streams, float* ring, int32_t* count,
                         uint8_t* labels, float* mfcc_scratch, void* stream) {
  if (!plan || !tree || n_streams < 0 || frame_len <= 0 || frame_stride < 0) return VAD_EINVAL;
  if (n_streams == 0) return VAD_OK;
  if (!frames || !ring || !count || !labels || !mfcc_scratch) return VAD_EINVAL;
  if (tree->n_features > 3 * plan->host.mfcc_n) return VAD_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (plan->generic())
    VAD_TRY(launch_generic(0, plan->dev, frames, frame_stride, frame_len, n_streams, plan->fft_n, plan->tw_gen,
                           mfcc_scratch, st));
  else
    VAD_TRY(launch_mfcc(0, plan->dev, launch_spec(plan), frames, frame_stride, frame_len, n_streams, mfcc_scratch, st));
  return (int)launch_stream_tree_ring(tree->cnodes_dev, tree->n_nodes, mfcc_scratch, ring, count, n_streams,
                                      plan->host.mfcc_n, labels, st);
}

// ---------------------------------------------------------------------------
// Live spectral noise subtraction in the hop kernels (stream_denoise.h)
// ---------------------------------------------------------------------------
int64_t vad_stream_spec_ring_floats(int64_t n_streams) { return n_streams * 5 * (int64_t)kBins; }
int64_t vad_stream_noise_rows_floats(int64_t n_streams) { return n_streams * kNoiseRows * (int64_t)kBins; }
int64_t vad_stream_noise_est_floats(int64_t n_streams) { return n_streams * (int64_t)kBins; }

// the state arrays of n_streams streams (the load entry has no spectrum
// ring): none null, no two overlapping
static bool denoise_state_ok(int64_t n_streams, bool with_spec, const float* spec_ring, const float* noise_rows,
                             const int32_t* noise_count, const float* noise_est) {
  if ((with_spec && !spec_ring) || !noise_rows || !noise_count || !noise_est) return false;
  struct Span { uintptr_t lo, hi; };
  const Span a[4] = {
      {(uintptr_t)spec_ring, (uintptr_t)spec_ring + (size_t)vad_stream_spec_ring_floats(n_streams) * sizeof(float)},
      {(uintptr_t)noise_rows, (uintptr_t)noise_rows + (size_t)vad_stream_noise_rows_floats(n_streams) * sizeof(float)},
      {(uintptr_t)noise_est, (uintptr_t)noise_est + (size_t)vad_stream_noise_est_floats(n_streams) * sizeof(float)},
      {(uintptr_t)noise_count, (uintptr_t)noise_count + (size_t)n_streams * sizeof(int32_t)}};
  for (int i = with_spec ? 0 : 1; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (a[i].lo < a[j].hi && a[j].lo < a[i].hi) return false;
  return true;
}

static bool denoise_alpha_ok(float alpha) { return alpha >= 0.f && alpha < 1.f; }  // false for NaN

// The checks of the scored entries in their order (scores may be null here:
// `active` and the score stride are read only with scores), then the denoise
// arguments; all before any device call.
static int stream_hops_denoise_entry(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, const vad_tree_plan* tree,
                                     float* frames, int64_t frame_stride, int32_t frame_len, const void* hop,
                                     int hop_bytes, int64_t hop_stride, int32_t hop_len, int64_t n_streams,
                                     int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count,
                                     uint8_t* labels, int64_t label_block_stride, int32_t walk, int32_t active,
                                     float* scores, int64_t score_block_stride, float* spec_ring, float* noise_rows,
                                     int32_t* noise_count, float* noise_est, float alpha, int32_t noise_class,
                                     int32_t update, void* stream, bool sessions = false,
                                     const int32_t* hop_counts = nullptr, uint8_t* restart = nullptr) {
  if (!plan || (!ffn && !tree) || n_streams < 0 || n_hops < 0 || frame_len <= 0 || frame_len > 1024 || hop_len <= 0 ||
      hop_len > frame_len || frame_stride < frame_len || hop_stride < hop_len)
    return VAD_EINVAL;
  if (tree && walk != VAD_TREE_WALK_AUTO && walk != VAD_TREE_WALK_GLOBAL) return VAD_EINVAL;
  if (n_hops > 1 && label_block_stride < n_streams) return VAD_EINVAL;
  if (scores && n_hops > 1 && score_block_stride < n_streams) return VAD_EINVAL;
  if (n_hops > 1 && !vad_hop_layout_disjoint(n_streams, n_hops, hop_block_stride, hop_stride, hop_len))
    return VAD_EINVAL;
  // the sessions entries run without denoising when all four state arrays are null (alpha, noise_class and
  // update are then not read); a partly set state is refused like any null array
  const bool denoise = !sessions || spec_ring || noise_rows || noise_count || noise_est;
  if (denoise) {
    if (!denoise_alpha_ok(alpha) || (update != 0 && update != 1) || noise_class < 0) return VAD_EINVAL;
    if (!denoise_state_ok(n_streams, true, spec_ring, noise_rows, noise_count, noise_est)) return VAD_EINVAL;
  }
  if (sessions && (!hop_counts || !restart)) return VAD_EINVAL;
  // from here on the plans are read
  if (scores) {
    if (tree && !tree->score_dev) return VAD_EINVAL;  // vad_tree_plan_set_scores first
    if (active < 0 || active >= (tree ? tree->n_score_classes : ffn->net.n_classes)) return VAD_EINVAL;
  }
  if (denoise && noise_class >= (tree ? tree->n_classes : ffn->net.n_classes)) return VAD_EINVAL;
  if (n_streams == 0 || n_hops == 0) return VAD_OK;
  if (!frames || !hop || !ring || !count || !labels) return VAD_EINVAL;
  if ((tree ? tree->n_features : ffn->net.dims[0]) > 3 * plan->host.mfcc_n) return VAD_EINVAL;
  if (plan->generic()) return VAD_EUNSUPPORTED;  // its FFT is the 256-point Stockham of fft_n = 512
  if (plan->spec == kSpecWindow) return VAD_EUNSUPPORTED;  // its table blob carries no analysis window
  const HopDenoise dn = {spec_ring, noise_rows, noise_count, noise_est, alpha, noise_class, update};
  if (sessions && tree)
    return (int)launch_stream_hop_tree_sessions(
        plan->hop_blob, plan->hop_blob_n, plan->host.n_filters, plan->n_taps, tree->cnodes_dev, tree->nodes_dev,
        tree->n_nodes, walk == VAD_TREE_WALK_GLOBAL, frames, frame_stride, frame_len, hop, hop_bytes, hop_stride,
        hop_len, n_streams, plan->host.mfcc_n, ring, count, labels, n_hops, hop_block_stride, label_block_stride,
        scores ? tree->score_dev + (size_t)active * (size_t)tree->n_nodes : nullptr, scores, score_block_stride,
        denoise ? &dn : nullptr, hop_counts, restart, (hipStream_t)stream);
  if (sessions)
    return (int)launch_stream_hop_sessions(plan->hop_blob, plan->hop_blob_n, plan->host.n_filters, plan->n_taps,
                                           ffn->net, frames, frame_stride, frame_len, hop, hop_bytes, hop_stride,
                                           hop_len, n_streams, plan->host.mfcc_n, ring, count, labels, n_hops,
                                           hop_block_stride, label_block_stride, active, scores, score_block_stride,
                                           denoise ? &dn : nullptr, hop_counts, restart, (hipStream_t)stream);
  if (tree)
    return (int)launch_stream_hop_tree_denoise(
        plan->hop_blob, plan->hop_blob_n, plan->host.n_filters, plan->n_taps, tree->cnodes_dev, tree->nodes_dev,
        tree->n_nodes, walk == VAD_TREE_WALK_GLOBAL, frames, frame_stride, frame_len, hop, hop_bytes, hop_stride,
        hop_len, n_streams, plan->host.mfcc_n, ring, count, labels, n_hops, hop_block_stride, label_block_stride,
        scores ? tree->score_dev + (size_t)active * (size_t)tree->n_nodes : nullptr, scores, score_block_stride, dn,
        (hipStream_t)stream);
  return (int)launch_stream_hop_denoise(plan->hop_blob, plan->hop_blob_n, plan->host.n_filters, plan->n_taps, ffn->net,
                                        frames, frame_stride, frame_len, hop, hop_bytes, hop_stride, hop_len,
                                        n_streams, plan->host.mfcc_n, ring, count, labels, n_hops, hop_block_stride,
                                        label_block_stride, active, scores, score_block_stride, dn,
                                        (hipStream_t)stream);
}

int vad_stream_hops_denoise(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                            int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len,
                            int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count,
                            uint8_t* labels, int64_t label_block_stride, int32_t active, float* scores,
                            int64_t score_block_stride, float* spec_ring, float* noise_rows, int32_t* noise_count,
                            float* noise_est, float alpha, int32_t noise_class, int32_t update, void* stream) {
  if (!ffn) return VAD_EINVAL;
  return stream_hops_denoise_entry(plan, ffn, nullptr, frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len,
                                   n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, 0,
                                   active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                   alpha, noise_class, update, stream);
}

int vad_stream_hops_denoise_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames,
                                int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                                int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                int32_t active, float* scores, int64_t score_block_stride, float* spec_ring,
                                float* noise_rows, int32_t* noise_count, float* noise_est, float alpha,
                                int32_t noise_class, int32_t update, void* stream) {
  if (!ffn) return VAD_EINVAL;
  return stream_hops_denoise_entry(plan, ffn, nullptr, frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len,
                                   n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, 0,
                                   active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                   alpha, noise_class, update, stream);
}

int vad_stream_hops_tree_denoise(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                 int64_t frame_stride, int32_t frame_len, const float* hop, int64_t hop_stride,
                                 int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                 float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                 int32_t walk, int32_t active, float* scores, int64_t score_block_stride,
                                 float* spec_ring, float* noise_rows, int32_t* noise_count, float* noise_est,
                                 float alpha, int32_t noise_class, int32_t update, void* stream) {
  if (!tree) return VAD_EINVAL;
  return stream_hops_denoise_entry(plan, nullptr, tree, frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len,
                                   n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk,
                                   active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                   alpha, noise_class, update, stream);
}

int vad_stream_hops_tree_denoise_i16(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                     int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                                     int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                     float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                     int32_t walk, int32_t active, float* scores, int64_t score_block_stride,
                                     float* spec_ring, float* noise_rows, int32_t* noise_count, float* noise_est,
                                     float alpha, int32_t noise_class, int32_t update, void* stream) {
  if (!tree) return VAD_EINVAL;
  return stream_hops_denoise_entry(plan, nullptr, tree, frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len,
                                   n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk,
                                   active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                   alpha, noise_class, update, stream);
}

// The sessions entries: the denoising entries' arguments (the four state
// arrays all null for no denoising), then the per-stream hop counts and
// restart flags.
int vad_stream_hops_sessions(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
    int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams, int32_t n_hops,
    int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
    int32_t active, float* scores, int64_t score_block_stride, float* spec_ring, float* noise_rows,
    int32_t* noise_count, float* noise_est, float alpha, int32_t noise_class, int32_t update,
    const int32_t* hop_counts, uint8_t* restart, void* stream) {
  if (!ffn) return VAD_EINVAL;
  return stream_hops_denoise_entry(plan, ffn, nullptr, frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len,
                                   n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, 0,
                                   active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                   alpha, noise_class, update, stream, true, hop_counts, restart);
}

int vad_stream_hops_sessions_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames,
    int64_t frame_stride,
    int32_t frame_len, const int16_t* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams, int32_t n_hops,
    int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
    int32_t active, float* scores, int64_t score_block_stride, float* spec_ring, float* noise_rows,
    int32_t* noise_count, float* noise_est, float alpha, int32_t noise_class, int32_t update,
    const int32_t* hop_counts, uint8_t* restart, void* stream) {
  if (!ffn) return VAD_EINVAL;
  return stream_hops_denoise_entry(plan, ffn, nullptr, frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len,
                                   n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, 0,
                                   active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                   alpha, noise_class, update, stream, true, hop_counts, restart);
}

int vad_stream_hops_tree_sessions(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
    int64_t frame_stride,
    int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams, int32_t n_hops,
    int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride, int32_t walk,
    int32_t active, float* scores, int64_t score_block_stride, float* spec_ring, float* noise_rows,
    int32_t* noise_count, float* noise_est, float alpha, int32_t noise_class, int32_t update,
    const int32_t* hop_counts, uint8_t* restart, void* stream) {
  if (!tree) return VAD_EINVAL;
  return stream_hops_denoise_entry(plan, nullptr, tree, frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len,
                                   n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk,
                                   active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                   alpha, noise_class, update, stream, true, hop_counts, restart);
}

int vad_stream_hops_tree_sessions_i16(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
    int64_t frame_stride,
    int32_t frame_len, const int16_t* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams, int32_t n_hops,
    int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride, int32_t walk,
    int32_t active, float* scores, int64_t score_block_stride, float* spec_ring, float* noise_rows,
    int32_t* noise_count, float* noise_est, float alpha, int32_t noise_class, int32_t update,
    const int32_t* hop_counts, uint8_t* restart, void* stream) {
  if (!tree) return VAD_EINVAL;
  return stream_hops_denoise_entry(plan, nullptr, tree, frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len,
                                   n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk,
                                   active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                   alpha, noise_class, update, stream, true, hop_counts, restart);
}

// ---------------------------------------------------------------------------
// The hop kernels with a random forest (stream_forest_kernel.hip): the tree
// sessions entry's arguments with the forest in place of the tree plan.
// scores, the four denoise arrays (all or none) and hop_counts / restart (both
// or neither) may be null; which are set selects the kernel.
// ---------------------------------------------------------------------------
static HopForest hop_forest(const vad_mfcc_plan* plan, const vad_forest* f, int32_t walk, int32_t active) {
  const int lds_trees =
      stream_forest_lds_trees(plan->hop_blob_n, f->roots_host, f->n_trees, walk == VAD_TREE_WALK_GLOBAL);
  return HopForest{forest_dev(f), lds_trees, f->roots_host[lds_trees], f->max_tree, active};
}

int64_t vad_stream_hop_forest_table_bytes(const vad_mfcc_plan* plan, const vad_forest* forest, int32_t walk) {
  if (!plan || !forest || !plan->hop_blob || plan->hop_blob_n <= 0) return VAD_EINVAL;
  if (walk != VAD_TREE_WALK_AUTO && walk != VAD_TREE_WALK_GLOBAL) return VAD_EINVAL;
  return (int64_t)stream_hop_forest_table_bytes(plan->hop_blob_n, hop_forest(plan, forest, walk, 0).lds_nodes);
}

int32_t vad_stream_forest_lds_trees(const vad_mfcc_plan* plan, const vad_forest* forest) {
  if (!plan || !forest || !plan->hop_blob || plan->hop_blob_n <= 0) return VAD_EINVAL;
  return hop_forest(plan, forest, VAD_TREE_WALK_AUTO, 0).lds_trees;
}

static int stream_hops_forest_entry(const vad_mfcc_plan* plan, const vad_forest* forest, float* frames,
                                    int64_t frame_stride, int32_t frame_len, const void* hop, int hop_bytes,
                                    int64_t hop_stride, int32_t hop_len, int64_t n_streams, int32_t n_hops,
                                    int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels,
                                    int64_t label_block_stride, int32_t walk, int32_t active, float* scores,
                                    int64_t score_block_stride, float* spec_ring, float* noise_rows,
                                    int32_t* noise_count, float* noise_est, float alpha, int32_t noise_class,
                                    int32_t update, const int32_t* hop_counts, uint8_t* restart, void* stream) {
  if (!plan || !forest || n_streams < 0 || n_hops < 0 || frame_len <= 0 || frame_len > 1024 || hop_len <= 0 ||
      hop_len > frame_len || frame_stride < frame_len || hop_stride < hop_len)
    return VAD_EINVAL;
  if (walk != VAD_TREE_WALK_AUTO && walk != VAD_TREE_WALK_GLOBAL) return VAD_EINVAL;
  if (n_hops > 1 && label_block_stride < n_streams) return VAD_EINVAL;
  if (scores && n_hops > 1 && score_block_stride < n_streams) return VAD_EINVAL;
  if (n_hops > 1 && !vad_hop_layout_disjoint(n_streams, n_hops, hop_block_stride, hop_stride, hop_len))
    return VAD_EINVAL;
  const bool denoise = spec_ring || noise_rows || noise_count || noise_est;  // a partly set state is refused
  if (denoise) {
    if (!denoise_alpha_ok(alpha) || (update != 0 && update != 1) || noise_class < 0) return VAD_EINVAL;
    if (!denoise_state_ok(n_streams, true, spec_ring, noise_rows, noise_count, noise_est)) return VAD_EINVAL;
  }
  if ((hop_counts != nullptr) != (restart != nullptr)) return VAD_EINVAL;
  // the score is the average's class `active`, computed with or without `scores`
  if (active < 0) return VAD_EINVAL;
  // from here on the plan and the forest are read
  if (active >= forest->n_classes || (denoise && noise_class >= forest->n_classes)) return VAD_EINVAL;
  if (forest->n_features > 3 * plan->host.mfcc_n) return VAD_EINVAL;
  if (n_streams == 0 || n_hops == 0) return VAD_OK;
  if (!frames || !hop || !ring || !count || !labels) return VAD_EINVAL;
  if (plan->generic()) return VAD_EUNSUPPORTED;  // its FFT is the 256-point Stockham of fft_n = 512
  if (plan->spec == kSpecWindow) return VAD_EUNSUPPORTED;  // its table blob carries no analysis window
  const HopDenoise dn = {spec_ring, noise_rows, noise_count, noise_est, alpha, noise_class, update};
  return (int)launch_stream_hop_forest(plan->hop_blob, plan->hop_blob_n, plan->host.n_filters, plan->n_taps,
                                       hop_forest(plan, forest, walk, active), frames, frame_stride, frame_len, hop,
                                       hop_bytes, hop_stride, hop_len, n_streams, plan->host.mfcc_n, ring, count,
                                       labels, n_hops, hop_block_stride, label_block_stride, scores,
                                       score_block_stride, denoise ? &dn : nullptr, hop_counts, restart,
                                       (hipStream_t)stream);
}

int vad_stream_hops_forest(const vad_mfcc_plan* plan, const vad_forest* forest, float* frames, int64_t frame_stride,
    int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams, int32_t n_hops,
    int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride, int32_t walk,
    int32_t active, float* scores, int64_t score_block_stride, float* spec_ring, float* noise_rows,
    int32_t* noise_count, float* noise_est, float alpha, int32_t noise_class, int32_t update,
    const int32_t* hop_counts, uint8_t* restart, void* stream) {
  return stream_hops_forest_entry(plan, forest, frames, frame_stride, frame_len, hop, 4, hop_stride, hop_len,
                                  n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk,
                                  active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                  alpha, noise_class, update, hop_counts, restart, stream);
}

int vad_stream_hops_forest_i16(const vad_mfcc_plan* plan, const vad_forest* forest, float* frames,
    int64_t frame_stride,
    int32_t frame_len, const int16_t* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams, int32_t n_hops,
    int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride, int32_t walk,
    int32_t active, float* scores, int64_t score_block_stride, float* spec_ring, float* noise_rows,
    int32_t* noise_count, float* noise_est, float alpha, int32_t noise_class, int32_t update,
    const int32_t* hop_counts, uint8_t* restart, void* stream) {
  return stream_hops_forest_entry(plan, forest, frames, frame_stride, frame_len, hop, 2, hop_stride, hop_len,
                                  n_streams, n_hops, hop_block_stride, ring, count, labels, label_block_stride, walk,
                                  active, scores, score_block_stride, spec_ring, noise_rows, noise_count, noise_est,
                                  alpha, noise_class, update, hop_counts, restart, stream);
}

// n frames per stream, (S, n, frame_len) with the strides given in elements,
// become the noise rows 0..n-1, the count n and the estimate
static int stream_noise_load_entry(const vad_mfcc_plan* plan, const void* frames, int in_bytes, int64_t stream_stride,
                                   int64_t frame_stride, int32_t frame_len, int32_t n, int64_t n_streams,
                                   float* noise_rows, int32_t* noise_count, float* noise_est, float alpha,
                                   void* stream) {
  if (!plan || n_streams < 0 || frame_len <= 0 || frame_len > 1024 || n < 1 || n > kNoiseRows ||
      frame_stride < frame_len || stream_stride < (int64_t)(n - 1) * frame_stride + frame_len)
    return VAD_EINVAL;
  if (!denoise_alpha_ok(alpha)) return VAD_EINVAL;
  if (!denoise_state_ok(n_streams, false, nullptr, noise_rows, noise_count, noise_est)) return VAD_EINVAL;
  if (n_streams == 0) return VAD_OK;
  if (!frames) return VAD_EINVAL;
  if (plan->generic()) return VAD_EUNSUPPORTED;
  if (plan->spec == kSpecWindow) return VAD_EUNSUPPORTED;
  return (int)launch_stream_noise_load(plan->hop_blob, frames, in_bytes, stream_stride, frame_stride, frame_len, n,
                                       n_streams, noise_rows, noise_count, noise_est, alpha, (hipStream_t)stream);
}

int vad_stream_noise_load(const vad_mfcc_plan* plan, const float* frames, int64_t stream_stride, int64_t frame_stride,
                          int32_t frame_len, int32_t n, int64_t n_streams, float* noise_rows, int32_t* noise_count,
                          float* noise_est, float alpha, void* stream) {
  return stream_noise_load_entry(plan, frames, 4, stream_stride, frame_stride, frame_len, n, n_streams, noise_rows,
                                 noise_count, noise_est, alpha, stream);
}

int vad_stream_noise_load_i16(const vad_mfcc_plan* plan, const int16_t* frames, int64_t stream_stride,
                              int64_t frame_stride, int32_t frame_len, int32_t n, int64_t n_streams,
                              float* noise_rows, int32_t* noise_count, float* noise_est, float alpha, void* stream) {
  return stream_noise_load_entry(plan, frames, 2, stream_stride, frame_stride, frame_len, n, n_streams, noise_rows,
                                 noise_count, noise_est, alpha, stream);
}

// ---------------------------------------------------------------------------
// Streaming segments (stream_segments_kernel.hip)
// ---------------------------------------------------------------------------
constexpr int64_t kSegParamMax = (int64_t)1 << 29;  // max_gap, min_run: the flush row count stays an int32
constexpr int64_t kSegRingMax = (int64_t)1 << 30;   // history elements per stream: ring indices stay an int32

int64_t vad_stream_seg_delay(int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop) {
  if (max_gap < 0 || min_run < 0 || max_gap > kSegParamMax || min_run > kSegParamMax) return -1;
  if (frame_size <= 0 || hop <= 0 || hop > frame_size) return -1;
  return max_gap + (min_run > 1 ? min_run : 1) + (frame_size / hop - 1) + 1;
}

int64_t vad_stream_seg_flush_rows(int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop) {
  const int64_t d = vad_stream_seg_delay(max_gap, min_run, frame_size, hop);
  return d < 0 ? -1 : d + 2 + (frame_size + hop - 1) / hop;
}

// The operating-point forms (vad_stream_segments_op*): pad_before more windows
// of delay, pad_after none (stream_segments_kernel.hip's header).
static bool seg_pad_ok(int64_t pad_before, int64_t pad_after) {
  return pad_before >= 0 && pad_after >= 0 && pad_before <= kSegParamMax && pad_after <= kSegParamMax;
}

int64_t vad_stream_seg_delay_pad(int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                                 int64_t pad_before, int64_t pad_after) {
  const int64_t d = vad_stream_seg_delay(max_gap, min_run, frame_size, hop);
  return d < 0 || !seg_pad_ok(pad_before, pad_after) ? -1 : d + pad_before;
}

int64_t vad_stream_seg_flush_rows_pad(int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                                      int64_t pad_before, int64_t pad_after) {
  const int64_t d = vad_stream_seg_delay_pad(max_gap, min_run, frame_size, hop, pad_before, pad_after);
  return d < 0 ? -1 : d + 2 + (frame_size + hop - 1) / hop;
}

size_t vad_stream_seg_state_bytes(int64_t n_streams) {
  return n_streams > 0 ? (size_t)n_streams * kSegStreamStateBytes : 0;
}

// history elements one stream needs for blocks of n_hops hops (-1: bad arguments or past kSegRingMax)
static int64_t seg_ring_need(int64_t n_hops, int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                             int64_t pad_before = 0, int64_t pad_after = 0) {
  const int64_t d = vad_stream_seg_delay_pad(max_gap, min_run, frame_size, hop, pad_before, pad_after);
  if (d < 0 || n_hops < 0) return -1;
  const int64_t need = (d + 3 + n_hops) * hop + frame_size;
  return need > kSegRingMax ? -1 : need;
}

int64_t vad_stream_seg_history_elems(int64_t n_streams, int32_t n_hops_max, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop) {
  const int64_t need = seg_ring_need(n_hops_max, max_gap, min_run, frame_size, hop);
  if (need < 0 || n_streams < 0 || n_streams > INT32_MAX) return -1;
  return n_streams * need;
}

int64_t vad_stream_seg_history_elems_pad(int64_t n_streams, int32_t n_hops_max, int64_t max_gap, int64_t min_run,
                                         int32_t frame_size, int32_t hop, int64_t pad_before, int64_t pad_after) {
  const int64_t need = seg_ring_need(n_hops_max, max_gap, min_run, frame_size, hop, pad_before, pad_after);
  if (need < 0 || n_streams < 0 || n_streams > INT32_MAX) return -1;
  return n_streams * need;
}

// The operating point of the _op entries; null for the label entries.
struct SegOpHost {
  int32_t block_is_scores;
  float on, off;
  int64_t pad_before, pad_after;
};

// The sessions entries' five pointers (vad_stream_segments_sessions*); null
// for every other entry.
struct SegSessHost {
  const int32_t* hop_counts;
  uint8_t* restart;
  void* end_voiced;
  int32_t* end_len;
  int32_t* table_session;
};

// One body for the six entries: labels == NULL with flush set is a flush of
// vad_stream_seg_flush_rows hops; audio_bytes 0 is the events-only form.
// Every check comes before any HIP call, in the same order for every form.
static int stream_segments_entry(bool flush, const uint8_t* labels, int64_t label_block_stride, int64_t n_streams,
                                 int64_t n_hops, int32_t active, int64_t max_gap, int64_t min_run,
                                 int32_t frame_size, int32_t hop, void* state, int64_t* segments, int64_t capacity,
                                 int64_t* found, int audio_bytes, const void* hop_samples, int64_t hop_stride,
                                 int64_t hop_block_stride, void* history, int64_t history_elems, void* voiced,
                                 int32_t* voiced_len, void* stream, const SegOpHost* op = nullptr,
                                 const SegSessHost* sess = nullptr) {
  const int64_t delay = op ? vad_stream_seg_delay_pad(max_gap, min_run, frame_size, hop, op->pad_before, op->pad_after)
                           : vad_stream_seg_delay(max_gap, min_run, frame_size, hop);
  if (delay < 0) return VAD_EINVAL;  // hop outside (0, frame_size], a negative gap, run or pad
  if (op) {
    if (op->block_is_scores != 0 && op->block_is_scores != 1) return VAD_EINVAL;
    if (!(op->off >= 0.f && op->off <= op->on && op->on <= 1.f)) return VAD_EINVAL;  // NaN fails too
  }
  if (n_streams < 0 || n_streams > INT32_MAX || n_hops < 0 || n_hops > INT32_MAX || capacity < 0)
    return VAD_EINVAL;
  if (active < 0 || active >= 255) return VAD_EINVAL;  // 255 is "no label yet"
  if (!flush && n_hops > 1 && label_block_stride < n_streams) return VAD_EINVAL;
  if (audio_bytes && !flush) {
    if (hop_stride < hop) return VAD_EINVAL;
    if (n_hops > 1 && !vad_hop_layout_disjoint(n_streams, (int32_t)n_hops, hop_block_stride, hop_stride, hop))
      return VAD_EINVAL;
  }
  if (audio_bytes && history_elems < 0) return VAD_EINVAL;
  if (n_streams == 0 || n_hops == 0) return VAD_OK;
  if ((!flush && !labels) || !state || !found || (capacity > 0 && !segments)) return VAD_EINVAL;
  if (capacity > INT64_MAX / 2 / n_streams) return VAD_EINVAL;
  if (reinterpret_cast<uintptr_t>(state) % 8 || reinterpret_cast<uintptr_t>(segments) % 8 ||
      reinterpret_cast<uintptr_t>(found) % 8)
    return VAD_EINVAL;
  if (sess) {
    if (!sess->hop_counts || !sess->restart || !sess->end_len || (capacity > 0 && !sess->table_session))
      return VAD_EINVAL;
    if (audio_bytes && !sess->end_voiced) return VAD_EINVAL;
    if (reinterpret_cast<uintptr_t>(sess->hop_counts) % 4 || reinterpret_cast<uintptr_t>(sess->end_len) % 4 ||
        reinterpret_cast<uintptr_t>(sess->table_session) % 4 ||
        (audio_bytes && reinterpret_cast<uintptr_t>(sess->end_voiced) % audio_bytes))
      return VAD_EINVAL;
  }
  SegStreamArgs a{};
  if (audio_bytes) {
    if ((!flush && !hop_samples) || !history || !voiced || !voiced_len) return VAD_EINVAL;
    if (reinterpret_cast<uintptr_t>(hop_samples) % audio_bytes || reinterpret_cast<uintptr_t>(history) % audio_bytes ||
        reinterpret_cast<uintptr_t>(voiced) % audio_bytes || reinterpret_cast<uintptr_t>(voiced_len) % 4)
      return VAD_EINVAL;
    const int64_t need = seg_ring_need(flush ? 0 : n_hops, max_gap, min_run, frame_size, hop,
                                       op ? op->pad_before : 0, op ? op->pad_after : 0);
    const int64_t ring = history_elems / n_streams;
    if (need < 0 || ring < need || ring > kSegRingMax) return VAD_EINVAL;
    a.hop_samples = hop_samples, a.hstride = hop_stride, a.hop_kstride = hop_block_stride;
    a.history = history, a.ring = (int)ring, a.voiced = voiced, a.voiced_len = voiced_len;
  }
  a.labels = flush ? nullptr : labels, a.lab_kstride = label_block_stride;
  a.n_streams = n_streams, a.n_hops = (int)n_hops, a.active = active;
  a.max_gap = max_gap, a.min_run = min_run, a.join = frame_size / hop - 1, a.delay = delay;
  a.frame_size = frame_size, a.hop = hop;
  a.state = state, a.segments = segments, a.capacity = capacity, a.found = found;
  SegSessArgs ss{};
  if (sess) {  // the end of a session is that stream's flush: as many rows
    ss.hop_counts = sess->hop_counts, ss.restart = sess->restart, ss.end_voiced = sess->end_voiced;
    ss.end_len = sess->end_len, ss.table_session = sess->table_session;
    ss.flush_rows = (int)(delay + 2 + (frame_size + hop - 1) / hop);
  }
  if (op) {
    if (!flush && op->block_is_scores && reinterpret_cast<uintptr_t>(labels) % 4) return VAD_EINVAL;
    SegOpArgs o{};
    o.on = op->on, o.off = op->off, o.is_scores = op->block_is_scores;
    o.pad_before = op->pad_before, o.pad_after = op->pad_after;
    if (sess) return (int)launch_stream_segments_sessions(a, &o, ss, audio_bytes, (hipStream_t)stream);
    return (int)launch_stream_segments_op(a, o, audio_bytes, (hipStream_t)stream);
  }
  if (sess) return (int)launch_stream_segments_sessions(a, nullptr, ss, audio_bytes, (hipStream_t)stream);
  return (int)launch_stream_segments(a, audio_bytes, (hipStream_t)stream);
}

int vad_stream_segments(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams, int32_t n_hops,
                        int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                        void* state, int64_t* segments, int64_t capacity, int64_t* found, void* stream) {
  return stream_segments_entry(false, labels, label_block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 0, nullptr, 0, 0, nullptr, 0,
                               nullptr, nullptr, stream);
}

int vad_stream_segments_f32(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams, int32_t n_hops,
                            int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                            void* state, int64_t* segments, int64_t capacity, int64_t* found,
                            const float* hop_samples, int64_t hop_stride, int64_t hop_block_stride, float* history,
                            int64_t history_elems, float* voiced, int32_t* voiced_len, void* stream) {
  return stream_segments_entry(false, labels, label_block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 4, hop_samples, hop_stride,
                               hop_block_stride, history, history_elems, voiced, voiced_len, stream);
}

int vad_stream_segments_i16(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams, int32_t n_hops,
                            int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                            void* state, int64_t* segments, int64_t capacity, int64_t* found,
                            const int16_t* hop_samples, int64_t hop_stride, int64_t hop_block_stride,
                            int16_t* history, int64_t history_elems, int16_t* voiced, int32_t* voiced_len,
                            void* stream) {
  return stream_segments_entry(false, labels, label_block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 2, hop_samples, hop_stride,
                               hop_block_stride, history, history_elems, voiced, voiced_len, stream);
}

int vad_stream_segments_flush(int64_t n_streams, int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                              void* state, int64_t* segments, int64_t capacity, int64_t* found, void* stream) {
  return stream_segments_entry(true, nullptr, 0, n_streams, vad_stream_seg_flush_rows(max_gap, min_run, frame_size, hop),
                               1, max_gap, min_run, frame_size, hop, state, segments, capacity, found, 0, nullptr,
                               0, 0, nullptr, 0, nullptr, nullptr, stream);
}

int vad_stream_segments_flush_f32(int64_t n_streams, int64_t max_gap, int64_t min_run, int32_t frame_size,
                                  int32_t hop, void* state, int64_t* segments, int64_t capacity, int64_t* found,
                                  float* history, int64_t history_elems, float* voiced, int32_t* voiced_len,
                                  void* stream) {
  return stream_segments_entry(true, nullptr, 0, n_streams, vad_stream_seg_flush_rows(max_gap, min_run, frame_size, hop),
                               1, max_gap, min_run, frame_size, hop, state, segments, capacity, found, 4, nullptr,
                               0, 0, history, history_elems, voiced, voiced_len, stream);
}

int vad_stream_segments_flush_i16(int64_t n_streams, int64_t max_gap, int64_t min_run, int32_t frame_size,
                                  int32_t hop, void* state, int64_t* segments, int64_t capacity, int64_t* found,
                                  int16_t* history, int64_t history_elems, int16_t* voiced, int32_t* voiced_len,
                                  void* stream) {
  return stream_segments_entry(true, nullptr, 0, n_streams, vad_stream_seg_flush_rows(max_gap, min_run, frame_size, hop),
                               1, max_gap, min_run, frame_size, hop, state, segments, capacity, found, 2, nullptr,
                               0, 0, history, history_elems, voiced, voiced_len, stream);
}

// The operating-point forms: `block` holds fp32 scores (block_is_scores 1: the
// hysteresis on / off decides; `active` is not read) or uint8 labels (0), and
// a confirmed run is padded by pad_before / pad_after windows.
#define VAD_SEG_OP_HOST const SegOpHost oph{block_is_scores, on, off, pad_before, pad_after}

int vad_stream_segments_op(const void* block, int32_t block_is_scores, int64_t block_stride, int64_t n_streams,
                           int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size,
                           int32_t hop, float on, float off, int64_t pad_before, int64_t pad_after, void* state,
                           int64_t* segments, int64_t capacity, int64_t* found, void* stream) {
  VAD_SEG_OP_HOST;
  return stream_segments_entry(false, (const uint8_t*)block, block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 0, nullptr, 0, 0, nullptr, 0,
                               nullptr, nullptr, stream, &oph);
}

int vad_stream_segments_op_f32(const void* block, int32_t block_is_scores, int64_t block_stride, int64_t n_streams,
                               int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size,
                               int32_t hop, float on, float off, int64_t pad_before, int64_t pad_after, void* state,
                               int64_t* segments, int64_t capacity, int64_t* found, const float* hop_samples,
                               int64_t hop_stride, int64_t hop_block_stride, float* history, int64_t history_elems,
                               float* voiced, int32_t* voiced_len, void* stream) {
  VAD_SEG_OP_HOST;
  return stream_segments_entry(false, (const uint8_t*)block, block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 4, hop_samples, hop_stride,
                               hop_block_stride, history, history_elems, voiced, voiced_len, stream, &oph);
}

int vad_stream_segments_op_i16(const void* block, int32_t block_is_scores, int64_t block_stride, int64_t n_streams,
                               int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size,
                               int32_t hop, float on, float off, int64_t pad_before, int64_t pad_after, void* state,
                               int64_t* segments, int64_t capacity, int64_t* found, const int16_t* hop_samples,
                               int64_t hop_stride, int64_t hop_block_stride, int16_t* history, int64_t history_elems,
                               int16_t* voiced, int32_t* voiced_len, void* stream) {
  VAD_SEG_OP_HOST;
  return stream_segments_entry(false, (const uint8_t*)block, block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 2, hop_samples, hop_stride,
                               hop_block_stride, history, history_elems, voiced, voiced_len, stream, &oph);
}

// Flush: the thresholds are not read (every flush window is inactive), but
// they are checked like a push's, so one set of arguments serves both.
int vad_stream_segments_op_flush(int64_t n_streams, int32_t block_is_scores, int64_t max_gap, int64_t min_run,
                                 int32_t frame_size, int32_t hop, float on, float off, int64_t pad_before,
                                 int64_t pad_after, void* state, int64_t* segments, int64_t capacity, int64_t* found,
                                 void* stream) {
  VAD_SEG_OP_HOST;
  return stream_segments_entry(true, nullptr, 0, n_streams,
                               vad_stream_seg_flush_rows_pad(max_gap, min_run, frame_size, hop, pad_before, pad_after),
                               1, max_gap, min_run, frame_size, hop, state, segments, capacity, found, 0, nullptr, 0,
                               0, nullptr, 0, nullptr, nullptr, stream, &oph);
}

int vad_stream_segments_op_flush_f32(int64_t n_streams, int32_t block_is_scores, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop, float on, float off, int64_t pad_before,
                                     int64_t pad_after, void* state, int64_t* segments, int64_t capacity,
                                     int64_t* found, float* history, int64_t history_elems, float* voiced,
                                     int32_t* voiced_len, void* stream) {
  VAD_SEG_OP_HOST;
  return stream_segments_entry(true, nullptr, 0, n_streams,
                               vad_stream_seg_flush_rows_pad(max_gap, min_run, frame_size, hop, pad_before, pad_after),
                               1, max_gap, min_run, frame_size, hop, state, segments, capacity, found, 4, nullptr, 0,
                               0, history, history_elems, voiced, voiced_len, stream, &oph);
}

int vad_stream_segments_op_flush_i16(int64_t n_streams, int32_t block_is_scores, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop, float on, float off, int64_t pad_before,
                                     int64_t pad_after, void* state, int64_t* segments, int64_t capacity,
                                     int64_t* found, int16_t* history, int64_t history_elems, int16_t* voiced,
                                     int32_t* voiced_len, void* stream) {
  VAD_SEG_OP_HOST;
  return stream_segments_entry(true, nullptr, 0, n_streams,
                               vad_stream_seg_flush_rows_pad(max_gap, min_run, frame_size, hop, pad_before, pad_after),
                               1, max_gap, min_run, frame_size, hop, state, segments, capacity, found, 2, nullptr, 0,
                               0, history, history_elems, voiced, voiced_len, stream, &oph);
}

// The sessions forms of a push (include/vad_amd.h, "Sessions in the streaming
// segmenter"): the siblings' arguments and checks, plus the five pointers.
#define VAD_SEG_SESS_HOST(ev) const SegSessHost ssh{hop_counts, restart, ev, end_len, table_session}

int vad_stream_segments_sessions(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams,
                                 int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run,
                                 int32_t frame_size, int32_t hop, void* state, int64_t* segments, int64_t capacity,
                                 int64_t* found, const int32_t* hop_counts, uint8_t* restart, int32_t* end_len,
                                 int32_t* table_session, void* stream) {
  VAD_SEG_SESS_HOST(nullptr);
  return stream_segments_entry(false, labels, label_block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 0, nullptr, 0, 0, nullptr, 0,
                               nullptr, nullptr, stream, nullptr, &ssh);
}

int vad_stream_segments_sessions_f32(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams,
                                     int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop, void* state, int64_t* segments,
                                     int64_t capacity, int64_t* found, const float* hop_samples, int64_t hop_stride,
                                     int64_t hop_block_stride, float* history, int64_t history_elems, float* voiced,
                                     int32_t* voiced_len, const int32_t* hop_counts, uint8_t* restart,
                                     float* end_voiced, int32_t* end_len, int32_t* table_session, void* stream) {
  VAD_SEG_SESS_HOST(end_voiced);
  return stream_segments_entry(false, labels, label_block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 4, hop_samples, hop_stride,
                               hop_block_stride, history, history_elems, voiced, voiced_len, stream, nullptr, &ssh);
}

int vad_stream_segments_sessions_i16(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams,
                                     int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop, void* state, int64_t* segments,
                                     int64_t capacity, int64_t* found, const int16_t* hop_samples,
                                     int64_t hop_stride, int64_t hop_block_stride, int16_t* history,
                                     int64_t history_elems, int16_t* voiced, int32_t* voiced_len,
                                     const int32_t* hop_counts, uint8_t* restart, int16_t* end_voiced,
                                     int32_t* end_len, int32_t* table_session, void* stream) {
  VAD_SEG_SESS_HOST(end_voiced);
  return stream_segments_entry(false, labels, label_block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 2, hop_samples, hop_stride,
                               hop_block_stride, history, history_elems, voiced, voiced_len, stream, nullptr, &ssh);
}

int vad_stream_segments_op_sessions(const void* block, int32_t block_is_scores, int64_t block_stride,
                                    int64_t n_streams, int32_t n_hops, int32_t active, int64_t max_gap,
                                    int64_t min_run, int32_t frame_size, int32_t hop, float on, float off,
                                    int64_t pad_before, int64_t pad_after, void* state, int64_t* segments,
                                    int64_t capacity, int64_t* found, const int32_t* hop_counts, uint8_t* restart,
                                    int32_t* end_len, int32_t* table_session, void* stream) {
  VAD_SEG_OP_HOST;
  VAD_SEG_SESS_HOST(nullptr);
  return stream_segments_entry(false, (const uint8_t*)block, block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 0, nullptr, 0, 0, nullptr, 0,
                               nullptr, nullptr, stream, &oph, &ssh);
}

int vad_stream_segments_op_sessions_f32(const void* block, int32_t block_is_scores, int64_t block_stride,
                                        int64_t n_streams, int32_t n_hops, int32_t active, int64_t max_gap,
                                        int64_t min_run, int32_t frame_size, int32_t hop, float on, float off,
                                        int64_t pad_before, int64_t pad_after, void* state, int64_t* segments,
                                        int64_t capacity, int64_t* found, const float* hop_samples,
                                        int64_t hop_stride, int64_t hop_block_stride, float* history,
                                        int64_t history_elems, float* voiced, int32_t* voiced_len,
                                        const int32_t* hop_counts, uint8_t* restart, float* end_voiced,
                                        int32_t* end_len, int32_t* table_session, void* stream) {
  VAD_SEG_OP_HOST;
  VAD_SEG_SESS_HOST(end_voiced);
  return stream_segments_entry(false, (const uint8_t*)block, block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 4, hop_samples, hop_stride,
                               hop_block_stride, history, history_elems, voiced, voiced_len, stream, &oph, &ssh);
}

int vad_stream_segments_op_sessions_i16(const void* block, int32_t block_is_scores, int64_t block_stride,
                                        int64_t n_streams, int32_t n_hops, int32_t active, int64_t max_gap,
                                        int64_t min_run, int32_t frame_size, int32_t hop, float on, float off,
                                        int64_t pad_before, int64_t pad_after, void* state, int64_t* segments,
                                        int64_t capacity, int64_t* found, const int16_t* hop_samples,
                                        int64_t hop_stride, int64_t hop_block_stride, int16_t* history,
                                        int64_t history_elems, int16_t* voiced, int32_t* voiced_len,
                                        const int32_t* hop_counts, uint8_t* restart, int16_t* end_voiced,
                                        int32_t* end_len, int32_t* table_session, void* stream) {
  VAD_SEG_OP_HOST;
  VAD_SEG_SESS_HOST(end_voiced);
  return stream_segments_entry(false, (const uint8_t*)block, block_stride, n_streams, n_hops, active, max_gap, min_run,
                               frame_size, hop, state, segments, capacity, found, 2, hop_samples, hop_stride,
                               hop_block_stride, history, history_elems, voiced, voiced_len, stream, &oph, &ssh);
}
#undef VAD_SEG_SESS_HOST
#undef VAD_SEG_OP_HOST

// Replay of a captured graph (a hop block with its host copies,
// vad_amd.stream.StreamBatch.capture): hipGraphLaunch on the caller's stream.
int vad_graph_launch(void* graph_exec, void* stream) {
  if (!graph_exec) return VAD_EINVAL;
  return (int)hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream);
}

// A captured step prepared for replay.  A graph of exactly one kernel node
// (the one-hop step of StreamBatch, kernel="hop") is dispatched as that
// node: its captured function, grid, block, dynamic LDS and argument values
// (kernelParams point into the graph's own copy, so the graph must outlive
// the plan) go to hipLaunchKernel -- on ROCm 7.2 a hipGraphLaunch of one
// kernel node costs ~5 us more host time per call than the launch it wraps
// (profiles/r06/c5_graph/), so back-to-back one-hop replays were host-bound
// at ~15 us against ~10 us launched directly.  Any other graph replays
// through hipGraphLaunch.
struct vad_graph_plan {
  hipGraphExec_t exec;
  int32_t n_nodes;
  bool direct;
  hipKernelNodeParams kp;
};

int vad_graph_plan_create(void* graph, void* graph_exec, vad_graph_plan** out) {
  if (!graph || !graph_exec || !out) return VAD_EINVAL;
  *out = nullptr;
  size_t n = 0;
  hipError_t e = hipGraphGetNodes((hipGraph_t)graph, nullptr, &n);
  if (e != hipSuccess) return (int)e;
  vad_graph_plan* p = (vad_graph_plan*)calloc(1, sizeof(vad_graph_plan));
  if (!p) return VAD_ENOMEM;
  p->exec = (hipGraphExec_t)graph_exec;
  p->n_nodes = (int32_t)n;
  p->direct = false;
  if (n == 1) {
    hipGraphNode_t node;
    size_t one = 1;
    hipGraphNodeType ty;
    if (hipGraphGetNodes((hipGraph_t)graph, &node, &one) == hipSuccess && one == 1 &&
        hipGraphNodeGetType(node, &ty) == hipSuccess && ty == hipGraphNodeTypeKernel &&
        hipGraphKernelNodeGetParams(node, &p->kp) == hipSuccess && p->kp.func && p->kp.kernelParams &&
        !p->kp.extra)
      p->direct = true;
  }
  *out = p;
  return VAD_OK;
}

int vad_graph_plan_launch(const vad_graph_plan* p, void* stream) {
  if (!p) return VAD_EINVAL;
  if (p->direct)
    return (int)hipLaunchKernel(p->kp.func, p->kp.gridDim, p->kp.blockDim, p->kp.kernelParams,
                                p->kp.sharedMemBytes, (hipStream_t)stream);
  return (int)hipGraphLaunch(p->exec, (hipStream_t)stream);
}

int32_t vad_graph_plan_direct(const vad_graph_plan* p) { return p && p->direct ? 1 : 0; }

int vad_graph_plan_destroy(vad_graph_plan* p) {
  free(p);
  return VAD_OK;
}

}  // extern "C"
