// The per-stream state machine of the energy / ZCR / spectral analyser
// (realtime_analysis/simple_analyzer.py:78-112, 144-164, 245-256), one step
// per feature row, for simple_stream_kernel.hip.  Both kernels there call
// simple_state_step, so a stream gives the same labels and state whichever
// way its rows were computed; their sessions forms call simple_state_init_step
// too, one definition of a joining stream's init for both paths.
//
// A stream's state in memory (include/vad_amd.h, vad_simple_stream_state_bytes):
//   double noise[noise_buf_len][6]   energy, std|fft|, band 0..3 of the noise frames
//   double thresh[6]                 energy, spectral std, band 0..3
//   int32  status, silence, noise_pointer, frame_number
// status: the 20-entry status buffer, bit 0 the newest entry.
//
// The host computes without FMA and one ulp of a threshold can flip a label:
// the functions that do the state's arithmetic switch contraction off and use
// the plain operators (#pragma clang fp contract(off); __dmul_rn / __dadd_rn
// are inline functions compiled under their own header's mode, and the
// compiler fuses their product and sum all the same).
#pragma once

#include "vad_common.h"

namespace vad {

constexpr int kSimpleNoiseCols = 6;
constexpr int kSimpleStatusBits = 20;    // TEMP_BUFFER_SIZE
constexpr int kSimpleActiveRun = 5;      // TEMP_ACTIVE_THRESHOLD
constexpr int kSimpleInactiveRun = 15;   // TEMP_INACTIVE_THRESHOLD
constexpr int kSimpleMaxNoise = VAD_SIMPLE_MAX_NOISE;

__host__ __device__ constexpr size_t simple_state_bytes(int nb) {
  return (size_t)(kSimpleNoiseCols * nb + 6) * sizeof(double) + 4 * sizeof(int32_t);
}

// The registers of one stream between steps (the noise rows stay in memory).
struct SimpleState {
  double e_th, std_th, b_th[4];
  uint32_t status;
  int silence, ptr, frame_no;
};

__device__ __forceinline__ void simple_state_load(SimpleState& s, const double* st, int nb) {
  const double* t = st + kSimpleNoiseCols * nb;
  s.e_th = t[0];
  s.std_th = t[1];
#pragma unroll
  for (int j = 0; j < 4; ++j) s.b_th[j] = t[2 + j];
  const int32_t* w = reinterpret_cast<const int32_t*>(t + 6);
  s.status = (uint32_t)w[0];
  s.silence = w[1];
  s.ptr = w[2];
  s.frame_no = w[3];
}

__device__ __forceinline__ void simple_state_store(const SimpleState& s, double* st, int nb) {
  double* t = st + kSimpleNoiseCols * nb;
  t[0] = s.e_th;
  t[1] = s.std_th;
#pragma unroll
  for (int j = 0; j < 4; ++j) t[2 + j] = s.b_th[j];
  int32_t* w = reinterpret_cast<int32_t*>(t + 6);
  w[0] = (int32_t)s.status;
  w[1] = s.silence;
  w[2] = s.ptr;
  w[3] = s.frame_no;
}

// np.uint32(energy) as the reference stores it (:309): truncated toward
// zero; saturated from 2^32 on, where numpy's cast is undefined.
__device__ __forceinline__ uint64_t simple_energy_u32(double e) {
  if (!(e >= 1.0)) return 0;
  if (e >= 4294967296.0) return 4294967295ull;
  return (uint64_t)e;
}

// The three means over the noise rows (:269-299, :362-384): the energies as
// integers (exact, any order), the std and the bands left to right in double.
__device__ __forceinline__ void simple_noise_means(const double* noise, int nb, double& em, double& sm,
                                                   double (&bm)[4]) {
#pragma clang fp contract(off)
  uint64_t es = simple_energy_u32(noise[0]);
  double ss = noise[1];
  double bs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bs[j] = noise[2 + j];
  for (int i = 1; i < nb; ++i) {
    const double* r = noise + kSimpleNoiseCols * i;
    es += simple_energy_u32(r[0]);
    ss = ss + r[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) bs[j] = bs[j] + r[2 + j];
  }
  const double n = (double)nb;
  em = (double)es / n;
  sm = ss / n;
#pragma unroll
  for (int j = 0; j < 4; ++j) bm[j] = bs[j] / n;
}

// _add_inactive_frame (:245-256): the row replaces the oldest noise entry,
// every threshold moves a quarter of the way to its new mean.
__device__ __forceinline__ void simple_add_inactive(SimpleState& s, double* noise, int nb, const double* f) {
#pragma clang fp contract(off)
  double* row = noise + kSimpleNoiseCols * s.ptr;
  row[0] = f[0];
  row[1] = f[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) row[2 + j] = f[3 + j];
  double em, sm, bm[4];
  simple_noise_means(noise, nb, em, sm, bm);
  s.e_th = 0.75 * s.e_th + 0.25 * em;
#pragma unroll
  for (int j = 0; j < 4; ++j) s.b_th[j] = 0.75 * s.b_th[j] + 0.25 * bm[j];
  s.std_th = 0.75 * s.std_th + 0.25 * sm;
  s.ptr = s.ptr == nb - 1 ? 0 : s.ptr + 1;
}

// feed_frame (:78-112) on the row f = [stEnergy, zcr * n, std|fft|, band 0..3]:
// 1 (active) or 0 (inactive).
__device__ __forceinline__ int simple_state_step(SimpleState& s, double* noise, int nb, const double* f) {
#pragma clang fp contract(off)
  s.frame_no += 1;
  const double k_band = 3.0, k_energy = 2.0, k_std = 2.0;
  const bool zcr = 20.0 >= f[1] && f[1] >= 5.0;
  bool spec = false;
  if (f[3] > s.b_th[0] * k_band) {
    int n = 0;
#pragma unroll
    for (int j = 1; j < 4; ++j) n += f[3 + j] > s.b_th[j] * k_band;
    spec = n >= 2;
  }
  const bool status = (spec && zcr) ||
                      (zcr && f[0] > k_energy * s.e_th && f[2] > s.std_th * k_std);
  s.status = ((s.status << 1) | (status ? 1u : 0u)) & ((1u << kSimpleStatusBits) - 1u);
  const int active = __popc(s.status);
  if (status) {
    if (s.silence && active >= kSimpleActiveRun) s.silence = 0;
    return 1;
  }
  if (s.silence) {
    simple_add_inactive(s, noise, nb, f);
    return 0;
  }
  if (kSimpleStatusBits - active >= kSimpleInactiveRun) {
    simple_add_inactive(s, noise, nb, f);
    s.silence = 1;
  }
  return 1;
}

// One init frame of a stream that initialises itself (the sessions kernels):
// load_init_inactive_frames (:120-138) a frame at a time.  The row fills noise
// row nb - init_left; the last one (init_left 1 -> 0) makes the thresholds the
// plain means and leaves what simple_stream_init_kernel leaves: status
// cleared, silence on, noise_pointer 0, frame_number 0.
__device__ __forceinline__ void simple_state_init_step(SimpleState& s, double* noise, int nb, int& init_left,
                                                       const double* f) {
#pragma clang fp contract(off)
  double* row = noise + kSimpleNoiseCols * (nb - init_left);
  row[0] = f[0];
  row[1] = f[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) row[2 + j] = f[3 + j];
  if (--init_left > 0) return;
  simple_noise_means(noise, nb, s.e_th, s.std_th, s.b_th);
  s.status = 0;
  s.silence = 1;
  s.ptr = 0;
  s.frame_no = 0;
}

}  // namespace vad
