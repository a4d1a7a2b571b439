// The body of simple_stream_state_kernel and, with VAD_SIMPLE_SESSIONS 1, of
// simple_stream_state_sessions_kernel (the plain kernel's arguments, then
// SimpleSessions ss): one wave per stream, lane 0 stepping.  With
// VAD_SIMPLE_SESSIONS 0 it preprocesses to the text the plain kernel always
// had.  The sessions form reads the stream's three words in every lane of its
// wave before lane 0 stores any of them; the features launch before it has
// computed all n_frames rows of every stream, and rows 0..n_s-1 are stepped.
  const int lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (s >= n_streams) return;
  double* st = reinterpret_cast<double*>(static_cast<char*>(state) + s * simple_state_bytes(nb));
#if VAD_SIMPLE_SESSIONS
  int n_s = __builtin_amdgcn_readfirstlane(ss.frame_counts[s]);
  n_s = n_s < 0 ? 0 : n_s > n_frames ? n_frames : n_s;
  const int restarted = __builtin_amdgcn_readfirstlane((int)ss.restart[s]);
  int left = restarted ? nb : __builtin_amdgcn_readfirstlane(ss.init_left[s]);
  left = left < 0 ? 0 : left > nb ? nb : left;  // whatever the word holds, the noise row stays inside
  for (int k = n_s + lane; k < n_frames; k += 64)  // the rows this stream has no frame in
    labels[(int64_t)k * lab_stride + s] = (uint8_t)VAD_LABEL_NO_HOP;
  if (n_s == 0 && !restarted) {  // stalled: the record and init_left keep every byte
    if (lane == 0 && voiced_len) voiced_len[s] = 0;
    return;
  }
  SimpleState reg{};
  if (restarted) {  // a fresh record: the noise rows by the wave, the rest from reg below
    for (int j = lane; j < kSimpleNoiseCols * nb; j += 64) st[j] = 0.0;
    __threadfence_block();  // lane 0 reads and writes these rows
    if (lane == 0) ss.restart[s] = 0;
  } else if (lane == 0) {
    simple_state_load(reg, st, nb);
  }
#define VAD_SIMPLE_N n_s
#else
  SimpleState reg{};
  if (lane == 0) simple_state_load(reg, st, nb);
#define VAD_SIMPLE_N n_frames
#endif
  int n_voiced = 0;
  for (int k = 0; k < VAD_SIMPLE_N; ++k) {
    int lab = 0;
    if (lane == 0) {
      double f[7];
      const double* row = feats + ((int64_t)k * n_streams + s) * 7;
#pragma unroll
      for (int i = 0; i < 7; ++i) f[i] = row[i];
#if VAD_SIMPLE_SESSIONS
      lab = VAD_LABEL_INIT;
      if (left > 0)  // an init frame: never voiced
        simple_state_init_step(reg, st, nb, left, f);
      else
        lab = simple_state_step(reg, st, nb, f);
#else
      lab = simple_state_step(reg, st, nb, f);
#endif
      labels[(int64_t)k * lab_stride + s] = (uint8_t)lab;
    }
    if (voiced) {
      lab = __shfl(lab, 0);
#if VAD_SIMPLE_SESSIONS
      if (lab == 1) {
#else
      if (lab) {
#endif
        const float* x = frames + k * block_stride + s * stream_stride;
        float* d = voiced + s * voiced_stride + (int64_t)n_voiced * frame_len;
        for (int i = lane; i < frame_len; i += 64) d[i] = x[i];
        ++n_voiced;
      }
    }
  }
  if (lane == 0) {
    simple_state_store(reg, st, nb);
    if (voiced_len) voiced_len[s] = n_voiced * frame_len;
#if VAD_SIMPLE_SESSIONS
    ss.init_left[s] = left;
#endif
  }
#undef VAD_SIMPLE_N
