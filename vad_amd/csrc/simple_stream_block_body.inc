// The body of simple_stream_block_kernel<T>(SimpleBlockArgs a) and, with
// VAD_SIMPLE_SESSIONS 1, of simple_stream_block_sessions_kernel<T>(a,
// SimpleSessions ss): included once per kernel (simple_stream_kernel.hip has
// the LDS layout and the barrier argument).  With VAD_SIMPLE_SESSIONS 0 it
// preprocesses to the text the plain kernel always had.
//
// The sessions form reads the stream's three words once, in every thread,
// before the first barrier, so they are uniform in the workgroup; thread 0
// stores the consumed flag after that barrier.  The frame count bounds the
// round loop, a restart replaces the load of the old record by zeros, and the
// stepping lane runs simple_state_init_step in place of simple_state_step
// while the stream still owes init frames.
  extern __shared__ __attribute__((aligned(16))) double ssm[];
  const int L = a.L, nb = a.nb, K = a.n_frames;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  double* twc = ssm;
  double* tws = ssm + (L >> 1);
  double* re = ssm + L + (size_t)wave * 2 * L;
  double* im = re + L;
  double* noise = ssm + L + (size_t)waves * 2 * L;
  double* rows = noise + kSimpleNoiseCols * nb;
  int* slot = reinterpret_cast<int*>(rows + 2 * waves * kFeatRow);
  const int64_t s = blockIdx.x;
  double* st = reinterpret_cast<double*>(static_cast<char*>(a.state) + s * simple_state_bytes(nb));
  const T* frames = static_cast<const T*>(a.frames) + s * a.stream_stride;
  T* voiced = a.voiced ? static_cast<T*>(a.voiced) + s * a.voiced_stride : nullptr;
#if VAD_SIMPLE_SESSIONS
  // the stream's session for this launch, wave-uniform (scalar): the frames it
  // takes from its column, whether it starts over first, the init frames it owes
  int n_s = __builtin_amdgcn_readfirstlane(ss.frame_counts[s]);
  n_s = n_s < 0 ? 0 : n_s > K ? K : n_s;
  const int restarted = __builtin_amdgcn_readfirstlane((int)ss.restart[s]);
  int left = restarted ? nb : __builtin_amdgcn_readfirstlane(ss.init_left[s]);
  left = left < 0 ? 0 : left > nb ? nb : left;  // whatever the word holds, the noise row stays inside
  for (int k = n_s + threadIdx.x; k < K; k += blockDim.x)  // the rows this stream has no frame in
    a.labels[(int64_t)k * a.lab_stride + s] = (uint8_t)VAD_LABEL_NO_HOP;
  if (n_s == 0 && !restarted) {  // stalled: no barrier yet, the record and init_left keep every byte
    if (threadIdx.x == 0 && a.voiced_len) a.voiced_len[s] = 0;
    return;
  }
#define VAD_SIMPLE_N n_s
#else
#define VAD_SIMPLE_N K
#endif
  int log2L = 0;
  while ((1 << log2L) < L) ++log2L;
#if VAD_SIMPLE_SESSIONS
  if (n_s > 0)  // a restart with no frame needs no table
#endif
  for (int j = threadIdx.x; j < (L >> 1); j += blockDim.x)
    sincospi(-2.0 * (double)j / (double)L, &tws[j], &twc[j]);
#if VAD_SIMPLE_SESSIONS
  for (int j = threadIdx.x; j < kSimpleNoiseCols * nb; j += blockDim.x) noise[j] = restarted ? 0.0 : st[j];
  SimpleState reg{};
  if (threadIdx.x == 0 && !restarted) simple_state_load(reg, st, nb);
#else
  for (int j = threadIdx.x; j < kSimpleNoiseCols * nb; j += blockDim.x) noise[j] = st[j];
  SimpleState reg{};
  if (threadIdx.x == 0) simple_state_load(reg, st, nb);
#endif
  int n_voiced = 0;
  __syncthreads();
#if VAD_SIMPLE_SESSIONS
  if (restarted && threadIdx.x == 0) ss.restart[s] = 0;  // every thread has read it: consumed once, also under replay
#endif
  const int rounds = (VAD_SIMPLE_N + waves - 1) / waves;
  for (int r = 0; r <= rounds; ++r) {
    const int k = r * waves + wave;
    if (r < rounds && k < VAD_SIMPLE_N) {
      double* o = rows + ((r & 1) * waves + wave) * kFeatRow;
      simple_wave_features(frames + k * a.block_stride, a.frame_len, L, log2L, a.pad, a.band_bins, 4, 1, twc, tws,
                           re, im, lane, o);
      if (a.features_out && lane == 0) {
        double* fo = a.features_out + ((int64_t)k * a.n_streams + s) * 7;
#pragma unroll
        for (int i = 0; i < 7; ++i) fo[i] = o[i];
      }
      wave_lds_sync();  // the next round overwrites re / im
    }
    __syncthreads();
    // the frames of round r - 1 that were labelled active, packed in order
    const int kp = k - waves;
    if (voiced && r > 0 && kp < VAD_SIMPLE_N) {
      const int at = slot[((r - 1) & 1) * waves + wave];
      if (at >= 0) {
        const T* x = frames + kp * a.block_stride;
        T* d = voiced + (int64_t)at * a.frame_len;
        for (int i = lane; i < a.frame_len; i += 64) d[i] = x[i];
      }
    }
    if (threadIdx.x == 0 && r < rounds) {
      for (int w = 0; w < waves && r * waves + w < VAD_SIMPLE_N; ++w) {
#if VAD_SIMPLE_SESSIONS
        int lab = VAD_LABEL_INIT;
        if (left > 0)  // an init frame: never voiced
          simple_state_init_step(reg, noise, nb, left, rows + ((r & 1) * waves + w) * kFeatRow);
        else
          lab = simple_state_step(reg, noise, nb, rows + ((r & 1) * waves + w) * kFeatRow);
        a.labels[(int64_t)(r * waves + w) * a.lab_stride + s] = (uint8_t)lab;
        slot[(r & 1) * waves + w] = lab == 1 ? n_voiced++ : -1;
#else
        const int lab = simple_state_step(reg, noise, nb, rows + ((r & 1) * waves + w) * kFeatRow);
        a.labels[(int64_t)(r * waves + w) * a.lab_stride + s] = (uint8_t)lab;
        slot[(r & 1) * waves + w] = lab ? n_voiced++ : -1;
#endif
      }
    }
  }
  // the last pass of the loop (r == rounds) was the barrier after the last steps
  for (int j = threadIdx.x; j < kSimpleNoiseCols * nb; j += blockDim.x) st[j] = noise[j];
  if (threadIdx.x == 0) {
    simple_state_store(reg, st, nb);
    if (a.voiced_len) a.voiced_len[s] = n_voiced * a.frame_len;
#if VAD_SIMPLE_SESSIONS
    ss.init_left[s] = left;
#endif
  }
#undef VAD_SIMPLE_N
