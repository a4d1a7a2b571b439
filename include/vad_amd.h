/*
 * vad_amd.h -- C ABI of libvad_amd.so, the MI355X-native MFCC + FFN VAD path.
 *
 * The reference (nameofuser1/vad) is pure Python with no FFI, so there is no
 * existing binding to match byte for byte; each entry point below names the
 * reference function whose semantics it implements (file:line in the
 * reference tree) and the Python host layer (vad_amd/, ctypes) that mirrors
 * the reference API on top of it.
 *
 * Conventions
 *   - All data pointers are DEVICE pointers owned by the caller (torch tensors
 *     on the host side).  Plans own small device buffers of their own.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).
 *   - No allocation, no host synchronisation on any hot call: every hot call
 *     is capturable into a hipGraph.
 *   - Return value: 0 on success, a negative VAD_E* code for argument
 *     errors, or a positive hipError_t from the HIP runtime.
 */
#ifndef VAD_AMD_H
#define VAD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAD_MAX_FILTERS 64
#define VAD_MAX_MFCC 16
#define VAD_MAX_TAPS 16384
#define VAD_FFT_N 512
#define VAD_MAX_FFT_N 8192  /* other fft_n (2..8192) run a direct-DFT path */
#define VAD_MAX_FFN_LAYERS 4

#define VAD_OK 0
#define VAD_EINVAL (-1)        /* bad argument (null, negative size, ...) */
#define VAD_EUNSUPPORTED (-2)  /* valid for the reference, not built here (see each entry) */
#define VAD_ENOMEM (-3)
#define VAD_ERCCL (-4)         /* RCCL returned an error: vad_rccl_error_string() */

typedef struct vad_mfcc_plan vad_mfcc_plan;
typedef struct vad_ffn_plan vad_ffn_plan;

/* Library version string. */
const char* vad_version(void);

/* Number of frames split_into_frames() yields: frames are taken while
 * len - offset > frame_size (reference dataset/file_processing.py:99). */
int64_t vad_n_frames(int64_t n_samples, int32_t frame_size, int32_t hop);

/* ---------------------------------------------------------------------------
 * MFCC plan.  Replaces the per-call arguments of mfcc.get_mfcc /
 * get_mfcc_from_spec (reference mfcc.py:67-78): the (n_filters, 256)
 * filterbank from get_mel_filterbanks (mfcc.py:39-56, built on the host in
 * fp64 exactly as the reference does), the MFCC count (mfcc.py:76 [:mfcc_n])
 * and the lifter length (mfcc.py:85, L=22 in every reference call).
 * fft_n: any length 2..VAD_MAX_FFT_N, as np.fft.fft(frame, fft_n) takes
 * (mfcc.py:61; the filterbank is then (n_filters, fft_n / 2)).  512, the
 * reference's only value (config.py:27, sklearn_analyser.py:21), runs the
 * radix-16 x 16 kernels; other lengths a direct DFT with fp64 accumulation
 * (vad_mfcc_f32 / _i16, vad_spec_*, vad_mfcc_from_spec_f32, the workspace
 * form of vad_mfcc_ffn and vad_stream_step; the fused clip kernel, the
 * analysis window and vad_stream_hop return VAD_EUNSUPPORTED for them).
 * ------------------------------------------------------------------------- */
int vad_mfcc_plan_create(const double* filterbank_host, int32_t n_filters, int32_t fft_n,
                         int32_t mfcc_n, int32_t lifter_L, vad_mfcc_plan** out);
/* destroy: frees the plan's device tables with hipFree, which waits for the
 * device, so launches still queued with the plan complete first (a plan
 * captured in a hipGraph must outlive the graph's replays). */
int vad_mfcc_plan_destroy(vad_mfcc_plan* plan);

/* Kernel variant a plan dispatches to: 0 = runtime filterbank tables,
 * 1 / 2 = the compile-time tables of the reference's 26 / 40-filter banks
 * (selected only when the plan equals them bit for bit).  set_variant(0)
 * forces the runtime path (tests compare the two). */
int32_t vad_mfcc_plan_variant(const vad_mfcc_plan* plan);
int vad_mfcc_plan_set_variant(vad_mfcc_plan* plan, int32_t variant);

/* Optional stages NOT in the reference (mfcc.py:59-61 feeds the raw frame to
 * the FFT: rectangular window, no pre-emphasis; BASELINE's north_star names
 * both).  Default off; with both off every output is bit-identical to a plan
 * that never had them.  Parity for them is pinned to the oracle's
 * restatement only (python_speech_features conventions).
 *   set_window: multiply sample t of every frame by window_host[t] (t < len
 *     <= 512, e.g. numpy.hamming(400)) before the FFT; NULL removes it.
 *     Windowed plans run the runtime-table kernel (variant kSpecWindow = 3).
 *   vad_preemphasis_f32: y[r][0] = x[r][0], y[r][t] = x[r][t] - coeff
 *     x[r][t-1] for each of n_rows rows of row_len samples (a clip: one row),
 *     out of place -- run before framing. */
int vad_mfcc_plan_set_window(vad_mfcc_plan* plan, const float* window_host, int32_t len);
int vad_preemphasis_f32(const float* x, float* y, int64_t n_rows, int64_t row_len, int64_t row_stride,
                        float coeff, void* stream);

/* Frames f = 0..n_frames-1 start at src + f*frame_stride and hold frame_len
 * samples (fp32); only the first min(frame_len, 512) feed the 512-point FFT
 * (np.fft.fft(x, 512) zero-pads / truncates, mfcc.py:61).
 * A clip framed at hop H is frame_stride = H, frame_len = 400
 * (file_processing.py:80-103); a frame matrix is frame_stride = row length. */

/* get_spec_mag (mfcc.py:59-61) of every frame -> spec[f*256 + k], fp32. */
int vad_spec_f32(const vad_mfcc_plan* plan, const float* src, int64_t frame_stride,
                 int32_t frame_len, int64_t n_frames, float* spec, void* stream);

/* get_mfcc (mfcc.py:67-69) of every frame -> mfcc[f*mfcc_n + c], fp32. */
int vad_mfcc_f32(const vad_mfcc_plan* plan, const float* src, int64_t frame_stride,
                 int32_t frame_len, int64_t n_frames, float* mfcc, void* stream);

/* int16 PCM input: the same as vad_spec_f32 / vad_mfcc_f32 on the samples
 * converted to fp32 (exact), i.e. the reference's int16 wav data followed by
 * astype(float32) (vad.py:37, dataset/file_processing.py:26-35), at half the
 * input bytes.  Frames are src + f*frame_stride (in samples). */
int vad_spec_i16(const vad_mfcc_plan* plan, const int16_t* src, int64_t frame_stride,
                 int32_t frame_len, int64_t n_frames, float* spec, void* stream);
int vad_mfcc_i16(const vad_mfcc_plan* plan, const int16_t* src, int64_t frame_stride,
                 int32_t frame_len, int64_t n_frames, float* mfcc, void* stream);

/* get_mfcc_from_spec (mfcc.py:72-78) of n spectra spec[f*256 + k]. */
int vad_mfcc_from_spec_f32(const vad_mfcc_plan* plan, const float* spec, int64_t n,
                           float* mfcc, void* stream);

/* ---------------------------------------------------------------------------
 * FFN plan: a Keras Sequential of Dense layers with ReLU between them and a
 * softmax at the end, predicted class = argmax (reference
 * learning/ffn_trainer.py:106-116; config.py:45-47 labels).  Weights are
 * Keras-layout W (in, out) row-major fp32 and b (out).  Constraints of this
 * build: 1..4 layers, in_dim <= 64, hidden <= 64, classes <= 4.
 * ------------------------------------------------------------------------- */
int vad_ffn_plan_create(int32_t n_layers, const int32_t* dims /* n_layers+1 */,
                        const float* const* W_host, const float* const* b_host,
                        vad_ffn_plan** out);
int vad_ffn_plan_destroy(vad_ffn_plan* plan);

/* Arithmetic of the forward.  VAD_FFN_SPLIT_F16 (the default of the two
 * specialised topologies 39-64-32-16-3 and 13-64-64-N): every GEMM operand
 * split v = hi + lo into two f16 halves, lo*hi + hi*lo + hi*hi accumulated in
 * f32 on v_mfma_f32_16x16x32_f16 (~22-bit operands, logits within a few f32
 * ulps of an exact-f32 forward; tests/test_gpu_fullsize.py bounds it).
 * VAD_FFN_EXACT_F32: v_mfma_f32_16x16x4_f32 (exact f32 products; every other
 * topology always runs this).  set_arith returns VAD_EINVAL for split-f16 on
 * a topology without it. */
#define VAD_FFN_EXACT_F32 0
#define VAD_FFN_SPLIT_F16 1
int32_t vad_ffn_plan_arith(const vad_ffn_plan* plan);
int vad_ffn_plan_set_arith(vad_ffn_plan* plan, int32_t arith);

/* Feature rows (reference feature layout, 39 = 3 x 13):
 *   mode VAD_FEAT_ANALYSER: [Mn, M+1 - M-1, (M+2 - Mn) - (Mn - M-2)] with the
 *     centre MFCC normalised by the 5-frame mean / std (ddof 0)
 *     (realtime_analysis/sklearn_analyser.py:52-69,103-107);
 *   mode VAD_FEAT_OFFLINE: [Mc, M+1 - M-1, (M+2 - Mc) - (Mc - M-2)], no
 *     normalisation (dataset/file_processing.py:40-70).
 * Row i is centred on MFCC frame i+2, i = 0..n_frames-6 (F-5 rows; the last
 * full window is never emitted, exactly as both reference loops do).
 * Supported range (analyser mode): the normalisation is fp32, v_rsq_f32 on
 * 0.2 * var * 2^24.  For caller-supplied rows whose 5-frame std lies in
 * [2^-60, 2^50] Mn is the fp32 formula's (log-MFCCs of any audio are far
 * inside); past ~2^52 the scaled variance overflows and Mn = 0, below ~2^-75
 * the squares underflow and Mn = +-inf, where the reference's fp64 gives a
 * finite value (tests/test_gpu_parity.py::test_feature_range_edges). */
#define VAD_FEAT_ANALYSER 0
#define VAD_FEAT_OFFLINE 1

/* features[i*3*mfcc_n + j] (fp32), i < n_frames-5. */
int vad_features_f32(const float* mfcc, int64_t n_frames, int32_t mfcc_n, int32_t mode,
                     float* features, void* stream);

/* Labels of every analyser window: classifier.predict of the features above
 * (sklearn_analyser.py:71) -> labels[i] (uint8), i < n_frames-5. */
int vad_features_ffn(const vad_ffn_plan* ffn, const float* mfcc, int64_t n_frames,
                     int32_t mfcc_n, int32_t mode, uint8_t* labels, void* stream);

/* The same labels plus every window's fp32 logits, logits[i*n_classes + c]
 * (before the softmax; parity tests of the FFN arithmetic). */
int vad_features_ffn_logits(const vad_ffn_plan* ffn, const float* mfcc, int64_t n_frames,
                            int32_t mfcc_n, int32_t mode, uint8_t* labels, float* logits, void* stream);

/* FFN forward over caller-built feature rows x[i*in_dim + j] (predict on a
 * batch, ffn_trainer.py:106-116) -> labels[i]. */
int vad_ffn_predict(const vad_ffn_plan* ffn, const float* x, int64_t n, uint8_t* labels,
                    void* stream);

/* Clip path: framing + MFCC + features + FFN (dataset_creator/process_file
 * framing, file_processing.py:38-70, with the analyser's classifier call,
 * sklearn_analyser.py:71).  labels[i] for windows i < n_frames-5 of the clip.
 * Two forms, identical labels:
 *   workspace != NULL (>= vad_mfcc_ffn_workspace_bytes(): the clip's MFCC
 *     rows): the MFCC kernel, then the window kernel -- the faster form on
 *     gfx950;
 *   workspace == NULL: one fused kernel, the MFCC rows never leave the CU --
 *     for the reference framing (frame 400, hop 160), the compiled 26-filter
 *     bank, a split-f16 FFN topology (39-64-32-16-3 or 13-64-64-N) and
 *     pair-aligned audio (8 B fp32 / 4 B int16: every torch allocation is);
 *     VAD_EINVAL otherwise.  vad_mfcc_ffn_fusable() tells whether the plans
 *     and framing qualify. */
size_t vad_mfcc_ffn_workspace_bytes(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, int64_t n_samples,
                                    int32_t frame_size, int32_t hop);
int32_t vad_mfcc_ffn_fusable(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, int32_t frame_size,
                             int32_t hop);
int vad_mfcc_ffn(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, const float* audio,
                 int64_t n_samples, int32_t frame_size, int32_t hop, int32_t mode,
                 uint8_t* labels, void* workspace, size_t workspace_bytes, void* stream);
/* The same from int16 PCM (the wav samples vad.py:37 converts with
 * astype(float32); the conversion is exact, so the labels are identical). */
int vad_mfcc_ffn_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, const int16_t* audio,
                     int64_t n_samples, int32_t frame_size, int32_t hop, int32_t mode,
                     uint8_t* labels, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * FFN training (reference learning/ffn_trainer.py:118-154: Keras
 * optimizer='adadelta', loss='categorical_crossentropy', train_on_batch):
 * many models per launch, one workgroup per model, the model's state in LDS
 * for all the steps of a launch.
 *
 * A model's state block is 3 * count floats, count =
 * vad_ffn_train_param_count(): [params | E[g^2] | E[dx^2]], each section
 * W0 (in, out) row-major, b0, W1, b1, ...  Zero accumulators = a fresh model.
 * Model m's block starts at state + m * 3 * count.
 *
 * One step on rows r < batch of x[order[step * batch + r]] (x: n_rows rows of
 * dims[0] floats, y: their class indices): forward with ReLU between layers
 * and a max-subtracted softmax, loss = -mean(log p[label]), gradient
 * (p - onehot) / batch back through the layers, then Adadelta (Keras 1 /
 * torch.optim.Adadelta) on every parameter:
 *   a = rho a + (1 - rho) g^2;  u = g sqrt(d + eps) / sqrt(a + eps);
 *   p -= lr u;  d = rho d + (1 - rho) u^2.
 * The softmax output is not clipped before the log (Keras clips it to
 * [1e-7, 1 - 1e-7]).  GEMMs: v_mfma_f32_16x16x4_f32, everything else fp32 in
 * a fixed order; a run is bit-reproducible, and a model's result does not
 * depend on the other models of the launch.
 *
 * Shapes: those of vad_ffn_plan_create (1..4 layers, every dim 1..64, classes
 * <= 4), batch 1..64.  LDS budget: 4 bytes x (3 count, rounded up to 4,
 *   + bp * (2 (pad16(dims[0]) + 2) + sum_{l=1..L-1} (pad16(dims[l]) + 2)
 *           + sum_{l=1..L} (pad16(dims[l]) + 2)) + 128)  <=  160 KiB,
 * bp = batch rounded up to 16, pad16 = rounded up to 16; VAD_EUNSUPPORTED
 * past it.  39-64-32-16-3 and 13-64-64-2 fit at every batch.
 * ------------------------------------------------------------------------- */
#define VAD_TRAIN_EVAL_CHUNK_ROWS 1024

/* Parameters of one model; -1 for shapes outside the limits above. */
int64_t vad_ffn_train_param_count(int32_t n_layers, const int32_t* dims /* n_layers+1 */);

/* n_steps consecutive steps of n_models models.  order: n_steps * batch row
 * indices per model, model m's at order + m * order_model_stride (0: every
 * model runs the same order).  The caller guarantees 0 <= order[i] < n_rows
 * and y[i] < dims[n_layers]; neither is checked on the device (a label is
 * only ever compared, an index is an address).  hyper: (lr, rho, eps) per
 * model.  step_loss (may be NULL): step_loss[m * n_steps + k] = the loss of
 * step k before its update. */
int vad_ffn_train_steps(int32_t n_layers, const int32_t* dims, float* state, int64_t n_models,
                        const float* x, const uint8_t* y, int64_t n_rows, const int32_t* order,
                        int64_t order_model_stride, int32_t batch, int64_t n_steps,
                        const float* hyper, float* step_loss, void* stream);

/* model.evaluate_generator (ffn_trainer.py:154).  Rows are taken in chunks
 * of VAD_TRAIN_EVAL_CHUNK_ROWS: n_chunks = vad_ffn_train_eval_chunks(n_rows)
 * (-1 for n_rows < 0); loss_sums[m * n_chunks + c] = the summed loss (fp32)
 * and correct[m * n_chunks + c] = the rows whose first-max argmax equals the
 * label, of chunk c under model m.  The caller adds the chunks. */
int64_t vad_ffn_train_eval_chunks(int64_t n_rows);
int vad_ffn_train_eval(int32_t n_layers, const int32_t* dims, const float* state, int64_t n_models,
                       const float* x, const uint8_t* y, int64_t n_rows, float* loss_sums,
                       int32_t* correct, void* stream);

/* ---------------------------------------------------------------------------
 * Decision-tree plan: the classifier vad.py deploys
 * (learning/decision_classifier_trainer.py:26-35: sklearn
 * DecisionTreeClassifier, predict through sklearn_analyser.py:71) as a flat
 * node table, e.g. from an sklearn tree_: feature[i] (< 0 for a leaf),
 * threshold[i] (float64), left[i] / right[i] (children_left / _right),
 * leaf_class[i] = argmax of the leaf's value row (class index), and nan_left[i]
 * (missing_go_to_left, sklearn >= 1.3; NULL: NaN goes right).  Traversal is
 * sklearn's: left iff float32(x[feature]) <= threshold (compared in double).
 * Returned labels are class indices (uint8); the caller maps them through
 * classes_.  Constraints: 1 <= n_nodes <= 2^24, feature < n_features <= 64.
 * ------------------------------------------------------------------------- */
typedef struct vad_tree_plan vad_tree_plan;

int vad_tree_plan_create(int32_t n_nodes, const int32_t* feature, const double* threshold,
                         const int32_t* left, const int32_t* right, const int32_t* leaf_class,
                         const uint8_t* nan_left, int32_t n_features, vad_tree_plan** out);
int vad_tree_plan_destroy(vad_tree_plan* plan);

/* labels[i] of caller-built feature rows x[i*n_features + f] (fp32). */
int vad_tree_predict(const vad_tree_plan* tree, const float* x, int64_t n, uint8_t* labels,
                     void* stream);

/* Labels of every window of an MFCC sequence (features as vad_features_f32,
 * mode VAD_FEAT_ANALYSER or VAD_FEAT_OFFLINE), labels[i], i < n_frames-5. */
int vad_features_tree(const vad_tree_plan* tree, const float* mfcc, int64_t n_frames,
                      int32_t mfcc_n, int32_t mode, uint8_t* labels, void* stream);

/* ---------------------------------------------------------------------------
 * Decision-tree training (learning/decision_classifier_trainer.py:26-30; the
 * grid of learning/cross_validation.py:20-27): sklearn 1.7.2's Gini / best
 * splitter over all features and unweighted rows, made deterministic (ties
 * between features: the lowest feature, then the lowest position), for
 * n_jobs jobs in one chain of launches.  DESIGN.md section 4 has the rule.
 *
 * x[i*n_features + f] (fp32, finite) and y[i] (class index < n_classes) are
 * the device rows; order[f*n_rows + i] (int32, device) lists the rows by
 * rising x[., f] (any order among equal values).  Job j trains on the rows r
 * with mask[j*n_rows + r] != 0 (device; NULL: every job takes every row);
 * jobs[j].n_rows must be their number.  Limits: 1 <= n_features <= 64,
 * 2 <= n_classes <= 8, 1 <= n_rows < 2^27, 1 <= n_jobs <= 4096 (jobs of one
 * row: at most 1024), all jobs' rows together < 2^31 - 4096.
 *
 * Job j's nodes are written at the sum of the earlier jobs' node_capacity, in
 * level order (the root first, the two children of a node adjacent); a leaf
 * has feature -1, threshold -2, left = right = -1.  feature / threshold /
 * left / right / leaf / nan_left are what vad_tree_plan_create reads; value
 * holds n_classes class counts per node.  status[j] is 0 or a sum of the
 * VAD_TREE_TRAIN_* bits.  vad_tree_train_node_capacity(n_rows,
 * min_samples_leaf) = 2*floor(n_rows / max(min_samples_leaf, 1)) - 1 (at least
 * 1) always suffices; with less the job stops where its next level would not
 * fit, nothing is written past its nodes, and the call returns VAD_ENOMEM.
 *
 * All arguments are checked before any HIP call.  The call returns after the
 * stream has run it: it reads two integers back per level of the trees (the
 * count is returned in *n_levels, may be NULL).  VAD_EINVAL after the launch:
 * a job's mask does not hold jobs[j].n_rows rows, or a label >= n_classes.
 * ------------------------------------------------------------------------- */
#define VAD_TREE_TRAIN_MAX_CLASSES 8
#define VAD_TREE_TRAIN_ROW_BITS 27
#define VAD_TREE_TRAIN_OVERFLOW 1 /* status: node_capacity too small */
#define VAD_TREE_TRAIN_BAD_ROWS 2 /* status: mask / n_rows / label mismatch */
#define VAD_TREE_TRAIN_BAD_WEIGHT 4 /* status: a job's total weight above VAD_TREE_TRAIN_MAX_WEIGHT */
#define VAD_TREE_TRAIN_MAX_WEIGHT (1 << 26) /* vad_tree_train_weighted: largest total weight of a job */

typedef struct vad_tree_job {
  int64_t n_rows;
  int64_t node_capacity;
  int32_t max_depth;         /* >= 1 */
  int32_t min_samples_split; /* >= 2 */
  int32_t min_samples_leaf;  /* >= 1 */
  int32_t reserved;          /* 0 */
} vad_tree_job;

typedef struct vad_tree_tables { /* device arrays; N = the sum of node_capacity */
  int32_t* feature;              /* [N] */
  double* threshold;             /* [N] */
  int32_t* left;                 /* [N] */
  int32_t* right;                /* [N] */
  int32_t* leaf;                 /* [N] */
  uint8_t* nan_left;             /* [N] */
  int32_t* n_node_samples;       /* [N] */
  int32_t* depth;                /* [N] */
  int32_t* value;                /* [N * n_classes] */
  int32_t* n_nodes;              /* [n_jobs] */
  int32_t* status;               /* [n_jobs] */
} vad_tree_tables;

/* -1 for n_rows < 1 or min_samples_leaf < 1 */
int64_t vad_tree_train_node_capacity(int64_t n_rows, int32_t min_samples_leaf);
/* device bytes vad_tree_train needs for these jobs; 0 for arguments it refuses */
size_t vad_tree_train_workspace_bytes(int64_t n_rows, int32_t n_features, int32_t n_classes, int32_t n_jobs,
                                      const vad_tree_job* jobs);
int vad_tree_train(const float* x, const uint8_t* y, int64_t n_rows, int32_t n_features, int32_t n_classes,
                   const int32_t* order, const uint8_t* mask, int32_t n_jobs, const vad_tree_job* jobs,
                   const vad_tree_tables* tables, void* workspace, size_t workspace_bytes, int32_t* n_levels,
                   void* stream);
/* vad_tree_train with a feature subset per job (a forest's max_features in
 * its per-tree form): feature_masks[j] (host, n_jobs words) has bit f set when
 * job j may split on feature f; NULL: every job may use every feature, and
 * the call is vad_tree_train.  A feature whose bit is clear contributes no
 * candidate to the job's nodes; the rule is otherwise unchanged (the largest
 * score, then the lowest allowed feature, then the lowest position), so job j
 * grows the tree of its rows restricted to its columns.  A job none of whose
 * allowed features can split is a single leaf.  VAD_EINVAL before any HIP
 * call: a mask with no bit below n_features set. */
int vad_tree_train_features(const float* x, const uint8_t* y, int64_t n_rows, int32_t n_features, int32_t n_classes,
                            const int32_t* order, const uint8_t* mask, const uint64_t* feature_masks, int32_t n_jobs,
                            const vad_tree_job* jobs, const vad_tree_tables* tables, void* workspace,
                            size_t workspace_bytes, int32_t* n_levels, void* stream);
/* vad_tree_train_features with an integer weight per (job, row) in the mask's
 * place: weights[j*n_rows + r] (uint8, device) is 0 for a row that is not in
 * job j and otherwise the weight sklearn's fit(X, y, sample_weight=) gives the
 * row -- bootstrap counts, integer class weights or their product.  NULL: all
 * ones (every job takes every row once, the unweighted rule and kernels).
 * jobs[j].n_rows is the number of rows with weight > 0.  Distinct rows go on
 * counting for n_node_samples, max_depth, min_samples_split, min_samples_leaf,
 * a candidate's position and nan_left; the class counts are weighted: the
 * score is (sum_k cL[k]^2) / WL + (sum_k cR[k]^2) / WR with c[k] the summed
 * weights of class k and W their total, a node is pure when its largest count
 * is its total, leaf is the first maximum of the weighted counts and value
 * holds them.  A job's total weight is at most VAD_TREE_TRAIN_MAX_WEIGHT
 * (2^26: every sum of squares is then exact in a double, as sklearn adds
 * them).  vad_tree_train_node_capacity is unchanged (it bounds by distinct
 * rows); the workspace is vad_tree_train_weighted_workspace_bytes.
 * VAD_EINVAL before any HIP call: what vad_tree_train_features refuses, NULL
 * weights with a job whose n_rows is not n_rows.  VAD_EINVAL after the
 * launch: a job's weights do not hold jobs[j].n_rows rows above 0, a label >=
 * n_classes, or a total weight above the limit (status says which). */
size_t vad_tree_train_weighted_workspace_bytes(int64_t n_rows, int32_t n_features, int32_t n_classes,
                                               int32_t n_jobs, const vad_tree_job* jobs);
int vad_tree_train_weighted(const float* x, const uint8_t* y, int64_t n_rows, int32_t n_features, int32_t n_classes,
                            const int32_t* order, const uint8_t* weights, const uint64_t* feature_masks,
                            int32_t n_jobs, const vad_tree_job* jobs, const vad_tree_tables* tables, void* workspace,
                            size_t workspace_bytes, int32_t* n_levels, void* stream);

/* ---------------------------------------------------------------------------
 * Random forest: n_trees decision trees in one node table, their leaf class
 * shares averaged -- predict_proba / predict of sklearn's
 * RandomForestClassifier, ExtraTreesClassifier and BaggingClassifier over
 * decision trees with n_jobs = 1.  Per row, n_classes double accumulators
 * start at 0; for t = 0 .. n_trees-1 in order acc[k] += proba[leaf_t][k];
 * then acc[k] /= n_trees.  The score is (float)acc[active], the label the
 * first maximum of acc (a class index).  The walk is vad_tree_plan's.
 *
 * The node arrays are vad_tree_plan_create's (host), the trees one after
 * another: tree t is the nodes [roots[t], roots[t + 1]) (the last tree ends
 * at n_nodes), its root first; roots[0] = 0, roots ascending; left / right are
 * indices into the whole table and must stay inside their tree.  proba[i *
 * n_classes + k] (host, float64) is node i's share of class k (the rows of
 * leaves are read).  Limits: n_trees >= 1, 1 <= n_classes <= 8, n_nodes <=
 * 2^24, n_features <= 64; anything else, a root outside the table included,
 * is VAD_EINVAL before any HIP call.
 *
 * vad_forest_predict: rows x[i*n_features + f].  vad_features_forest: every
 * window of an MFCC sequence, as vad_features_tree (a clip's rows or a packed
 * clip batch's), the features of a window computed once for all trees.
 * labels[i] always, scores[i] when scores is not NULL.  VAD_EINVAL: a NULL
 * forest / input / labels, n or n_frames < 0, active outside 0 .. n_classes-1,
 * outputs that overlap the input or each other.
 * ------------------------------------------------------------------------- */
#define VAD_FOREST_MAX_CLASSES 8
typedef struct vad_forest vad_forest;

int vad_forest_create(int32_t n_nodes, const int32_t* feature, const double* threshold, const int32_t* left,
                      const int32_t* right, const uint8_t* nan_left, int32_t n_trees, const int32_t* roots,
                      int32_t n_classes, const double* proba, int32_t n_features, vad_forest** out);
int vad_forest_destroy(vad_forest* forest);
int vad_forest_predict(const vad_forest* forest, const float* x, int64_t n, int32_t active, uint8_t* labels,
                       float* scores, void* stream);
int vad_features_forest(const vad_forest* forest, const float* mfcc, int64_t n_frames, int32_t mfcc_n, int32_t mode,
                        int32_t active, uint8_t* labels, float* scores, void* stream);

/* ---------------------------------------------------------------------------
 * Offline dataset export (dataset_creator.py:58-66 -> file_processing.py,
 * dataset/utils.py).
 * ------------------------------------------------------------------------- */

/* scale_features (dataset/utils.py:5-34) of feature rows
 * rows[i*3*mfcc_n + t*mfcc_n + c] (t: mfcc / delta1 / delta2, the OFFLINE
 * layout), in place on the device: one global mean and population std per
 * group t over all rows, x = (x - mean_t) / std_t; statistics in fp64.
 * `workspace` (device, >= vad_scale_workspace_bytes()) ends with the six
 * doubles mean[3], std[3]. */
size_t vad_scale_workspace_bytes(void);
int vad_scale_features(float* rows, int64_t n_rows, int32_t mfcc_n, void* workspace,
                       size_t workspace_bytes, void* stream);

/* CSV text of host feature rows as write_features writes them
 * (file_processing.py:126-146: features, then the label; values printed like
 * numpy float32, rows ending in "\r\n").  Returns the bytes written, or
 * -(bytes needed) when buf is NULL or too small. */
int64_t vad_format_csv_rows(const float* rows, int64_t n_rows, int32_t n_cols, double label,
                            char* buf, int64_t buf_size);

/* ---------------------------------------------------------------------------
 * Dataset CSV import: the text that write_features / vad_format_csv_rows
 * wrote, back into feature rows and labels on the device (load_csv,
 * file_processing.py:151-184; create_file_index, file_index.py:7-23).
 *
 * `bytes` is the text on the device.  Lines end in "\r\n" or "\n"; the last
 * line may lack its terminator; a final '\n' starts no line.  The three
 * calls run in this order on one stream:
 *
 *   vad_csv_count_lines  writes the number of lines to *n_lines (device) and
 *                        leaves the per-tile carries in `ws`;
 *   vad_csv_index        from those carries (same bytes, n_bytes and ws):
 *                        index[r - skip] = base + byte offset of line r for
 *                        skip <= r < skip + capacity -- create_file_index's
 *                        offsets when base is the text's offset in its file;
 *   vad_csv_parse        rows of n_cols comma-separated fields, one per index
 *                        entry (row r ends where row r + 1 starts, the last
 *                        at n_bytes).  X[r][j] = field columns[j] (host array
 *                        of n_used <= VAD_CSV_MAX_USED indices; NULL: columns
 *                        0 .. n_cols-2, n_used = n_cols - 1), the correctly
 *                        rounded double of the text cast once to float32, or
 *                        the double itself (out_f64 != 0); y[r] =
 *                        int(float(last field)).
 *
 * row_status[r] is 0 or a sum of VAD_CSV_ROW_*.  HOST: a used field that the
 * device does not decide (more than 19 significant digits, an unresolved
 * rounding, blanks, a signed nan, anything outside
 * [+-]?(d+[.d*]|.d+)([eE][+-]?d+)?, nan, [+-]?inf, [+-]?infinity); the caller
 * parses that row itself.  MALFORMED: not n_cols fields, more than
 * VAD_CSV_MAX_LINE bytes, or offsets outside the text.  LABEL: a label
 * outside 0..255.  X and y of a row with a nonzero status are unspecified.
 *
 * The scans run on tiles of VAD_CSV_TILE bytes, VAD_CSV_CARRY_PASS tile
 * counts per pass of the one carry workgroup.  VAD_EINVAL: a null pointer,
 * a negative size, skip or capacity, n_cols < 2 or > VAD_CSV_MAX_COLS, n_used
 * outside 1..VAD_CSV_MAX_USED, a column outside 0..n_cols-1, a misaligned
 * output, a workspace below vad_csv_workspace_bytes(n_bytes).
 * ------------------------------------------------------------------------- */
#define VAD_CSV_TILE 4096
#define VAD_CSV_CARRY_PASS 256
#define VAD_CSV_MAX_LINE 4096
#define VAD_CSV_MAX_COLS 2048
#define VAD_CSV_MAX_USED 1024
#define VAD_CSV_ROW_HOST 1
#define VAD_CSV_ROW_MALFORMED 2
#define VAD_CSV_ROW_LABEL 4
size_t vad_csv_workspace_bytes(int64_t n_bytes); /* 0 for n_bytes < 0 */
int vad_csv_count_lines(const uint8_t* bytes, int64_t n_bytes, int64_t* n_lines, void* ws, size_t ws_bytes,
                        void* stream);
int vad_csv_index(const uint8_t* bytes, int64_t n_bytes, int64_t skip, int64_t base, int64_t* index,
                  int64_t capacity, const void* ws, size_t ws_bytes, void* stream);
int vad_csv_parse(const uint8_t* bytes, int64_t n_bytes, const int64_t* index, int64_t n_rows, int64_t base,
                  int32_t n_cols, const int32_t* columns, int32_t n_used, int32_t out_f64, void* X, uint8_t* y,
                  int32_t* row_status, void* stream);

/* ---------------------------------------------------------------------------
 * Energy / ZCR / spectral analyser (realtime_analysis/simple_analyzer.py,
 * SimpleAnalyser): per-frame features in fp64, out[f*(3+n_bands) + i]:
 *   0  stEnergy(frame)                    = sum x^2 / frame_len
 *   1  stZCR(frame) * frame_len           (:210-215)
 *   2  np.std(|fft|) over all fft_len bins (:203-208)
 *   3+b stEnergy(|fft|[b*band_bins : (b+1)*band_bins])   (:171-197)
 * |fft| = |DFT_fft_len([zeros(pad), frame, zeros(pad)])| with
 * fft_len = frame_len + 2*pad (:386-400; pad 0: the frame itself): frames of
 * up to 8192 samples, fft_len up to 8193 (a power of two runs a radix-2 FFT,
 * any other length -- the reference's odd pads -- a direct DFT).
 * stEnergy / stZCR are pyAudioAnalysis's (restated; the package is absent).
 * Frames are frames + f*frame_stride (fp32 samples, exact for int16 audio).
 * ------------------------------------------------------------------------- */
int vad_simple_features(const float* frames, int64_t n_frames, int32_t frame_len,
                        int64_t frame_stride, int32_t fft_len, int32_t pad, int32_t band_bins,
                        int32_t n_bands, double* out, void* stream);

/* ---------------------------------------------------------------------------
 * Streams of that analyser: S independent SimpleAnalyser.feed_frame loops
 * (simple_analyzer.py:78-112, 144-164, 245-256) advanced by a block of K
 * frames each per call, every stream's state in device memory.
 *
 * state: n_streams records of vad_simple_stream_state_bytes(noise_buf_len)
 * bytes each (8-byte aligned), 1 <= noise_buf_len <= VAD_SIMPLE_MAX_NOISE:
 *   double noise[noise_buf_len][6]  energy, std|fft|, band 0..3 of the noise
 *                                   buffer's frames (their feature rows)
 *   double energy_thresh, spectral_std_thresh, spectral_energy_bands_thresh[4]
 *   int32  status         the 20-entry status buffer, bit 0 the newest entry
 *   int32  silence        1 / 0
 *   int32  noise_pointer
 *   int32  frame_number   frames fed
 * vad_simple_stream_init writes a whole record; all other entries read and
 * update it.
 *
 * A feature row is vad_simple_features' with n_bands = 4:
 * [stEnergy, zcr * frame_len, std|fft|, band 0..3].  The step is the
 * reference's, update for update: classification with the ZCR window
 * 5 <= z <= 20 and strict > everywhere else; the status buffer shifted, then
 * counted; silence off at 5 active entries, on again at 15 inactive ones (that
 * frame is still labelled active, and joins the noise buffer); thresholds
 * 0.75 t + 0.25 mean, two products and a sum, never an FMA.  The energy mean
 * is over energies truncated toward zero to uint32 (:309); an energy of 2^32
 * or more, where numpy's cast is undefined, saturates to 2^32 - 1.  The std
 * and band means are summed over the noise rows left to right, in double.
 *
 * frames: (K, S, frame_len), frame k of stream s at
 * frames + k * block_stride + s * stream_stride (elements), samples
 * contiguous; the frames of a block may not overlap each other (K blocks of
 * S rows, or S rows of K frames).  fft_len = frame_len + 2 * pad as for
 * vad_simple_features, 4 * band_bins <= fft_len.  A power-of-two fft_len up
 * to 4096 runs one kernel (one workgroup per stream); any other fft_len up
 * to 8193 runs vad_simple_features and then the state steps, takes fp32
 * frames only and needs features_out as its workspace.
 *   labels[k * label_block_stride + s] = 1 (active) / 0 (inactive).
 *   features_out (optional, (K, S, 7) doubles): the rows that were classified.
 *   voiced / voiced_len (optional, both or neither): voiced + s * voiced_stride
 *     receives the block's active frames of stream s packed in order (bits
 *     copied), voiced_len[s] their total length in samples; nothing past it
 *     is written.  voiced_stride >= n_frames * frame_len.
 * One or two kernels, no allocation, no synchronisation: capturable.
 *
 * VAD_EINVAL before any launch: a null required pointer, n_streams < 1,
 * n_frames < 0, noise_buf_len outside 1..VAD_SIMPLE_MAX_NOISE, frame_len < 2,
 * frame_len > 8192, fft_len != frame_len + 2 * pad or > 8193, band_bins < 1,
 * 4 * band_bins > fft_len, strides under which two frames of a block overlap
 * in the input or an output (stream_stride < frame_len with n_streams > 1; with
 * n_frames > 1 overlapping frames or label_block_stride < n_streams;
 * voiced_stride < n_frames * frame_len with n_streams > 1), voiced without
 * voiced_len or the reverse, n_frames * frame_len > INT32_MAX, a misaligned state,
 * int16 frames with an fft_len the one-kernel form does not take, such an
 * fft_len without features_out.  n_frames == 0: VAD_OK, nothing written.
 *
 * vad_simple_stream_state: the state steps alone over feats (K, S, 7).
 * vad_simple_stream_init: load_init_inactive_frames (:120-138) for every
 * stream from the rows feats (S, noise_buf_len, 7) of its init frames: noise
 * buffer, the three thresholds as plain means, status 0, silence 1,
 * noise_pointer 0, frame_number 0.
 *
 * Sessions (vad_simple_stream_block_sessions_f32 / _i16,
 * vad_simple_stream_state_sessions): the sibling entry's arguments, then three
 * per-stream device arrays read inside the kernels, so callers join, leave
 * and stall without a host step:
 *   frame_counts (S) int32: stream s takes n_s = min(max(frame_counts[s], 0),
 *     n_frames) frames, rows 0..n_s-1 of its column of the block.
 *   restart (S) uint8: nonzero makes the stream fresh before its frames of
 *     this call (its state record all zero, init_left = noise_buf_len); the
 *     kernel stores 0 back, so a flag set once restarts once, also when a
 *     captured graph is replayed.
 *   init_left (S) int32, read and written: the frames the stream still needs
 *     before it is initialised (0: initialised; set it to 0 after
 *     vad_simple_stream_init, to noise_buf_len with a zeroed record for a new
 *     batch).  While it is positive each frame taken is an init frame: its
 *     feature row fills noise row noise_buf_len - init_left, and the last one
 *     does what vad_simple_stream_init does on those noise_buf_len rows.
 *     Frames after it in the same block are classified.  The state record
 *     above does not change.
 *   labels: VAD_LABEL_INIT in the row of an init frame (never copied to
 *     voiced), VAD_LABEL_NO_HOP in rows n_s..n_frames-1; features_out rows
 *     n_s..n_frames-1 are not written by the one-kernel form (the two-launch
 *     form computes all rows).  voiced_len[s] counts the frames labelled 1.
 *   A stream with n_s = 0 and no restart keeps every byte of its record and
 *   its init_left.  With every count n_frames, no restart and every init_left
 *   0, all outputs equal the sibling entry's bit for bit.
 * VAD_EINVAL as for the sibling, and for a null frame_counts, restart or
 * init_left or a frame_counts / init_left that is not 4-byte aligned.
 * n_frames == 0: VAD_OK, nothing written, no flag consumed.
 * ------------------------------------------------------------------------- */
#define VAD_SIMPLE_MAX_NOISE 64
#define VAD_LABEL_INIT 253 /* a label row that holds one of the stream's init frames (sessions) */
size_t vad_simple_stream_state_bytes(int32_t noise_buf_len); /* 0 outside 1..VAD_SIMPLE_MAX_NOISE */
int vad_simple_stream_init(const double* feats, int64_t n_streams, int32_t noise_buf_len, void* state, void* stream);
int vad_simple_stream_block_f32(const float* frames, int64_t block_stride, int64_t stream_stride, int32_t frame_len,
                                int32_t fft_len, int32_t pad, int32_t band_bins, int64_t n_streams, int32_t n_frames,
                                int32_t noise_buf_len, void* state, uint8_t* labels, int64_t label_block_stride,
                                double* features_out, float* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                void* stream);
int vad_simple_stream_block_i16(const int16_t* frames, int64_t block_stride, int64_t stream_stride, int32_t frame_len,
                                int32_t fft_len, int32_t pad, int32_t band_bins, int64_t n_streams, int32_t n_frames,
                                int32_t noise_buf_len, void* state, uint8_t* labels, int64_t label_block_stride,
                                double* features_out, int16_t* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                void* stream);
int vad_simple_stream_state(const double* feats, int64_t n_streams, int32_t n_frames, int32_t noise_buf_len,
                            void* state, uint8_t* labels, int64_t label_block_stride, void* stream);
int vad_simple_stream_block_sessions_f32(const float* frames, int64_t block_stride, int64_t stream_stride,
                                         int32_t frame_len, int32_t fft_len, int32_t pad, int32_t band_bins,
                                         int64_t n_streams, int32_t n_frames, int32_t noise_buf_len, void* state,
                                         uint8_t* labels, int64_t label_block_stride, double* features_out,
                                         float* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                         const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                         void* stream);
int vad_simple_stream_block_sessions_i16(const int16_t* frames, int64_t block_stride, int64_t stream_stride,
                                         int32_t frame_len, int32_t fft_len, int32_t pad, int32_t band_bins,
                                         int64_t n_streams, int32_t n_frames, int32_t noise_buf_len, void* state,
                                         uint8_t* labels, int64_t label_block_stride, double* features_out,
                                         int16_t* voiced, int64_t voiced_stride, int32_t* voiced_len,
                                         const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                         void* stream);
int vad_simple_stream_state_sessions(const double* feats, int64_t n_streams, int32_t n_frames, int32_t noise_buf_len,
                                     void* state, uint8_t* labels, int64_t label_block_stride,
                                     const int32_t* frame_counts, uint8_t* restart, int32_t* init_left,
                                     void* stream);

/* ---------------------------------------------------------------------------
 * Streaming: S independent analyser streams advanced by one frame each
 * (SKLearnAnalyzer.feed_frame, sklearn_analyser.py:46-82, for S streams at
 * once).  State lives in device buffers the caller allocates with the sizes
 * below; every stream's state is independent.
 *   frames[s*frame_stride + t], t < frame_len: the new frame of stream s.
 *   ring: (S, 5, mfcc_n) fp32 MFCC ring; count: (S,) int32 frames seen.
 * After the call, labels[s] = class of the window centred 3 calls ago, or
 * 255 while the stream has seen fewer than 5 frames before this one
 * (feed_frame returns None for its first 5 calls, :48-50).
 * ------------------------------------------------------------------------- */
int64_t vad_stream_ring_floats(int64_t n_streams, int32_t mfcc_n);
/* Advance every stream's frame buffer by one hop, in place:
 *   frames[s, 0 : L-H] <- frames[s, H : L];  frames[s, L-H : L] <- hop[s, 0 : H]
 * (L = frame_len <= 1024, H = hop_len, 0 < H <= L), i.e. the next frame the
 * live loop of vad.py:37-49 hands to feed_frame.  One kernel; capturable. */
int vad_stream_push_hop(float* frames, int64_t frame_stride, int32_t frame_len, const float* hop,
                        int64_t hop_stride, int32_t hop_len, int64_t n_streams, void* stream);
/* One hop of every stream in ONE kernel (one wave per stream): advance the
 * frame buffer by the hop (as vad_stream_push_hop), 512-point FFT of the new
 * frame, mel / log10 / lifter x DCT, classify the ring's window, push the
 * new MFCC row (as vad_stream_step) -- the FFN forward in exact f32 on the
 * VALU, one output unit per lane.  The hipGraph-free, latency-first form of
 * push_hop + step for many small batches (BASELINE config 5). */
int vad_stream_hop(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                   int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams,
                   float* ring, int32_t* count, uint8_t* labels, void* stream);
/* n_hops consecutive hops of every stream in ONE kernel: exactly n_hops calls
 * of vad_stream_hop, hop k's new samples at hop + k * hop_block_stride (row s
 * at + s * hop_stride), its labels at labels + k * label_block_stride.  The
 * plan tables are staged into LDS once per launch instead of once per hop;
 * the form a hipGraph captures for many hops per replay (n_hops = 1 is
 * vad_stream_hop).  Same refusals as vad_stream_hop, plus VAD_EINVAL for
 * n_hops < 0, or n_hops > 1 with label_block_stride < n_streams, or with
 * hop rows that repeat or overlap: hop_block_stride must be > 0 and the rows
 * disjoint in one of the two orderings, hop-major (hop_block_stride >=
 * (n_streams - 1) * hop_stride + hop_len) or stream-major (hop_block_stride
 * >= hop_len and hop_stride >= (n_hops - 1) * hop_block_stride + hop_len,
 * e.g. an (S, K * hop) buffer viewed as (K, S, hop)). */
int vad_stream_hops(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                    int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams,
                    int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels,
                    int64_t label_block_stride, void* stream);
/* The same three entries for int16 PCM hop samples (the live signal as it
 * is recorded, vad.py:37): the arguments, checks and refusals of the f32
 * entry, all strides in int16 elements; a row needs only 2-byte alignment
 * (base, hop_stride, hop_block_stride and hop_len may be odd).  Each sample
 * is converted by an exact (float) where it is loaded, so labels and state
 * (frames, ring, count -- fp32 / int32 as above) are identical to the f32
 * entry fed the same values as floats. */
int vad_stream_push_hop_i16(float* frames, int64_t frame_stride, int32_t frame_len, const int16_t* hop,
                            int64_t hop_stride, int32_t hop_len, int64_t n_streams, void* stream);
int vad_stream_hop_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                       int32_t frame_len, const int16_t* hop, int64_t hop_stride, int32_t hop_len,
                       int64_t n_streams, float* ring, int32_t* count, uint8_t* labels, void* stream);
int vad_stream_hops_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                        int32_t frame_len, const int16_t* hop, int64_t hop_stride, int32_t hop_len,
                        int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count,
                        uint8_t* labels, int64_t label_block_stride, void* stream);
int vad_stream_step(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, const float* frames,
                    int64_t frame_stride, int32_t frame_len, int64_t n_streams, float* ring,
                    int32_t* count, uint8_t* labels, float* mfcc_scratch, void* stream);
/* The streaming entries with the decision tree (the classifier vad.py
 * deploys) in place of the FFN: vad_stream_hops_tree(_i16) is
 * vad_stream_hops(_i16) -- one wave per stream, n_hops hops per launch, the
 * same front end bit for bit -- ending in a walk of the tree that is uniform
 * over the wave; vad_stream_step_tree is vad_stream_step (the clip MFCC
 * kernel, then the ring step), the only streaming form for a windowed or
 * generic-fft_n plan.  labels are class indices (vad_tree_predict), 255
 * while a stream has seen fewer than five frames.
 * walk: VAD_TREE_WALK_AUTO walks the compact node table from LDS when it fits
 * (n_nodes <= vad_stream_tree_max_lds_nodes(plan): the plan's hop tables, the
 * 16-B nodes and one wave's scratch within 160 KiB) and from global memory
 * otherwise; VAD_TREE_WALK_GLOBAL always walks from global memory.  Both give
 * the same labels.
 * Refusals: those of vad_stream_hops, checked before any device call
 * (VAD_EINVAL for null plans, bad sizes, strides and layouts; after the
 * n_streams == 0 / n_hops == 0 return, VAD_EINVAL for a null buffer and
 * VAD_EUNSUPPORTED for a generic or windowed plan), plus VAD_EINVAL for any
 * other `walk` and for a tree with n_features > 3 * mfcc_n (as
 * vad_features_tree: a node's feature must lie in the window's row). */
#define VAD_TREE_WALK_AUTO 0
#define VAD_TREE_WALK_GLOBAL 1
int vad_stream_hops_tree(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames, int64_t frame_stride,
                         int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len, int64_t n_streams,
                         int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count, uint8_t* labels,
                         int64_t label_block_stride, int32_t walk, void* stream);
int vad_stream_hops_tree_i16(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                             int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                             int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring,
                             int32_t* count, uint8_t* labels, int64_t label_block_stride, int32_t walk, void* stream);
int vad_stream_step_tree(const vad_mfcc_plan* plan, const vad_tree_plan* tree, const float* frames,
                         int64_t frame_stride, int32_t frame_len, int64_t n_streams, float* ring, int32_t* count,
                         uint8_t* labels, float* mfcc_scratch, void* stream);
/* largest table the hop kernel walks from LDS; -1 on a bad plan */
int64_t vad_stream_tree_max_lds_nodes(const vad_mfcc_plan* plan);
/* The block shape of a hop launch, as a read-only query (no device work; the
 * launchers of every vad_stream_hops* entry call the same rule).  A block
 * holds 1, 2, 4, 8 or 16 waves, one stream each: at least 4 for a one-hop
 * launch and 1 for n_hops > 1, doubled while there are more streams than
 * waves x compute units of the current device (256 when none answers), then
 * halved while the staged tables and the waves' scratch exceed 160 KiB.
 *   vad_stream_hop_table_bytes       the bytes an FFN launch stages per block
 *                                    (the plan's hop tables and the weights);
 *   vad_stream_hop_tree_table_bytes  the same for a tree launch with `walk`
 *                                    (the hop tables, and the 16-B nodes when
 *                                    they are walked from LDS);
 *   vad_stream_hop_block_waves       waves per block for those bytes, or 0
 *                                    for n_streams == 0 or n_hops == 0 (the
 *                                    entries return before any launch).
 * Refusals: VAD_EINVAL for a null or table-less plan, any other `walk`, a
 * negative argument, and table_bytes that leave no room for one wave. */
int64_t vad_stream_hop_table_bytes(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn);
int64_t vad_stream_hop_tree_table_bytes(const vad_mfcc_plan* plan, const vad_tree_plan* tree, int32_t walk);
int32_t vad_stream_hop_block_waves(int64_t table_bytes, int64_t n_streams, int32_t n_hops);

/* Scored hops: the operating point on the live path.  Each entry is the label
 * entry of the same name plus `active`, `scores` and `score_block_stride`:
 * besides labels[k * label_block_stride + s] the hop kernel writes the fp32
 * score of class index `active`, in [0, 1], to
 * scores[k * score_block_stride + s] -- NaN for a hop whose stream has no
 * window yet (label 255).  Labels, frames, ring and count are those of the
 * label entry, bit for bit.
 *   FFN   s = 1 / (1 + sum_{j != active} expf(z_j - z_active)) of the window's
 *         logits, 0 when a logit is inf or NaN: vad_scores_from_logits' function
 *         (one device function serves both).
 *   tree  the plan's score table (vad_tree_plan_set_scores: a host array of
 *         n_classes rows of n_nodes floats, row c the score of class c per
 *         node, copied to the device; it may be set again) read at the leaf
 *         NODE the walk ends in, row `active`: vad_features_tree_scores' value.
 * Refusals: those of the label entries, plus VAD_EINVAL for `active` outside
 * [0, the classifier's classes) (the FFN's outputs; the rows of the tree's
 * score table), a tree plan without a score table, a null `scores` and, for
 * n_hops > 1, score_block_stride < n_streams.  All before any device call. */
int vad_tree_plan_set_scores(vad_tree_plan* plan, const float* table /* host, n_classes x n_nodes */,
                             int32_t n_classes);
int32_t vad_tree_plan_score_classes(const vad_tree_plan* plan); /* 0: no table; -1: null plan */
int vad_stream_hops_scores(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                           int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len,
                           int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count,
                           uint8_t* labels, int64_t label_block_stride, int32_t active, float* scores,
                           int64_t score_block_stride, void* stream);
int vad_stream_hops_scores_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames,
                               int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                               int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                               float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                               int32_t active, float* scores, int64_t score_block_stride, void* stream);
int vad_stream_hops_tree_scores(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                int64_t frame_stride, int32_t frame_len, const float* hop, int64_t hop_stride,
                                int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride, int32_t walk,
                                int32_t active, float* scores, int64_t score_block_stride, void* stream);
int vad_stream_hops_tree_scores_i16(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                    int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                                    int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                    float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                    int32_t walk, int32_t active, float* scores, int64_t score_block_stride,
                                    void* stream);
/* Live spectral noise subtraction in the hop kernels.  The reference's live
 * analyser computes a noise estimate and the subtracted spectrum and then
 * takes the MFCC from the unsubtracted one (sklearn_analyser.py:84-101,
 * 122-123); these entries take it from the subtracted spectrum.  Per stream,
 * beside frames / ring / count, contiguous fp32 arrays in the kernels' units
 * |2X|^2 (x 2^-20 gives |X/512|^2), all zero = a fresh stream:
 *   spec_ring   (S, 5, 256)  raw power rows of the last five frames; slot =
 *                            the MFCC ring's slot of the same frame
 *   noise_rows  (S, 5, 256)  the noise rows in arrival order, row 0 the oldest
 *   noise_count (S) int32    rows held, 0..5
 *   noise_est   (S, 256)     the estimate e in force: the mean m of the rows
 *                            held, (((r0 + r1) + r2) + ...) / n, low-passed
 *                            over the bins with the reference's wrap at bin 0:
 *                            e[0] = alpha m[255] + (1 - alpha) m[0],
 *                            e[i] = alpha e[i-1] + (1 - alpha) m[i]; fp32, in
 *                            the order stream_denoise.h states (an affine scan
 *                            across the wave); all zero with no rows held
 * One hop: the frame advances, its power row p goes to spec_ring, the MFCC
 * row is taken from max(p - e, 0) (NaN kept), the window of the five previous
 * rows is classified as by the plain entries, and, if the stream has a window,
 * its label is noise_class and update is 1, the RAW row of the window's middle
 * frame (three hops old) joins noise_rows -- the oldest row dropped past five
 * -- and e is taken anew, in force from the next hop.  With an all-zero state
 * and update 0 labels, scores, frames, ring and count are the plain entries',
 * bit for bit.
 * Arguments: those of the scored entry of the same classifier and input type,
 * then the four state arrays, alpha in [0, 1), noise_class, update (0 / 1).
 * scores may be null (labels only; active and score_block_stride are then not
 * read, and a tree plan needs no score table).
 * vad_stream_noise_load(_i16): n = 1..5 frames per stream, frame j of stream s
 * at frames + s * stream_stride + j * frame_stride (elements), become noise
 * rows 0..n-1 (the row a hop stores for that frame, bit for bit), the count n
 * and the estimate: the reference's load_init_inactive_frames.
 * Refusals (VAD_EINVAL, before any device call): those of the scored entries;
 * a null state array; two state arrays that overlap; alpha outside [0, 1) or
 * NaN; noise_class outside the classifier's classes (the FFN's outputs, the
 * tree's leaf classes); update not 0 / 1; n outside 1..5.  A plan whose fft_n
 * is not 512, or with an analysis window: VAD_EUNSUPPORTED, as the plain
 * hop entries. */
int64_t vad_stream_spec_ring_floats(int64_t n_streams);  /* n_streams * 5 * 256 */
int64_t vad_stream_noise_rows_floats(int64_t n_streams); /* n_streams * 5 * 256 */
int64_t vad_stream_noise_est_floats(int64_t n_streams);  /* n_streams * 256 */
int vad_stream_hops_denoise(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                            int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len,
                            int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count,
                            uint8_t* labels, int64_t label_block_stride, int32_t active, float* scores,
                            int64_t score_block_stride, float* spec_ring, float* noise_rows, int32_t* noise_count,
                            float* noise_est, float alpha, int32_t noise_class, int32_t update, void* stream);
int vad_stream_hops_denoise_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames,
                                int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                                int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                int32_t active, float* scores, int64_t score_block_stride, float* spec_ring,
                                float* noise_rows, int32_t* noise_count, float* noise_est, float alpha,
                                int32_t noise_class, int32_t update, void* stream);
int vad_stream_hops_tree_denoise(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                 int64_t frame_stride, int32_t frame_len, const float* hop, int64_t hop_stride,
                                 int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                 float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                 int32_t walk, int32_t active, float* scores, int64_t score_block_stride,
                                 float* spec_ring, float* noise_rows, int32_t* noise_count, float* noise_est,
                                 float alpha, int32_t noise_class, int32_t update, void* stream);
int vad_stream_hops_tree_denoise_i16(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                     int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                                     int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                     float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                     int32_t walk, int32_t active, float* scores, int64_t score_block_stride,
                                     float* spec_ring, float* noise_rows, int32_t* noise_count, float* noise_est,
                                     float alpha, int32_t noise_class, int32_t update, void* stream);
int vad_stream_noise_load(const vad_mfcc_plan* plan, const float* frames, int64_t stream_stride, int64_t frame_stride,
                          int32_t frame_len, int32_t n, int64_t n_streams, float* noise_rows, int32_t* noise_count,
                          float* noise_est, float alpha, void* stream);
int vad_stream_noise_load_i16(const vad_mfcc_plan* plan, const int16_t* frames, int64_t stream_stride,
                              int64_t frame_stride, int32_t frame_len, int32_t n, int64_t n_streams,
                              float* noise_rows, int32_t* noise_count, float* noise_est, float alpha, void* stream);
/* Sessions: streams that join, leave and stall inside the hop kernel.  The
 * entries above advance every stream by n_hops hops; these read, per stream
 * and launch, two more device arrays (a stream is one wave, so both are scalar
 * in it):
 *   hop_counts (S) int32   the hops stream s takes in this launch,
 *                          n_s = min(max(hop_counts[s], 0), n_hops): rows
 *                          0..n_s-1 of its column of the hop block; rows from
 *                          n_s on are not read
 *   restart    (S) uint8   nonzero: before its hops the stream's state becomes
 *                          a fresh stream's -- frame, ring and count zero, and
 *                          with denoising its spec_ring, noise_rows,
 *                          noise_count and noise_est too; the kernel then
 *                          stores restart[s] = 0 (the flag is consumed: set it
 *                          once, a graph replay does not restart again)
 * The stream then advances n_s hops exactly as by the entries above: label
 * and score rows 0..n_s-1 hold what they write (255 / NaN during the first
 * five hops after a restart), rows n_s..n_hops-1 hold VAD_LABEL_NO_HOP and NaN.
 * With n_s = 0 and no restart no byte of the stream's state is written.  With
 * all counts n_hops and no restart, labels, scores and state are those of the
 * entries above, bit for bit.
 * Arguments: those of the denoising entry of the same classifier and input
 * type -- scores may be null; the four state arrays are either all set, or
 * all null for no denoising (alpha, noise_class and update are then not read)
 * -- then hop_counts and restart.  Row 0 of every stream's column of the hop
 * block is loaded whatever its count (and dropped), so the whole block must be
 * readable, as for the entries above.
 * Refusals (VAD_EINVAL, before any device call): a null hop_counts or restart;
 * a partly set denoise state; everything the denoising entries refuse (without
 * denoising: everything the scored entries refuse, a null `scores` excepted). */
#define VAD_LABEL_NO_HOP 254 /* a label row the stream has no hop in */
int vad_stream_hops_sessions(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames, int64_t frame_stride,
                             int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len,
                             int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count,
                             uint8_t* labels, int64_t label_block_stride, int32_t active, float* scores,
                             int64_t score_block_stride, float* spec_ring, float* noise_rows, int32_t* noise_count,
                             float* noise_est, float alpha, int32_t noise_class, int32_t update,
                             const int32_t* hop_counts, uint8_t* restart, void* stream);
int vad_stream_hops_sessions_i16(const vad_mfcc_plan* plan, const vad_ffn_plan* ffn, float* frames,
                                 int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                                 int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                 float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                 int32_t active, float* scores, int64_t score_block_stride, float* spec_ring,
                                 float* noise_rows, int32_t* noise_count, float* noise_est, float alpha,
                                 int32_t noise_class, int32_t update, const int32_t* hop_counts, uint8_t* restart,
                                 void* stream);
int vad_stream_hops_tree_sessions(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                  int64_t frame_stride, int32_t frame_len, const float* hop, int64_t hop_stride,
                                  int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                  float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                  int32_t walk, int32_t active, float* scores, int64_t score_block_stride,
                                  float* spec_ring, float* noise_rows, int32_t* noise_count, float* noise_est,
                                  float alpha, int32_t noise_class, int32_t update, const int32_t* hop_counts,
                                  uint8_t* restart, void* stream);
int vad_stream_hops_tree_sessions_i16(const vad_mfcc_plan* plan, const vad_tree_plan* tree, float* frames,
                                      int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                                      int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                                      float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                                      int32_t walk, int32_t active, float* scores, int64_t score_block_stride,
                                      float* spec_ring, float* noise_rows, int32_t* noise_count, float* noise_est,
                                      float alpha, int32_t noise_class, int32_t update, const int32_t* hop_counts,
                                      uint8_t* restart, void* stream);
/* Hops labelled and scored by a random forest (vad_forest above), in the hop
 * kernel: one wave per stream, lane l walking tree l (trees 64.. in further
 * passes), then the ordered double average of vad_features_forest -- K sums
 * from 0, tree 0 .. T-1 in order, divided by (double)T.  labels[k *
 * label_block_stride + s] is the first maximum (a class index), scores[k *
 * score_block_stride + s] (when `scores` is not NULL) the fp32 share of class
 * `active`: what vad_features_forest gives for the same MFCC rows, bit for
 * bit.  255 / NaN during a stream's first five hops.  Frames, ring and count
 * advance as by every other hop entry.
 * Arguments: vad_stream_hops_tree_sessions', with the forest in place of the
 * tree plan.  Nullable: scores; the four denoise arrays (all or none: none =
 * no denoising, and alpha, noise_class, update are not read); hop_counts and
 * restart (both or neither: neither = every stream takes n_hops hops).  With
 * denoising the noise_class test uses the forest's label.
 * `walk`: VAD_TREE_WALK_AUTO stages the compact nodes of the longest prefix of
 * whole trees that fits in LDS beside the hop tables and one wave's scratch
 * (vad_stream_forest_lds_trees of them) and walks the other trees from the
 * global table; VAD_TREE_WALK_GLOBAL stages none.  Same labels and scores.
 * Refusals (VAD_EINVAL, before any device call): a null plan, forest, frames,
 * hop, ring, count or labels; forest n_features > 3 * mfcc_n; active outside
 * 0 .. n_classes-1 (with or without scores); any other `walk`; the strides and
 * overlap rules of the tree entries; a partly set denoise state, alpha outside
 * [0, 1), update other than 0 / 1, noise_class outside 0 .. n_classes-1;
 * hop_counts without restart or the reverse.
 *   vad_stream_hop_forest_table_bytes  the bytes a launch stages per block
 *                                      (for vad_stream_hop_block_waves);
 *   vad_stream_forest_lds_trees        the leading trees an AUTO launch stages;
 * both VAD_EINVAL for a null or table-less plan or a null forest. */
int vad_stream_hops_forest(const vad_mfcc_plan* plan, const vad_forest* forest, float* frames, int64_t frame_stride,
                           int32_t frame_len, const float* hop, int64_t hop_stride, int32_t hop_len,
                           int64_t n_streams, int32_t n_hops, int64_t hop_block_stride, float* ring, int32_t* count,
                           uint8_t* labels, int64_t label_block_stride, int32_t walk, int32_t active, float* scores,
                           int64_t score_block_stride, float* spec_ring, float* noise_rows, int32_t* noise_count,
                           float* noise_est, float alpha, int32_t noise_class, int32_t update,
                           const int32_t* hop_counts, uint8_t* restart, void* stream);
int vad_stream_hops_forest_i16(const vad_mfcc_plan* plan, const vad_forest* forest, float* frames,
                               int64_t frame_stride, int32_t frame_len, const int16_t* hop, int64_t hop_stride,
                               int32_t hop_len, int64_t n_streams, int32_t n_hops, int64_t hop_block_stride,
                               float* ring, int32_t* count, uint8_t* labels, int64_t label_block_stride,
                               int32_t walk, int32_t active, float* scores, int64_t score_block_stride,
                               float* spec_ring, float* noise_rows, int32_t* noise_count, float* noise_est,
                               float alpha, int32_t noise_class, int32_t update, const int32_t* hop_counts,
                               uint8_t* restart, void* stream);
int64_t vad_stream_hop_forest_table_bytes(const vad_mfcc_plan* plan, const vad_forest* forest, int32_t walk);
int32_t vad_stream_forest_lds_trees(const vad_mfcc_plan* plan, const vad_forest* forest);
/* Replay a captured hipGraph (hipGraphExec_t) on `stream`: the per-hop step
 * of a StreamBatch captured with its host I/O (the H2D copy of every
 * stream's new samples from pinned memory, the hop kernel, the D2H copy of
 * the labels -- vad.py:32-59's loop body for S streams).  The capture itself
 * is the host's (hipStreamBeginCapture / torch.cuda.graph); this entry only
 * launches, so a host replays without a runtime wrapper in between. */
int vad_graph_launch(void* graph_exec, void* stream);
/* The same replay, prepared once from the captured hipGraph_t and its
 * hipGraphExec_t (StreamBatch.capture keeps both; the graph must outlive the
 * plan): a graph of exactly one kernel node -- the one-hop step -- is
 * dispatched as that node (its captured function, grid, block, dynamic LDS
 * and argument values), whose host cost is a kernel launch's rather than
 * hipGraphLaunch's (~5 us more per call on ROCm 7.2); any other graph goes
 * through hipGraphLaunch.  vad_graph_plan_direct says which (1: the node). */
typedef struct vad_graph_plan vad_graph_plan;
int vad_graph_plan_create(void* graph, void* graph_exec, vad_graph_plan** out);
int vad_graph_plan_launch(const vad_graph_plan* plan, void* stream);
int32_t vad_graph_plan_direct(const vad_graph_plan* plan);
int vad_graph_plan_destroy(vad_graph_plan* plan);

/* ---------------------------------------------------------------------------
 * Speech segments and voiced audio from clip labels: what vad.py:52-57,67-72
 * does on the host with the frames the analyser returned as active
 * (active_frames += np_frame.tobytes(), written out as a wav), here on the
 * device, from the per-window labels of the clip path.
 *   a[i] = (labels[i] == active), i < n; window i stands for frame i + 2, the
 *   samples [(i+2)*hop, (i+2)*hop + frame_size) (Row i above;
 *   sklearn_analyser.py:19,52,77).
 *   close(g): every maximal run of a == 0 of length <= g with an active
 *     window on both sides becomes 1 (a run touching an end never closes);
 *   open(m): every maximal run of a == 1 shorter than m becomes 0 (runs at
 *     the ends included);
 *   smooth(max_gap, min_run) = close(max_gap), then open(min_run); both in
 *     windows, 0 = off, any value works.
 * The scans run on tiles of VAD_SEG_TILE labels; one pass of the tile-total
 * scan covers VAD_SEG_CARRY_PASS tiles (more tiles: more passes of its one
 * workgroup).  `ws` is a device workspace of >= vad_segments_workspace_bytes(n)
 * bytes, 16-byte aligned (may be NULL for n == 0).
 * ------------------------------------------------------------------------- */
#define VAD_SEG_TILE 1024
#define VAD_SEG_CARRY_PASS 256
size_t vad_segments_workspace_bytes(int64_t n_labels);

/* out[i] = smooth(max_gap, min_run)(a)[i] as uint8 0 / 1.  out must not
 * overlap labels (VAD_EINVAL). */
int vad_label_smooth(const uint8_t* labels, int64_t n, int32_t active, int64_t max_gap, int64_t min_run,
                     uint8_t* out, void* ws, size_t ws_bytes, void* stream);

/* Segments in samples.  After smooth(max_gap, min_run), close(frame_size /
 * hop - 1) joins runs whose frame ranges overlap or touch; each remaining run
 * [i0, i1] is row k of `segments`, three int64:
 *   start = (i0+2)*hop, end = min((i1+2)*hop + frame_size, n_samples),
 *   offset = sum of end - start over the rows before it (its place in the
 *   packed output of vad_gather_segments_*).
 * Rows are ascending, disjoint and non-touching.  counts[0] = rows found,
 * counts[1] = voiced samples of all rows found; only the first `capacity`
 * rows are written.  VAD_EINVAL unless 0 < hop <= frame_size and
 * n <= vad_n_frames(n_samples, frame_size, hop) - 5. */
int vad_label_segments(const uint8_t* labels, int64_t n, int32_t active, int64_t max_gap, int64_t min_run,
                       int32_t frame_size, int32_t hop, int64_t n_samples,
                       int64_t* segments /* capacity x 3 */, int64_t capacity, int64_t* counts /* 2 */,
                       void* ws, size_t ws_bytes, void* stream);

/* out = the concatenation of audio[start_k : end_k] over the rows written
 * (min(counts[0], capacity) of them), bits copied; writing stops at
 * out_capacity elements and nothing past the voiced count is touched.  out
 * must not overlap audio. */
int vad_gather_segments_f32(const float* audio, int64_t n_samples, const int64_t* segments, const int64_t* counts,
                            int64_t capacity, float* out, int64_t out_capacity, void* stream);
int vad_gather_segments_i16(const int16_t* audio, int64_t n_samples, const int64_t* segments, const int64_t* counts,
                            int64_t capacity, int16_t* out, int64_t out_capacity, void* stream);

/* The form vad.py itself writes: out[r*frame_size + t] = audio[(i_r+2)*hop + t]
 * for the r-th window with labels[i] == active (overlapping samples repeat,
 * as the reference's byte concatenation repeats them).  Any hop > 0 (hop ==
 * frame_size: the recorder's framing); the last window's frame must end
 * inside the clip.  *count = windows found; rows >= out_capacity_frames are
 * not written. */
int vad_gather_active_frames_f32(const float* audio, int64_t n_samples, const uint8_t* labels, int64_t n,
                                 int32_t active, int32_t frame_size, int32_t hop, float* out,
                                 int64_t out_capacity_frames, int64_t* count, void* ws, size_t ws_bytes,
                                 void* stream);
int vad_gather_active_frames_i16(const int16_t* audio, int64_t n_samples, const uint8_t* labels, int64_t n,
                                 int32_t active, int32_t frame_size, int32_t hop, int16_t* out,
                                 int64_t out_capacity_frames, int64_t* count, void* ws, size_t ws_bytes,
                                 void* stream);

/* ---------------------------------------------------------------------------
 * Clip batches: many finished clips of different lengths in one call
 * (dataset_creator.py:58-71 takes FILES_PER_STEP files at a time; a server
 * runs vad.py:52-72 over a queue of utterances).  The clips are packed into
 * one buffer on the hop grid and the clip entries above run ONCE over it:
 *   clip k (len[k] samples) starts at sample start[k] = hop * frame0[k] and
 *   occupies ceil(len[k] / hop) hop slots, start[k+1] = start[k] + hop *
 *   ceil(len[k] / hop); the tail of its last slot is zero.  Frame i of clip
 *   k is then frame frame0[k] + i of the packed buffer and window (row) i of
 *   clip k, i < n_rows[k] = max(vad_n_frames(len[k]) - 5, 0), is window
 *   frame0[k] + i.  Frames that straddle two clips are junk: nothing reads
 *   their rows.  row0[k] = sum of n_rows before k (rows packed clip after
 *   clip).
 * All tables are int64 arrays of n_clips entries in device memory.  Their
 * CONTENT is the caller's contract (frame0 non-decreasing, ranges disjoint);
 * whatever they hold, no entry reads or writes outside the arrays it is
 * given, the sources of vad_batch_pack_* excepted (those addresses are read
 * as given).
 *
 * vad_batch_pack_*: dst[start[k] + i] = (clip k)[i], i < lens[k]; every other
 * element of dst[0 .. total) = 0.  src_ptrs[k] is the device address of clip
 * k's first sample as an int64 (aligned to the sample size, otherwise
 * arbitrary); bits are copied.  dst must be 16-byte aligned.  One kernel
 * launch whatever n_clips.
 *
 * vad_batch_compact_rows: out[row0[k] + i] = rows[frame0[k] + i] for i <
 * n_rows[k], rows of row_bytes bytes (feature rows: 12 * mfcc_n; labels: 1);
 * rows has n_rows_in rows, out n_rows_out = sum of n_rows.  out must be
 * 16-byte aligned and must not overlap rows.
 * ------------------------------------------------------------------------- */
int vad_batch_pack_f32(const int64_t* src_ptrs, const int64_t* lens, const int64_t* start, int64_t n_clips,
                       float* dst, int64_t total, void* stream);
int vad_batch_pack_i16(const int64_t* src_ptrs, const int64_t* lens, const int64_t* start, int64_t n_clips,
                       int16_t* dst, int64_t total, void* stream);
int vad_batch_compact_rows(const void* rows, int64_t n_rows_in, int64_t row_bytes, const int64_t* frame0,
                           const int64_t* n_rows, const int64_t* row0, int64_t n_clips, void* out,
                           int64_t n_rows_out, void* stream);

/* Smoothing and segments over the global window array (n labels) of a batch.
 *   a[w] = (labels[w] == active) if frame0[k] <= w < frame0[k] + n_rows[k] for
 *   some k, else 0: a window of no clip is never active and never emitted.
 * close / open / smooth are those of "Speech segments", applied to every
 * clip's own range as if it were a whole sequence: a run that touches a
 * clip's first or last window touches an end; no gap closes and no run is
 * measured across a clip boundary.
 * vad_batch_label_smooth: out[w] = smooth(max_gap, min_run)(a)[w], 0 / 1.
 * vad_batch_label_segments: after smooth, close(frame_size / hop - 1) per
 * clip; each remaining run [i0, i1] of clip k (clip-local windows) is a row of
 * clip_segments, four int64:
 *   k, start = (i0+2)*hop, end = min((i1+2)*hop + frame_size, len[k]) in the
 *   clip's own samples, offset = sum of end - start over the rows before it;
 * rows ordered by clip, then start.  packed_segments holds the same rows as
 * three int64 (hop*frame0[k] + start, hop*frame0[k] + end, offset): the table
 * vad_gather_segments_* takes with the packed buffer as its audio.
 * counts[0] = rows found, counts[1] = voiced samples of all rows found; only
 * the first `capacity` rows of either table are written.  Per clip (n_clips
 * entries each): clip_rows[k] rows, the first of them row clip_row0[k] (the
 * exclusive prefix of clip_rows), clip_voiced[k] samples.
 * `ws`: >= vad_batch_segments_workspace_bytes(n, n_clips) bytes, 16-byte
 * aligned.  VAD_EINVAL: a null table with n_clips > 0, hop outside
 * (0, frame_size], a negative size, an output overlapping the labels, a
 * workspace that is too small.  The scans run on tiles of VAD_SEG_TILE
 * labels, in a fixed chain of launches.
 * ------------------------------------------------------------------------- */
size_t vad_batch_segments_workspace_bytes(int64_t n_labels, int64_t n_clips);
int vad_batch_label_smooth(const uint8_t* labels, int64_t n, const int64_t* frame0, const int64_t* n_rows,
                           int64_t n_clips, int32_t active, int64_t max_gap, int64_t min_run, uint8_t* out, void* ws,
                           size_t ws_bytes, void* stream);
int vad_batch_label_segments(const uint8_t* labels, int64_t n, const int64_t* frame0, const int64_t* n_rows,
                             const int64_t* len, int64_t n_clips, int32_t active, int64_t max_gap, int64_t min_run,
                             int32_t frame_size, int32_t hop, int64_t* clip_segments /* capacity x 4 */,
                             int64_t* packed_segments /* capacity x 3 */, int64_t capacity, int64_t* counts /* 2 */,
                             int64_t* clip_rows, int64_t* clip_row0, int64_t* clip_voiced, void* ws, size_t ws_bytes,
                             void* stream);

/* ---------------------------------------------------------------------------
 * Speech scores: an operating point for the classifiers.  Every entry above
 * ends in a hard label; here a window gets a score s[i], an fp32 value in
 * [0, 1] that estimates how likely window i is of class `active`, and labels
 * are decided from the scores with an onset and an offset threshold, padded,
 * and scored against a reference.  Nothing here changes what the entries above
 * compute.  All pointers are device memory; no entry synchronises.
 *
 * Scores
 *   vad_scores_from_logits: from the logits vad_features_ffn_logits writes
 *     (n rows of n_classes <= VAD_SCORE_MAX_CLASSES floats),
 *       s = 1 / (1 + sum over j != active of expf(z_j - z_active)),
 *     every operation in fp32; a row with any non-finite logit scores 0.
 *     scores must not overlap logits.
 *   vad_features_tree_scores / vad_tree_predict_scores: the walks of
 *     vad_features_tree / vad_tree_predict (same features, same comparison,
 *     same leaf), writing node_score[leaf node] in place of the leaf's class.
 *     node_score: one float per node of the plan, in the plan's node order
 *     (for sklearn's predict_proba: value[node][active] / sum(value[node])).
 *
 * Decisions (uint8 0 / 1; the segment entries take them with active = 1)
 *   vad_score_labels (hysteresis): h[-1] = 0 and
 *       h[i] = 1 if s[i] >= on;  h[i] = 0 if s[i] < off or s[i] is NaN;
 *       h[i] = h[i-1] otherwise.
 *     0 <= off <= on <= 1, else VAD_EINVAL (NaN thresholds too).
 *   vad_label_dilate (padding): out[i] = 1 iff labels[j] == active for some j
 *     in [i - pad_after, i + pad_before] inside the array: every active run
 *     grows by pad_before windows at its start and pad_after at its end.
 *     Any pad >= 0.
 *   vad_batch_score_labels / vad_batch_label_dilate: the same over the global
 *     window array of a clip batch ("Clip batches"), every clip's range a
 *     sequence of its own: h is 0 before a clip's first window, padding stops
 *     at a clip's first and last window, a window of no clip is 0.
 *   out must not overlap the input.  `ws`: >= vad_scores_workspace_bytes(n)
 *   bytes, 16-byte aligned, overlapping neither array (NULL for n == 0).  Each
 *   is a fixed chain of three launches over tiles of VAD_SEG_TILE windows.
 *
 * Scoring against a reference
 *   vad_reference_labels: `intervals` holds n_intervals rows (start, end) of
 *     int64, speech [start, end) in samples, ascending and disjoint.  Window i
 *     (frame i + 2) has the centre sample c = (i+2)*hop + frame_size/2 (integer
 *     division); out[i] = 1 iff start <= c < end for some row.
 *   vad_batch_reference_labels: rows (clip, start, end) in the clip's own
 *     samples, ordered by clip, then start; clip k's rows are
 *     [clip_row0[k], clip_row0[k+1]) (the last clip's: up to n_intervals), its
 *     windows frame0[k] + i, i < n_rows[k]; a window of no clip is 0.
 *   vad_score_histogram_f32: hist[r*bins + b] += the windows with ref[i] == r
 *     (r = 0, 1; any other ref is not counted) and
 *       b = min((int)(s[i] * bins), bins - 1) (the product in fp32; a NaN or
 *       negative product: bin 0),  1 <= bins <= VAD_SCORE_MAX_BINS.
 *     hist: 2 * bins int64, ZEROED BY THE CALLER (counts are added); the result
 *     does not depend on the order of the additions.
 *   vad_score_histogram_u8: the same with b = labels[i] (a label >= n_values
 *     is not counted), n_values <= 256: the confusion matrix.
 * ------------------------------------------------------------------------- */
#define VAD_SCORE_MAX_CLASSES 8
#define VAD_SCORE_MAX_BINS 4096
int vad_scores_from_logits(const float* logits, int64_t n, int32_t n_classes, int32_t active, float* scores,
                           void* stream);
int vad_features_tree_scores(const vad_tree_plan* tree, const float* node_score, const float* mfcc, int64_t n_frames,
                             int32_t mfcc_n, int32_t mode, float* scores /* n_frames - 5 */, void* stream);
int vad_tree_predict_scores(const vad_tree_plan* tree, const float* node_score, const float* x, int64_t n,
                            float* scores, void* stream);
size_t vad_scores_workspace_bytes(int64_t n);
int vad_score_labels(const float* scores, int64_t n, float on, float off, uint8_t* out, void* ws, size_t ws_bytes,
                     void* stream);
int vad_label_dilate(const uint8_t* labels, int64_t n, int32_t active, int64_t pad_before, int64_t pad_after,
                     uint8_t* out, void* ws, size_t ws_bytes, void* stream);
int vad_batch_score_labels(const float* scores, int64_t n, const int64_t* frame0, const int64_t* n_rows,
                           int64_t n_clips, float on, float off, uint8_t* out, void* ws, size_t ws_bytes,
                           void* stream);
int vad_batch_label_dilate(const uint8_t* labels, int64_t n, const int64_t* frame0, const int64_t* n_rows,
                           int64_t n_clips, int32_t active, int64_t pad_before, int64_t pad_after, uint8_t* out,
                           void* ws, size_t ws_bytes, void* stream);
int vad_reference_labels(const int64_t* intervals /* n_intervals x 2 */, int64_t n_intervals, int64_t n,
                         int32_t frame_size, int32_t hop, uint8_t* out, void* stream);
int vad_batch_reference_labels(const int64_t* intervals /* n_intervals x 3 */, int64_t n_intervals,
                               const int64_t* clip_row0, const int64_t* frame0, const int64_t* n_rows,
                               int64_t n_clips, int64_t n, int32_t frame_size, int32_t hop, uint8_t* out,
                               void* stream);
int vad_score_histogram_f32(const float* scores, const uint8_t* ref, int64_t n, int32_t bins,
                            int64_t* hist /* 2 x bins */, void* stream);
int vad_score_histogram_u8(const uint8_t* labels, const uint8_t* ref, int64_t n, int32_t n_values,
                           int64_t* hist /* 2 x n_values */, void* stream);

/* ---------------------------------------------------------------------------
 * Streaming segments: the same segments and voiced samples, online, for the
 * S streams of the hop kernels above (vad.py:32-59 keeps the samples of the
 * active frames while it feeds them).  Per stream the entries consume the
 * label blocks vad_stream_hops writes and, optionally, the same hop sample
 * blocks; with a fixed delay they append finished segments to a per-stream
 * table and emit the voiced samples.  One kernel per call, one wave per
 * stream; capturable after the hop kernel on the same stream, no host step.
 *
 * Equivalent clip of a stream (L = frame_size, H = hop, 0 < H <= L): the
 *   L - H carried samples (zeros, or what the host carried over) followed by
 *   every hop pushed since; T hops make L - H + T*H samples, hop t (0-based)
 *   sits at [L-H + t*H, L-H + (t+1)*H).  The label byte of hop t >= 5 is
 *   window t - 5 of that clip (any byte != active is inactive); the label
 *   bytes of hops t < 5 are ignored, whatever they hold.
 * Final mask: c = close(j)(open(min_run)(close(max_gap)(a))), j = L / H - 1,
 *   the mask whose runs vad_label_segments turns into rows.  Its rules at the
 *   end of a sequence equal "inactive windows follow forever", so a stream
 *   cut off anywhere and flushed gives the offline result on its labels.
 * Delay: D = max_gap + max(min_run, 1) + j + 1 windows (vad_stream_seg_delay;
 *   -1 for bad arguments: hop outside (0, frame_size], a negative value, or
 *   max_gap / min_run above 2^29).  c[i] is the same for every continuation
 *   once the labels up to window i + D are known.
 * Hop t decides window d = t - 5 - D (nothing while d < 0) and the slab
 *   [(d+2)H, (d+3)H) of the clip.  Every segment starts on a multiple of H,
 *   so the voiced part of a slab is a prefix, of length
 *   clamp((e+2)H + L - (d+2)H, 0, H) with e the last window <= d with c = 1
 *   (0 when there is none).  Row (k, s) of `voiced` gets that prefix of hop k
 *   of the block, copied bit for bit from the stream's samples, and
 *   voiced_len[k, s] its length; elements past the prefix are not touched.
 *   The prefixes of a stream, in order, are its packed voiced audio.
 * Segments: a run [i0, i1] of c is appended by the hop whose d is i1 + 1
 *   (the run is complete, the window after it decided and inactive), as the
 *   int64 pair start = (i0+2)H, end = (i1+2)H + L (inside the clip: the last
 *   window's frame ends in it).  found[s] counts every segment appended;
 *   only the first `capacity` rows of stream s are written; rows ascend.
 * State: vad_stream_seg_state_bytes(S) bytes, 8-byte aligned; ALL ZERO is a
 *   stream before its first hop, with found[s] = 0 (and a zeroed history
 *   slice when no carry is wanted).  The caller passes the same max_gap,
 *   min_run, frame_size, hop, history and history_elems on every call.
 * History: the entries with audio keep their own copy of the samples (the
 *   caller's hop blocks are recycled) in `history`, history_elems elements of
 *   the sample type, stream s owning [s*R, (s+1)*R), R = history_elems / S >=
 *   (D+3)H + L + n_hops*H (vad_stream_seg_history_elems gives S times that
 *   for the largest block; R <= 2^30).  Clip position p lives at index
 *   (p - (L-H)) mod R of the slice, so the carried samples, when they matter
 *   (L > 3H: positions in [2H, L-H) can be voiced), go to its last L - H
 *   elements before the first hop.
 * Flush: vad_stream_seg_flush_rows = D + 2 + ceil(L / H) more hops of
 *   inactive windows without samples: every window is decided, the open
 *   segment is appended, the remaining prefixes are emitted (F rows of
 *   voiced / voiced_len; positions past the clip's end are never voiced).
 *   After it every stream of the call equals vad_label_segments /
 *   vad_gather_segments_* on its equivalent clip.  CONTRACT: a flushed state
 *   is ended -- further hops and flushes emit empty rows and change nothing
 *   -- until the host zeroes it (state slice, found[s], and the history slice
 *   or its carry): zeroing one stream's slices restarts that stream alone,
 *   together with its ring / count of the hop kernel.
 * VAD_EINVAL: hop outside (0, frame_size]; a negative max_gap, min_run,
 *   capacity, n_streams or n_hops; active outside [0, 255) (255 is the "no
 *   label yet" byte); a NULL pointer that would be used; n_hops > 1 with
 *   label_block_stride < n_streams; hop_stride < hop, or hop rows refused by
 *   vad_stream_hops (the same layouts are read in place, any element
 *   offset); a history too small (or R > 2^30); misaligned pointers.
 *   n_streams == 0 or n_hops == 0: nothing is done, VAD_OK.
 * ------------------------------------------------------------------------- */
int64_t vad_stream_seg_delay(int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop);
int64_t vad_stream_seg_flush_rows(int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop);
size_t vad_stream_seg_state_bytes(int64_t n_streams);
int64_t vad_stream_seg_history_elems(int64_t n_streams, int32_t n_hops_max, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop);
/* Events only: segments and found, no audio, no history. */
int vad_stream_segments(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams, int32_t n_hops,
                        int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                        void* state, int64_t* segments /* S x capacity x 2 */, int64_t capacity,
                        int64_t* found /* S */, void* stream);
/* The same plus the hop block vad_stream_hops / _i16 read (hop k's row s at
 * hop_samples + k * hop_block_stride + s * hop_stride) and the voiced rows. */
int vad_stream_segments_f32(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams, int32_t n_hops,
                            int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                            void* state, int64_t* segments, int64_t capacity, int64_t* found,
                            const float* hop_samples, int64_t hop_stride, int64_t hop_block_stride, float* history,
                            int64_t history_elems, float* voiced /* n_hops x S x hop */,
                            int32_t* voiced_len /* n_hops x S */, void* stream);
int vad_stream_segments_i16(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams, int32_t n_hops,
                            int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                            void* state, int64_t* segments, int64_t capacity, int64_t* found,
                            const int16_t* hop_samples, int64_t hop_stride, int64_t hop_block_stride,
                            int16_t* history, int64_t history_elems, int16_t* voiced, int32_t* voiced_len,
                            void* stream);
/* Flush (see above); voiced is F x S x hop, voiced_len F x S, F = vad_stream_seg_flush_rows. */
int vad_stream_segments_flush(int64_t n_streams, int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                              void* state, int64_t* segments, int64_t capacity, int64_t* found, void* stream);
int vad_stream_segments_flush_f32(int64_t n_streams, int64_t max_gap, int64_t min_run, int32_t frame_size,
                                  int32_t hop, void* state, int64_t* segments, int64_t capacity, int64_t* found,
                                  float* history, int64_t history_elems, float* voiced, int32_t* voiced_len,
                                  void* stream);
int vad_stream_segments_flush_i16(int64_t n_streams, int64_t max_gap, int64_t min_run, int32_t frame_size,
                                  int32_t hop, void* state, int64_t* segments, int64_t capacity, int64_t* found,
                                  int16_t* history, int64_t history_elems, int16_t* voiced, int32_t* voiced_len,
                                  void* stream);

/* The operating point in the streaming segmenter: the clip chain of "Speech
 * scores" (hysteresis -> smooth -> dilate -> segments) one window at a time.
 * `block` is the (n_hops, n_streams) block the hop kernels wrote, row stride
 * block_stride elements: fp32 scores (block_is_scores 1) or uint8 labels (0).
 *   hysteresis  scores only: h = 1 at s >= on, 0 at s < off or NaN, else the
 *               previous h (0 before a stream's first window); the window is
 *               active iff h.  `active` is not read.  Labels: active iff
 *               label == active, as vad_stream_segments.
 *   padding     a run [r0, r1] that survives close(max_gap) and open(min_run)
 *               becomes [max(r0 - pad_before, 0), min(r1 + pad_after, N - 1)],
 *               N the stream's window count (known at the flush), before the
 *               close(frame_size / hop - 1) join: vad_label_dilate's result.
 *   delay       D = vad_stream_seg_delay_pad = vad_stream_seg_delay +
 *               pad_before; pad_after adds none.  The flush row count and the
 *               history grow with D (the _pad sizing entries; each equals the
 *               entry without _pad at pads (0, 0)).
 * After the flush a stream's rows and voiced samples are vad_label_segments /
 * vad_gather_segments of vad_label_dilate(vad_label_smooth(vad_score_labels(
 * scores))) on its equivalent clip, bit for bit.  State, history, segments,
 * found and the voiced rows are those of vad_stream_segments*; the state's
 * size does not change and all-zero is still a stream before its first hop.
 * One kernel, no LDS, no atomics, no workgroup waits on another.
 * Refusals: those of vad_stream_segments*, plus VAD_EINVAL for on / off outside
 * [0, 1], off > on or a NaN threshold, a negative pad (or one above 2^29), a
 * block_is_scores other than 0 / 1, a score block that is not 4-byte aligned,
 * and a history that would pass 2^30 elements per stream.  The flush forms
 * take and check the same operating point. */
int64_t vad_stream_seg_delay_pad(int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                                 int64_t pad_before, int64_t pad_after);
int64_t vad_stream_seg_flush_rows_pad(int64_t max_gap, int64_t min_run, int32_t frame_size, int32_t hop,
                                      int64_t pad_before, int64_t pad_after);
int64_t vad_stream_seg_history_elems_pad(int64_t n_streams, int32_t n_hops_max, int64_t max_gap, int64_t min_run,
                                         int32_t frame_size, int32_t hop, int64_t pad_before, int64_t pad_after);
int vad_stream_segments_op(const void* block, int32_t block_is_scores, int64_t block_stride, int64_t n_streams,
                           int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size,
                           int32_t hop, float on, float off, int64_t pad_before, int64_t pad_after, void* state,
                           int64_t* segments, int64_t capacity, int64_t* found, void* stream);
int vad_stream_segments_op_f32(const void* block, int32_t block_is_scores, int64_t block_stride, int64_t n_streams,
                               int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size,
                               int32_t hop, float on, float off, int64_t pad_before, int64_t pad_after, void* state,
                               int64_t* segments, int64_t capacity, int64_t* found, const float* hop_samples,
                               int64_t hop_stride, int64_t hop_block_stride, float* history, int64_t history_elems,
                               float* voiced, int32_t* voiced_len, void* stream);
int vad_stream_segments_op_i16(const void* block, int32_t block_is_scores, int64_t block_stride, int64_t n_streams,
                               int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run, int32_t frame_size,
                               int32_t hop, float on, float off, int64_t pad_before, int64_t pad_after, void* state,
                               int64_t* segments, int64_t capacity, int64_t* found, const int16_t* hop_samples,
                               int64_t hop_stride, int64_t hop_block_stride, int16_t* history, int64_t history_elems,
                               int16_t* voiced, int32_t* voiced_len, void* stream);
int vad_stream_segments_op_flush(int64_t n_streams, int32_t block_is_scores, int64_t max_gap, int64_t min_run,
                                 int32_t frame_size, int32_t hop, float on, float off, int64_t pad_before,
                                 int64_t pad_after, void* state, int64_t* segments, int64_t capacity, int64_t* found,
                                 void* stream);
int vad_stream_segments_op_flush_f32(int64_t n_streams, int32_t block_is_scores, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop, float on, float off, int64_t pad_before,
                                     int64_t pad_after, void* state, int64_t* segments, int64_t capacity,
                                     int64_t* found, float* history, int64_t history_elems, float* voiced,
                                     int32_t* voiced_len, void* stream);
int vad_stream_segments_op_flush_i16(int64_t n_streams, int32_t block_is_scores, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop, float on, float off, int64_t pad_before,
                                     int64_t pad_after, void* state, int64_t* segments, int64_t capacity,
                                     int64_t* found, int16_t* history, int64_t history_elems, int16_t* voiced,
                                     int32_t* voiced_len, void* stream);

/* Sessions in the streaming segmenter: the push entries above for the label
 * (or score) and hop blocks of vad_stream_hops_sessions*, where streams join,
 * leave and stall inside one launch.  Still one kernel, one wave per stream,
 * no atomics, no barrier, no wave waits on another.  The flush entries above
 * serve a sessions state unchanged (they end every stream).
 *   hop counts  hop_counts (S) int32 and restart (S) uint8 are read once per
 *               stream at the start of the launch.  Stream s takes n_s =
 *               min(max(hop_counts[s], 0), n_hops) hops: rows 0..n_s-1 of its
 *               column of the block and of the hop samples, the rows the
 *               sessions hop kernel consumed.  Its clock, history and
 *               decisions advance by n_s.  Rows n_s..n_hops-1 are never read,
 *               whatever they hold; voiced_len[n_s..n_hops-1, s] = 0 and
 *               nothing of `voiced` is written there.  A stream with n_s = 0
 *               and no restart keeps every byte of its state, history slice,
 *               found and table rows; only its voiced_len and end_len rows
 *               are written, as zeros.
 *   restart     restart[s] != 0: the kernel stores 0 back (a flag set once
 *               restarts once, also under graph replay; the flag is the
 *               segmenter's own, the hop kernel has cleared its own by then)
 *               and, before the stream's hops,
 *               1. ends the running session: what the flush entry does, for
 *                  this stream alone -- F = vad_stream_seg_flush_rows(_pad)
 *                  hops of inactive windows without samples, the newest padded
 *                  end stopped at window N - 1, finished rows appended, the
 *                  voiced prefixes to end_voiced (F x S x hop) / end_len
 *                  (F x S).  end_len[:, s] is written for every stream by
 *                  every call, zeros where no session ended (so also for a
 *                  fresh stream, t = 0, and for one a flush entry ended: no
 *                  rows are appended for those).  The events-only entries
 *                  write end_len too: the lengths the prefixes would have;
 *               2. makes the stream fresh: the state as zeroed -- hysteresis
 *                  bit and `ended` included -- but for a session ordinal that
 *                  goes up by one per consumed flag (all zero is still a
 *                  fresh state, ordinal 0; the state's size does not change),
 *                  and the L - H carry positions of its history slice zeroed;
 *               3. then the stream takes its n_s hops.  Sample positions in
 *                  rows, and the equivalent clip, start again at 0.
 *   table       segments and found keep appending across sessions (found
 *               counts past capacity as before); table_session (S x capacity)
 *               int32 gets the session ordinal of every row written.  The
 *               flush entries know no sessions and do not write it: the rows
 *               they append, [found before, found after) of a stream, belong
 *               to its running session (vad_amd.stream_segments files them).
 *   equality    per stream and session, the rows and the concatenation of the
 *               session's voiced prefixes, push rows then end rows, equal a
 *               one-stream vad_stream_segments* pushed with that session's
 *               hops and flushed, bit for bit; with every count n_hops and no
 *               flag, state, history, segments, found, voiced and voiced_len
 *               equal the sibling entry's byte for byte.
 *   history     the sibling's bound R >= (D+3)H + L + n_hops*H still holds:
 *               ending a session appends no samples and comes before the
 *               block's hops are written.
 * Refusals: the sibling's, plus VAD_EINVAL for a NULL hop_counts, restart,
 * end_len, table_session (with capacity > 0) or, in the audio forms,
 * end_voiced, and for one of them misaligned for its type. */
int vad_stream_segments_sessions(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams,
                                 int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run,
                                 int32_t frame_size, int32_t hop, void* state, int64_t* segments, int64_t capacity,
                                 int64_t* found, const int32_t* hop_counts, uint8_t* restart, int32_t* end_len,
                                 int32_t* table_session, void* stream);
int vad_stream_segments_sessions_f32(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams,
                                     int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop, void* state, int64_t* segments,
                                     int64_t capacity, int64_t* found, const float* hop_samples, int64_t hop_stride,
                                     int64_t hop_block_stride, float* history, int64_t history_elems, float* voiced,
                                     int32_t* voiced_len, const int32_t* hop_counts, uint8_t* restart,
                                     float* end_voiced, int32_t* end_len, int32_t* table_session, void* stream);
int vad_stream_segments_sessions_i16(const uint8_t* labels, int64_t label_block_stride, int64_t n_streams,
                                     int32_t n_hops, int32_t active, int64_t max_gap, int64_t min_run,
                                     int32_t frame_size, int32_t hop, void* state, int64_t* segments,
                                     int64_t capacity, int64_t* found, const int16_t* hop_samples,
                                     int64_t hop_stride, int64_t hop_block_stride, int16_t* history,
                                     int64_t history_elems, int16_t* voiced, int32_t* voiced_len,
                                     const int32_t* hop_counts, uint8_t* restart, int16_t* end_voiced,
                                     int32_t* end_len, int32_t* table_session, void* stream);
int vad_stream_segments_op_sessions(const void* block, int32_t block_is_scores, int64_t block_stride,
                                    int64_t n_streams, int32_t n_hops, int32_t active, int64_t max_gap,
                                    int64_t min_run, int32_t frame_size, int32_t hop, float on, float off,
                                    int64_t pad_before, int64_t pad_after, void* state, int64_t* segments,
                                    int64_t capacity, int64_t* found, const int32_t* hop_counts, uint8_t* restart,
                                    int32_t* end_len, int32_t* table_session, void* stream);
int vad_stream_segments_op_sessions_f32(const void* block, int32_t block_is_scores, int64_t block_stride,
                                        int64_t n_streams, int32_t n_hops, int32_t active, int64_t max_gap,
                                        int64_t min_run, int32_t frame_size, int32_t hop, float on, float off,
                                        int64_t pad_before, int64_t pad_after, void* state, int64_t* segments,
                                        int64_t capacity, int64_t* found, const float* hop_samples,
                                        int64_t hop_stride, int64_t hop_block_stride, float* history,
                                        int64_t history_elems, float* voiced, int32_t* voiced_len,
                                        const int32_t* hop_counts, uint8_t* restart, float* end_voiced,
                                        int32_t* end_len, int32_t* table_session, void* stream);
int vad_stream_segments_op_sessions_i16(const void* block, int32_t block_is_scores, int64_t block_stride,
                                        int64_t n_streams, int32_t n_hops, int32_t active, int64_t max_gap,
                                        int64_t min_run, int32_t frame_size, int32_t hop, float on, float off,
                                        int64_t pad_before, int64_t pad_after, void* state, int64_t* segments,
                                        int64_t capacity, int64_t* found, const int16_t* hop_samples,
                                        int64_t hop_stride, int64_t hop_block_stride, int16_t* history,
                                        int64_t history_elems, int16_t* voiced, int32_t* voiced_len,
                                        const int32_t* hop_counts, uint8_t* restart, int16_t* end_voiced,
                                        int32_t* end_len, int32_t* table_session, void* stream);

/* ---------------------------------------------------------------------------
 * Resampling: audio at another rate to the front end's (the mel bank, the
 * 400 / 160 framing and the classifiers assume 16 kHz; the reference has no
 * converter, file_processing.py:27-38 hands the file's samples on as they
 * are).  A polyphase FIR converter for the rational ratio up / down (reduced:
 * gcd 1), with P = 10 * max(up, down) (0 for 1 / 1) and 2P+1 taps h:
 *   n_out = ceil(n * up / down)
 *   y[m]  = sum_j x[j] * h[m * down - j * up + P],   0 <= m < n_out,
 * x zero outside [0, n): scipy.signal.resample_poly(x, up, down) without the
 * group delay when h is its default filter (vad_amd/resample.py builds it).
 * Every output is one fp32 chain x[jmax] * h[r], then fmaf over the T =
 * ceil((2P+1) / up) taps of its phase in falling j: the same bits from every
 * entry below.  int16 output: rint (ties to even) saturated to [-32768,
 * 32767], NaN -> 0.  1 / 1 copies.
 *
 * vad_resample_plan_create: `taps` are 2P+1 floats in HOST memory.
 * VAD_EINVAL: null, up or down <= 0 or not reduced, n_taps != 2P+1, a phase
 * table of up * (T | 1) floats over VAD_RESAMPLE_MAX_TABLE, or an input tile
 * ((VAD_RESAMPLE_TILE - 1) * down / up + T samples) over VAD_RESAMPLE_MAX_SPAN
 * (both live in LDS).  No HIP call: the device copy of the table is made by
 * vad_resample_plan_upload on the current device, or by the first launch (an
 * allocation: upload before capturing a launch into a graph).
 *
 * vad_resample_batch_<in>_<out>: clip k is lens_in[k] samples at the device
 * address src_ptrs[k] (aligned to the sample size, otherwise arbitrary);
 * dst[start[k] + m] = y_k[m] for m < n_out_k, every other element of
 * dst[0 .. total) = 0: with start / total from the clip-batch placement of
 * the OUTPUT lengths, dst is a packed clip buffer and needs no pack step.
 * Tables: int64, n_clips entries, device memory, start non-decreasing (the
 * clip-batch contract: whatever they hold, nothing is written outside
 * dst[0 .. total); a clip that passes `total` or the next clip's start is cut
 * there).  dst must be 16-byte aligned.  One launch whatever n_clips.
 * src_ptrs[k] == 0 leaves dst[start[k] .. start[k+1]) (.. total for the last
 * clip) as it is: a buffer of clips at several input rates is filled by one
 * launch per rate, each with the other rates' addresses zeroed.
 *
 * Streams: a hop of hop_out outputs takes hop_in = hop_out * down / up input
 * samples (VAD_EINVAL when that is no whole number).  With y taken over the
 * stream's whole input and d = vad_resample_delay = ceil(P / down), the
 * stream emits z[n] = y[n - d], z[n] = 0 for n < d.  in: element i of hop k of
 * stream s at in[k * block_stride + s * hop_stride + i], the layouts of
 * vad_stream_hops; out: (n_hops, n_streams, hop_out) contiguous.  state:
 * vad_resample_stream_state_bytes bytes, 4-byte aligned, all zero = a stream
 * before its first sample.  n_hops * hop_in plus the history
 * (ceil((d * down - P) / up) + T - 1 samples) must fit VAD_RESAMPLE_MAX_SPAN.
 * ------------------------------------------------------------------------- */
#define VAD_RESAMPLE_TILE 1024        /* outputs per destination tile */
#define VAD_RESAMPLE_MAX_TABLE 16384  /* floats of the phase table in LDS (64 KiB) */
#define VAD_RESAMPLE_MAX_SPAN 16384   /* floats of the input tile / stream window in LDS (64 KiB) */
typedef struct vad_resample_plan vad_resample_plan;
int32_t vad_resample_tile_outputs(void);
int vad_resample_plan_create(int32_t up, int32_t down, const float* taps, int32_t n_taps, vad_resample_plan** out);
int vad_resample_plan_upload(vad_resample_plan* plan);
int vad_resample_plan_destroy(vad_resample_plan* plan);
int64_t vad_resample_n_out(const vad_resample_plan* plan, int64_t n_in); /* -1: bad argument */
int32_t vad_resample_delay(const vad_resample_plan* plan);
int vad_resample_batch_f32_f32(vad_resample_plan* plan, const int64_t* src_ptrs, const int64_t* lens_in,
                               const int64_t* start, int64_t n_clips, float* dst, int64_t total, void* stream);
int vad_resample_batch_f32_i16(vad_resample_plan* plan, const int64_t* src_ptrs, const int64_t* lens_in,
                               const int64_t* start, int64_t n_clips, int16_t* dst, int64_t total, void* stream);
int vad_resample_batch_i16_f32(vad_resample_plan* plan, const int64_t* src_ptrs, const int64_t* lens_in,
                               const int64_t* start, int64_t n_clips, float* dst, int64_t total, void* stream);
int vad_resample_batch_i16_i16(vad_resample_plan* plan, const int64_t* src_ptrs, const int64_t* lens_in,
                               const int64_t* start, int64_t n_clips, int16_t* dst, int64_t total, void* stream);
size_t vad_resample_stream_state_bytes(const vad_resample_plan* plan, int64_t n_streams);
int vad_resample_stream_f32_f32(vad_resample_plan* plan, const float* in, int64_t hop_stride, int64_t block_stride,
                                int64_t n_streams, int32_t n_hops, int32_t hop_out, void* state, float* out,
                                void* stream);
int vad_resample_stream_f32_i16(vad_resample_plan* plan, const float* in, int64_t hop_stride, int64_t block_stride,
                                int64_t n_streams, int32_t n_hops, int32_t hop_out, void* state, int16_t* out,
                                void* stream);
int vad_resample_stream_i16_f32(vad_resample_plan* plan, const int16_t* in, int64_t hop_stride, int64_t block_stride,
                                int64_t n_streams, int32_t n_hops, int32_t hop_out, void* state, float* out,
                                void* stream);
int vad_resample_stream_i16_i16(vad_resample_plan* plan, const int16_t* in, int64_t hop_stride, int64_t block_stride,
                                int64_t n_streams, int32_t n_hops, int32_t hop_out, void* state, int16_t* out,
                                void* stream);

/* ---------------------------------------------------------------------------
 * Sessions through the stream resampler: the converter in front of
 * vad_stream_hops_sessions, each stream at a rate of its own.  `plans` is a
 * HOST array of n_rates plans (1 .. VAD_RESAMPLE_MAX_RATES, all for the same
 * output rate; each uploaded by vad_resample_plan_upload or by the first
 * launch, as above).  Per stream the kernel reads, at the start of every call,
 *   hop_counts[s]  int32: the stream converts n_s = min(max(count, 0), n_hops)
 *                  hops, rows 0 .. n_s-1 of its column of `in`, into rows
 *                  0 .. n_s-1 of its column of `out`; rows n_s .. n_hops-1 of
 *                  `out` are NOT written (the hop kernel does not read them);
 *   restart[s]     uint8, owned by the resampler: nonzero -> the stream's
 *                  history and emitted count become zero, its rate becomes
 *                  plans[min(max(rate_index[s], 0), n_rates - 1)], and the
 *                  kernel stores 0 back (a flag set once restarts once, also
 *                  under graph replay); only then are its hops converted;
 *   rate_index[s]  int32, read under a nonzero flag only: a running session
 *                  cannot change rate.
 * A stream with n_s = 0 and no flag writes nothing, its state included.  The
 * stream's rate picks the phase table, up, down, T, the history length,
 * hop_in, delay and c_off; each output is the one fp32 chain of the entries
 * above, so a session's rows equal, bit for bit, what vad_resample_stream_*
 * writes for the same plan and input from a zero state (z[n] = 0 for the
 * first `delay` outputs of every session).  in: element i of hop k of stream
 * s at in[k * block_stride + s * hop_stride + i], the layouts of
 * vad_stream_hops with a row as wide as the largest hop_in of the rates (a
 * stream reads the first hop_in(rate) samples of its rows).  out: (n_hops,
 * n_streams, hop_out) contiguous.  state: vad_resample_sessions_state_bytes
 * bytes, 4-byte aligned -- per stream a history padded to the longest of the
 * rates, the emitted count and the rate index; all zero = a fresh stream at
 * plans[0].  One workgroup per stream up to vad_resample_sessions_grid
 * workgroups, which loop over the streams past that; no atomics, no workgroup
 * waits on another.
 * VAD_EINVAL, before any HIP call: plans null or a null plan in it, n_rates
 * outside 1 .. VAD_RESAMPLE_MAX_RATES, a negative count, hop_out <= 0,
 * hop_out * down % up != 0 for any rate, n_hops * hop_in + history over
 * VAD_RESAMPLE_MAX_SPAN for any rate, rows that repeat or overlap; then, with
 * at least one stream and one hop (zero of either succeeds and does nothing):
 * a null pointer, in / out not aligned to their sample size, state /
 * hop_counts / rate_index not 4-byte aligned, or any two of in, out, state,
 * hop_counts, restart, rate_index sharing a byte.
 * ------------------------------------------------------------------------- */
#define VAD_RESAMPLE_MAX_RATES 8
int32_t vad_resample_sessions_grid(void);
size_t vad_resample_sessions_state_bytes(vad_resample_plan* const* plans, int32_t n_rates, int64_t n_streams);
int vad_resample_stream_sessions_f32_f32(vad_resample_plan* const* plans, int32_t n_rates, const float* in,
                                         int64_t hop_stride, int64_t block_stride, int64_t n_streams, int32_t n_hops,
                                         int32_t hop_out, const int32_t* hop_counts, uint8_t* restart,
                                         const int32_t* rate_index, void* state, float* out, void* stream);
int vad_resample_stream_sessions_f32_i16(vad_resample_plan* const* plans, int32_t n_rates, const float* in,
                                         int64_t hop_stride, int64_t block_stride, int64_t n_streams, int32_t n_hops,
                                         int32_t hop_out, const int32_t* hop_counts, uint8_t* restart,
                                         const int32_t* rate_index, void* state, int16_t* out, void* stream);
int vad_resample_stream_sessions_i16_f32(vad_resample_plan* const* plans, int32_t n_rates, const int16_t* in,
                                         int64_t hop_stride, int64_t block_stride, int64_t n_streams, int32_t n_hops,
                                         int32_t hop_out, const int32_t* hop_counts, uint8_t* restart,
                                         const int32_t* rate_index, void* state, float* out, void* stream);
int vad_resample_stream_sessions_i16_i16(vad_resample_plan* const* plans, int32_t n_rates, const int16_t* in,
                                         int64_t hop_stride, int64_t block_stride, int64_t n_streams, int32_t n_hops,
                                         int32_t hop_out, const int32_t* hop_counts, uint8_t* restart,
                                         const int32_t* rate_index, void* state, int16_t* out, void* stream);

/* ---------------------------------------------------------------------------
 * Multi-GPU clip sharding: one process per GPU, each
 * classifying its shard (vad_amd/dist.py split_clip: windows [w_lo, w_hi)
 * from samples [160 w_lo, 160 (w_hi + 4) + 401)), then ONE collective: the
 * gather of the per-window uint8 decisions to the root over RCCL / xGMI.
 * The reference's only parallelism is dataset_creator.py:84's process pool;
 * these entries replace nothing there -- they are the host-agnostic form of
 * vad_amd.dist.LabelGather (torch.distributed "nccl").  RCCL is resolved at
 * run time (the process's loaded copy, else librccl.so.1).
 * ------------------------------------------------------------------------- */
#define VAD_RCCL_ID_BYTES 128
typedef struct vad_rccl_comm vad_rccl_comm;
int vad_rccl_available(void);
const char* vad_rccl_error_string(void);
/* ncclGetUniqueId on the root; the caller ships the 128 bytes to every rank. */
int vad_rccl_unique_id(void* id_out /* VAD_RCCL_ID_BYTES */);
/* ncclCommInitRank on the current HIP device. */
int vad_rccl_init(vad_rccl_comm** out, int32_t nranks, const void* id, int32_t rank);
/* ncclGather of `count` uint8 per rank: recv (root only) = nranks * count,
 * rank r's block at recv + r * count.  Enqueued on `stream`. */
int vad_rccl_gather_u8(vad_rccl_comm* comm, const uint8_t* send, uint8_t* recv, size_t count, int32_t root,
                       void* stream);
int vad_rccl_destroy(vad_rccl_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* VAD_AMD_H */
