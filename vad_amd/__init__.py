"""vad_amd -- MI355X-native MFCC + FFN voice-activity detection.

A from-scratch gfx950 implementation of the hot path of nameofuser1/vad:
framing -> 512-point FFT power spectrum -> mel filterbank -> log10 ->
lifter x DCT-II (mfcc.py), the 5-frame feature window
(realtime_analysis/sklearn_analyser.py, dataset/file_processing.py) and the
Keras FFN forward (learning/ffn_trainer.py), behind the reference's own API:
``vad_amd.mfcc`` mirrors ``mfcc.py`` and ``vad_amd.sklearn_analyser``
mirrors ``realtime_analysis/sklearn_analyser.py``.

The arithmetic runs only in HIP kernels (libvad_amd.so, include/vad_amd.h);
importing a compute entry point without the built library raises.
"""
from .config import MfccConfig  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # SimpleStreamBatch needs torch and the built library: imported on first use
    if name == "SimpleStreamBatch":
        from .simple_stream import SimpleStreamBatch
        return SimpleStreamBatch
    # the forest needs torch: imported on first use
    if name == "ForestClassifier":
        from .forest import ForestClassifier
        return ForestClassifier
    if name == "ForestStreamBatch":
        from .stream import ForestStreamBatch
        return ForestStreamBatch
    # the resamplers load the built library on first use
    if name in ("Resampler", "StreamResampler", "SessionStreamResampler", "resample_clips", "resample_model",
                "ResampleSpec"):
        from . import resample
        return getattr(resample, name)
    # the score entries load the built library on first use
    if name in ("score_labels", "dilate_labels", "batch_score_labels", "batch_dilate_labels", "reference_labels",
                "batch_reference_labels", "histogram", "confusion", "roc", "roc_from_histogram", "threshold_at",
                "scores_from_logits", "BatchScores", "Roc"):
        from . import scores
        return getattr(scores, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
