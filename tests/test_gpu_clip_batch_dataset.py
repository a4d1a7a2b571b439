"""vad_amd.dataset.process_files (dataset_creator.py:19-73, a chunk of files
per call) against the per-file path it replaces: the CSV text of every chunk
equals, byte for byte, file_features per file -> torch.cat ->
scale_rows_device -> format_csv_rows."""
import io
import os
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# frames: 0 (empty), 0 (one frame's samples), 5 (no rows), 6 (one row), 70, 25, 9
WAV_LENS = [0, 400, 400 + 5 * 160, 400 + 5 * 160 + 1, 160 * 69 + 401, 4321, 1700]
STM = (b"talk 1 spk 0.0 0.25 <o,f0,male> some words\n"
       b"talk 1 spk 0.3 0.31 <o,f0,male> ignore_time_segment_in_scoring\n"
       b"talk 1 spk 0.4 0.4375 <o,f0,male> tail\n")


def write_wav(path, samples, rate=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(samples, "<i2").tobytes())


def write_sph(path, samples, rate=16000):
    """A SPHERE file as dataset/sph.py reads it: nine header lines, then
    big-endian 16-bit samples."""
    head = (f"NIST_1A\n   1024\nsample_count -i {len(samples)}\nsample_n_bytes -i 2\n"
            f"channel_count -i 1\nsample_byte_format -s2 10\nsample_rate -i {rate}\n"
            "sample_coding -s3 pcm\nend_head\n").encode()
    with open(path, "wb") as f:
        f.write(head + np.asarray(samples, ">i2").tobytes())


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from oracle import vad_oracle as O
    d = tmp_path_factory.mktemp("clips")
    for i, n in enumerate(WAV_LENS):
        write_wav(d / f"c{i:02d}.wav", O.synth_clip(n, seed=300 + i)[:n].astype(np.int16))
    write_sph(d / "talk.sph", O.synth_clip(9000, seed=320)[:9000].astype(np.int16))
    (d / "notes.txt").write_text("not audio\n")
    (d / "talk.stm").write_bytes(STM)
    return d


def per_file_text(paths, label, step, transcription_dir=None):
    import torch
    from vad_amd import dataset as D
    text, counts = [], []
    for lo in range(0, len(paths), step):
        feats = []
        for p in paths[lo:lo + step]:
            stm = None
            if transcription_dir is not None:
                stm = os.path.join(transcription_dir, os.path.basename(p).split(".")[0] + ".stm")
            feats.append(D.file_features(p, transcription_path=stm, device_out=True))
            counts.append(feats[-1].shape[0])
        rows = torch.cat(feats)
        D.scale_rows_device(rows)
        text.append(D.format_csv_rows(rows.cpu().numpy(), label))
    return "".join(text), counts


def test_process_files_equals_the_per_file_path(corpus):
    from vad_amd import dataset as D
    d = str(corpus)
    paths = D.list_audio_files([d])
    assert [os.path.basename(p) for p in paths] == [f"c{i:02d}.wav" for i in range(7)] + ["talk.sph"]  # notes.txt skipped
    want, want_counts = per_file_text(paths, 1, 3)
    assert want_counts == [0, 0, 0, 1, 65, 20, 4, 49] and want.count("\n") == sum(want_counts)
    out = io.StringIO()
    counts = D.process_files([d], 1, 100, out, files_per_step=3)
    assert counts == want_counts
    assert out.getvalue() == want
    # file paths instead of directories, another chunking and label
    out2 = io.StringIO()
    assert D.process_files(paths, 0, 100, out2, files_per_step=30) == want_counts
    assert out2.getvalue() == per_file_text(paths, 0, 30)[0] != want


def test_max_files_truncates(corpus):
    from vad_amd import dataset as D
    d = str(corpus)
    paths = D.list_audio_files([d], 5)
    assert len(paths) == 5
    out = io.StringIO()
    counts = D.process_files([d], 2, 5, out, files_per_step=3)
    want, want_counts = per_file_text(paths, 2, 3)
    assert counts == want_counts == [0, 0, 0, 1, 65] and out.getvalue() == want
    # a chunk whose files have no rows at all writes nothing and breaks nothing
    out = io.StringIO()
    assert D.process_files([d], 2, 3, out, files_per_step=3) == [0, 0, 0] and out.getvalue() == ""


def test_transcript_lookup_by_stem(corpus):
    from vad_amd import dataset as D
    d = str(corpus)
    sph = os.path.join(d, "talk.sph")
    out = io.StringIO()
    counts = D.process_files([sph], 1, 10, out, transcription_dir=d, files_per_step=3)
    want, want_counts = per_file_text([sph], 1, 3, transcription_dir=d)
    # 0.25 s and 0.0375 s at 16 kHz: 4000 + 600 samples -> 27 frames
    assert counts == want_counts == [22] and out.getvalue() == want
